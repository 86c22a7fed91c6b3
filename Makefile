# Builds libdgv2.so (HIP kernels for gfx950 behind the C ABI of include/dgv2.h).  hipcc cross-compiles without a GPU.
# `make ABLATE=1` compiles the benchmark-only ablation switches (DGV2_*_ABLATE: skip stores / MFMA loops; WRONG results)
# into the kernels; the default build has none of them.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := dusty-gan-v2_amd
SRC := $(wildcard $(PKG)/csrc/*.hip)
# `make BUILD=build_x LIB=build_x/libdgv2.so EXTRA=-DDGV2_...` builds an experiment variant beside the shipped library
# (DGV2_LIB_PATH points the binding at it for same-box A/B runs).
BUILD ?= build
OBJ := $(patsubst $(PKG)/csrc/%.hip,$(BUILD)/%.o,$(SRC))
LIB ?= $(PKG)/lib/libdgv2.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -Iinclude $(if $(ABLATE),-DDGV2_ABLATE) $(if $(FIR_RS),-DDGV2_FIR_RS=$(FIR_RS)) $(EXTRA)

all: $(LIB)

# Every object is assembled from the ISA the audit below has read (-save-temps=obj keeps that .s next to the object):
# hipcc's hazard recogniser does not look inside `asm`, so a compiler-generated VALU write into a register an asm-issued
# MFMA is still reading -- or a read of its result in flight -- goes unpadded.
# scripts/audit_asm_mfma.py scans the ISA for exactly that and FAILS THE BUILD on a finding, whatever the flags
# (EXTRA=, ABLATE=1, another ARCH, a compiler upgrade); sources without asm MFMAs pass trivially.
PYTHON ?= python3
$(BUILD)/%.o: $(PKG)/csrc/%.hip $(wildcard $(PKG)/csrc/*.h) include/dgv2.h scripts/audit_asm_mfma.py
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -save-temps=obj -c $< -o $@
	@$(PYTHON) scripts/audit_asm_mfma.py $(BUILD)/$*-hip-amdgcn-amd-amdhsa-$(ARCH).s > $(BUILD)/$*.audit \
	  || { cat $(BUILD)/$*.audit; echo "asm-MFMA hazard audit FAILED for $<"; rm -f $@; exit 1; }
	@rm -f $(BUILD)/$*-hip-*.bc $(BUILD)/$*-hip-*.hipi $(BUILD)/$*-hip-*.out $(BUILD)/$*-hip-*.out.resolution.txt \
	  $(BUILD)/$*-host-*.bc $(BUILD)/$*-host-*.hipi $(BUILD)/$*-host-*.s $(BUILD)/$*.hip-hip-*.hipfb $(BUILD)/$*-hip-*.o

# knn.hip is bound by vector-instruction issue, and the SLP vectoriser makes it worse there: it pairs the distance taps
# into v_pk_add / v_pk_fma, which have no |x| operand modifier, and pays for the sign masks and the register pairing
# (3987 against 3001 vector instructions, 151 against 124 VGPRs and 110 against 71 us at 5 x 5)
$(BUILD)/knn.o: HIPFLAGS += -fno-slp-vectorize

# segloss.hip promises the same bits from its vector and element-wise paths and from every dtype instantiation: no
# instantiation may fuse a multiply into an add that another leaves alone
$(BUILD)/segloss.o: HIPFLAGS += -ffp-contract=off

# sgd.hip promises the same bits from its 16-byte and element-wise paths (its fused multiply-adds are written out)
$(BUILD)/sgd.o: HIPFLAGS += -ffp-contract=off

# bev.hip states its projection per operation in float32 (include/dgv2.h "Bird's-eye view"): (p s focal + 0.5) size is
# two roundings, not a fused multiply-add that float32 restatements of the contract would not make
$(BUILD)/bev.o: HIPFLAGS += -ffp-contract=off

# latent.hip states Adam's update per operation in float32 (include/dgv2.h "Latent fitting"): m / denom is rounded before
# it is scaled and subtracted, as torch's addcdiv_ rounds it
$(BUILD)/latent.o: HIPFLAGS += -ffp-contract=off

# syncbn.hip promises the same bits from its 16-byte and element-wise paths and from every split of a batch over ranks:
# no instantiation may fuse a float64 multiply into an add that another leaves alone
$(BUILD)/syncbn.o: HIPFLAGS += -ffp-contract=off

# upsample.hip states both entries per operation in float32 (include/dgv2.h "Beam upsampling"): d_lo + t (d_hi - d_lo) is
# three roundings and m * (d d / r) three more, which the tests restate with separately rounded torch ops, and its
# 16-byte and element-wise paths must round alike
$(BUILD)/upsample.o: HIPFLAGS += -ffp-contract=off

$(LIB): $(OBJ)
	@mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ)

clean:
	rm -rf $(BUILD) $(LIB)

.PHONY: all clean
