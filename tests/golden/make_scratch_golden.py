#!/usr/bin/env python3
"""Generate tests/golden/scratch_sizes.json: the workspace sizes the built libdgv2.so reports (host calls, no GPU).

    make && python tests/golden/make_scratch_golden.py

The file is a list of {entry, args, elems}: `entry` is a `_scratch` entry of include/dgv2.h, `args` its arguments after
the `int64_t* elems` (a list stands for an int array), `elems` what it wrote -- 0 where it answered DGV2_ENOTSUP.  Any
other error code stops the script: such shapes belong to the error tests, not here.

The committed file was recorded at ABI 57, BEFORE six kernel entries lost their query mode: there the six `_scratch`
entries of QUERY_57 did not exist, and a row's number is what the Python layer formed then -- the count the kernel entry
reported in its `*_needed` argument times the per-block layout product of its call site.  From ABI 58 on the script asks
the `_scratch` entries themselves; tests/test_scratch_protocol.py holds the library to the recorded numbers.

CASES: for every entry the smallest shapes that reach each branch of its size formula, then the shapes of the
bench.py workload (batch 64, 64 x 512, 32 ... 512 channels).  None of the plan functions' environment switches
(DGV2_PW_BLOCKS, DGV2_MP_BLOCKS, DGV2_WS_*) may be set while recording.
"""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "..", "dusty-gan-v2_amd", "lib", "libdgv2.so")
OUT = os.path.join(HERE, "scratch_sizes.json")
F32, BF16 = 0, 1
ENOTSUP = -3

CASES = []


def case(entry, *rows):
    CASES.extend((entry, list(r)) for r in rows)


def both(*rows):
    return [(*r, dt) for r in rows for dt in (F32, BF16)]


# (B, H, W, C, O, k, stride, pad, dtype)
case("dgv2_conv_wgrad_stream_scratch", *both(
    (2, 8, 32, 32, 32, 3, 1, 1),          # k = 3 stride 1, small tiles
    (4, 16, 64, 64, 128, 3, 2, 1),        # k = 3 stride 2, O % 128 == 0: bf16 plans two o-groups per block (go == 2)
    (4, 16, 64, 64, 64, 3, 2, 1),         # ... O % 128 != 0: one o-group
    (2, 8, 32, 64, 64, 1, 1, 0),          # k = 1
    (2, 8, 32, 64, 64, 1, 2, 0),
    (4, 8, 64, 128, 128, 3, 1, 1),        # fp32 C, O >= 128: the wide tile
    (4, 8, 64, 128, 64, 3, 1, 1),         # fp32 just outside it
    (1, 4, 32, 32, 32, 3, 1, 1),          # one tile: the tile count caps the split
    (1, 3, 33, 8, 8, 3, 1, 1),            # odd sizes, two tiles
    (64, 64, 512, 32, 32, 3, 1, 1), (64, 64, 512, 32, 64, 3, 2, 1), (64, 64, 512, 32, 64, 1, 2, 0),
    (64, 32, 256, 64, 64, 3, 1, 1), (64, 32, 256, 64, 128, 3, 2, 1), (64, 16, 128, 128, 128, 3, 1, 1),
    (64, 16, 128, 128, 256, 3, 2, 1), (64, 8, 64, 256, 256, 3, 1, 1), (64, 8, 64, 256, 512, 3, 2, 1),
    (64, 4, 32, 512, 512, 3, 1, 1), (64, 4, 32, 544, 512, 3, 1, 1)))
# (B, H, W, C, O, dtype)
case("dgv2_bmm_tn_stream_scratch", *both(
    (8, 64, 256, 64, 32),                 # the two dtypes plan different tiles: 256 (fp32) against 512 (bf16) splits
    (2, 8, 32, 8, 8), (3, 5, 33, 8, 16),
    (64, 64, 512, 32, 32), (64, 32, 256, 64, 64), (64, 16, 128, 128, 128)))
# (B, H, W, C, clive, O): channel tails of 0, 1, 4, 16 past a multiple of 64 (and 2, 5: the tail kernel's next width)
case("dgv2_conv3x3_x3_wgrad_scratch",
     (2, 4, 32, 64, 64, 128), (2, 4, 32, 72, 65, 128), (2, 4, 32, 72, 68, 128), (2, 4, 32, 80, 80, 128),
     (2, 4, 32, 72, 66, 128), (2, 4, 32, 72, 69, 128),
     (1, 4, 32, 64, 64, 128),             # one tile
     (64, 8, 64, 136, 129, 256),          # more than 64 tiles: the tail slices stop at 64
     (2, 4, 32, 64, 64, 64),              # refused: O % 128
     (2, 4, 32, 96, 90, 128),             # refused: a tail of 26
     (2, 4, 48, 64, 64, 128),             # refused: W % 32
     (64, 4, 32, 544, 513, 512))
# (B, P, O, Ks)
case("dgv2_pe_wgrad_scratch",
     (16, 256, 8, 128), (16, 8192, 8, 128), (1, 4096, 128, 256),
     (64, 2048, 24, 512),                 # refused: O does not divide 128
     (3, 2048, 32, 512),                  # refused: B * O % 128
     (64, 32768, 32, 512), (64, 8192, 64, 512), (64, 2048, 128, 512))
# (B, C, out_h, out_w, Eh, dtype): out_h 4 / 8 / 32 choose the strip height, Eh >= 17 halves it (SH * Eh <= 64)
case("dgv2_resample_tab_actbwd_scratch", *both(
    *[(2, 32, oh, 33, eh) for oh in (4, 8, 32) for eh in (2, 20, 40)],
    (2, 32, 3, 5, 4), (1, 32, 64, 512, 64),
    (2, 24, 8, 32, 2),                    # refused: 3 (bf16) / 6 (fp32) channel vectors do not divide 256
    (2, 4, 8, 32, 2),                     # refused in bf16 (less than one vector), covered in fp32
    (2, 32, 8, 32, 65),                   # refused: Eh > 64
    (64, 32, 64, 512, 2), (64, 32, 64, 512, 4), (64, 64, 32, 256, 2), (64, 128, 16, 128, 2), (64, 256, 8, 64, 2),
    (64, 512, 4, 32, 4)))
# (B, C, H, W)
case("dgv2_fir_same_mfma_actbwd_scratch",
     (2, 32, 8, 32), (3, 64, 16, 96),
     (2, 32, 12, 32), (2, 32, 8, 48), (2, 16, 8, 32),   # refused: H % 8, W % 32, C % 32
     (64, 32, 64, 512), (64, 64, 32, 256))
# (H, W) -> BYTES of the band buffer
case("dgv2_fir_same_mfma_prep_scratch", (8, 32), (16, 96), (12, 32), (8, 48), (64, 512), (32, 256))
# (B, P, O, K, dtype); one grid plan for both entries
for _entry in ("dgv2_bmm_nn_small_act_scratch", "dgv2_head_bwd_scratch"):
    case(_entry, *both(
        (2, 100, 2, 32), (2, 1500, 2, 32),    # P small: nsplit clamped to the pixels
        (2, 100000, 1, 32), (3, 4097, 4, 64),  # unclamped; P no multiple of the split
        (4096, 64, 2, 32),                     # more samples than the block target
        (2, 100, 5, 32),                       # refused: O > 4
        (2, 100, 2, 24),                       # refused: 3 (bf16) / 6 (fp32) channel vectors do not divide 256
        (2, 100, 2, 4),                        # refused in bf16 (less than one vector), covered in fp32
        (64, 32768, 2, 32), (64, 8192, 2, 64), (64, 2048, 2, 128), (64, 512, 2, 256), (64, 128, 2, 512)))
# (B, P, K, dtype)
case("dgv2_modconv_pe_dgrad_actbwd_scratch",
     (2, 100, 32, BF16), (2, 100, 64, BF16), (300, 256, 32, BF16), (64, 32768, 32, BF16), (64, 8192, 64, BF16),
     (64, 2048, 128, BF16),               # refused: K = 128
     (2, 100, 32, F32))                   # refused: fp32
case("dgv2_fps_scratch", (2, 1024), (2, 32768), (2, 32769), (32, 2048), (4, 131072))   # (B, n)
case("dgv2_crf_rnn_backward_scratch", (2, 3, 5, 7, 1), (1, 8, 5, 70, 3), (8, 4, 64, 2048, 3))   # (B, C, H, W, iterations)
case("dgv2_seg_loss_scratch", (2, 9, 37), (8, 64, 2048))                                # (B, H, W)
case("dgv2_stem_bwd_scratch", (2, 8, 32, 8), (1, 3, 5, 64), (64, 64, 512, 32))           # (B, H, W, O)
# (O[L], I[L], B, L): the generator's modulated layers of one pass (conv0, conv1 with the PE columns, conv2, two heads)
_GEN_O = [512, 512, 1, 1] + [c for ch in (256, 128, 64, 32) for c in (ch, ch, ch, 1, 1)]
_GEN_I = [512 + 512, 512, 512, 512] + [i for ch in (256, 128, 64, 32) for i in (2 * ch, ch + 512, ch, ch, ch)]
case("dgv2_mod_prep_all_bwd_scratch", ([8], [8], 2, 1), ([5, 3], [12, 8], 3, 2), ([1, 1, 9], [32, 32, 4], 17, 3),
     (_GEN_O, _GEN_I, 64, len(_GEN_O)))

# ABI 57: kernel entry, its argument list in query mode (n: where the int64 count goes, then the row's own arguments by
# position), and the layout product of the Python call site of that time
_f, _z = ctypes.c_float(1.0), ctypes.c_int64(0)
QUERY_57 = {
    "dgv2_resample_tab_actbwd_scratch": (
        "dgv2_resample_tab_actbwd",
        lambda n, B, C, oh, ow, Eh, dt: (None, None, None, _z, n, None, None, None, None, None, Eh, None, None, None, 1, B, C,
                                         1, 1, oh, ow, _f, _f, dt, None),
        lambda cnt, B, C, oh, ow, Eh, dt: cnt * C),
    "dgv2_fir_same_mfma_actbwd_scratch": (
        "dgv2_fir_same_mfma_actbwd",
        lambda n, B, C, H, W: (None, None, None, _z, n, None, None, None, B, C, H, W, _f, _f, None),
        lambda cnt, B, C, H, W: cnt * C),
    "dgv2_fir_same_mfma_prep_scratch": (
        "dgv2_fir_same_mfma_prep",
        lambda n, H, W: (None, _z, n, None, None, None, 1, None, None, None, 1, H, W, None, None),
        lambda cnt, H, W: cnt),
    "dgv2_bmm_nn_small_act_scratch": (
        "dgv2_bmm_nn_small_act",
        lambda n, B, P, O, K, dt: (None, None, None, None, B, P, O, K, None, None, _f, _f, None, None, _z, n, dt, None),
        lambda cnt, B, P, O, K, dt: cnt * K),
    "dgv2_head_bwd_scratch": (
        "dgv2_head_bwd",
        lambda n, B, P, O, K, dt: (None, None, None, None, None, _z, n, None, None, None, None, None, None, _f, _f, B, P, O, K,
                                   dt, None),
        lambda cnt, B, P, O, K, dt: cnt * (K + O * K + O)),
    "dgv2_modconv_pe_dgrad_actbwd_scratch": (
        "dgv2_modconv_pe_dgrad_actbwd",
        lambda n, B, P, K, dt: (None, None, None, _z, n, None, None, None, None, _f, _f, B, P, K, dt, None),
        lambda cnt, B, P, K, dt: cnt * K),
}


def _c(a):
    return (ctypes.c_int * len(a))(*a) if isinstance(a, (list, tuple)) else a


def ask(lib, abi, entry, args):
    n = ctypes.c_int64(0)
    if abi <= 57 and entry in QUERY_57:
        kernel, query_args, product = QUERY_57[entry]
        rc = getattr(lib, kernel)(*query_args(ctypes.byref(n), *args))
        elems = product(n.value, *args)
    else:
        rc = getattr(lib, entry)(ctypes.byref(n), *[_c(a) for a in args])
        elems = n.value
    if rc == ENOTSUP:
        return 0
    if rc != 0:
        raise SystemExit(f"{entry}{tuple(args)}: error code {rc}; not a case for this file")
    return elems


def main():
    for v in ("DGV2_PW_BLOCKS", "DGV2_MP_BLOCKS", "DGV2_WS_NO_GO2", "DGV2_WS_GO2_S1", "DGV2_WS_BLOCKS_BIG",
              "DGV2_WS_BLOCKS_SMALL"):
        if v in os.environ:
            raise SystemExit(f"unset {v} first: it changes a plan")
    lib = ctypes.CDLL(LIB)
    abi = lib.dgv2_abi_version()
    rows = [dict(entry=e, args=a, elems=ask(lib, abi, e, a)) for e, a in CASES]
    got = {(r["entry"], json.dumps(r["args"])): r["elems"] for r in rows}
    tn = [got[("dgv2_bmm_tn_stream_scratch", json.dumps([8, 64, 256, 64, 32, dt]))] for dt in (F32, BF16)]
    assert tn[0] != tn[1], f"dgv2_bmm_tn_stream_scratch: the two dtypes agree at the key-test shape ({tn})"
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    refused = sum(r["elems"] == 0 for r in rows)
    print(f"ABI {abi}: {len(rows)} rows ({refused} of them 0) -> {OUT};  bmm_tn_stream fp32 / bf16: {tn}")


if __name__ == "__main__":
    main()
