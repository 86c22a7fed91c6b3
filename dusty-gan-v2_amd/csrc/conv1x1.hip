// conv1x1.hip -- the 1x1 stride-1 conv of channels-last bf16 activations as a streaming GEMM.
//
//   out[n, m] = bf16( sum_k in[n, k] * w[m, k]  (+ resid[n, m]) ),   n over the B * P pixels
//
// Forward (in = x, k = C, m = O, w = the weight bank's forward layout [O, C]) and data gradient (in = gy, k = O, m = C,
// w = the bank's transposed layout [C, O]) are the same product, so they share one kernel.  The general direct engine
// (conv_direct.hip) runs this shape through its halo tiles, tap lists and ring logic; here there is nothing but the
// product:
//   * a block owns one slab of 16 * MF output channels (blockIdx.y) and keeps the slab's weights [16 MF][K] in LDS for
//     its whole life (rows padded by one 16-byte slot); the grid is sized to the CUs and every wave walks over 32-pixel
//     tiles with the grid's stride;
//   * the activations never touch LDS: a lane's 16-byte global load (8 consecutive channels of one pixel) IS its B
//     fragment of v_mfma_f32_16x16x32_bf16 (B[k = 8 (lane >> 4) + j][col = lane & 15]); the weights are the A operand, so a
//     lane's four accumulator registers are four consecutive output channels of one pixel;
//   * K runs ascending into one accumulator per fragment, each K-step in the direct engine's own operand order, so
//     the fp32 sums are the direct engine's bit for bit; two fragments trade halves across 16-lane rows (pack_pair_bf16)
//     so that a lane owns 8 consecutive channels, the residual (one 16-byte load, issued ahead of the product) is added
//     to the rounded product exactly as the direct engine adds it, and the result leaves as one 16-byte store: a
//     training step computes the same bits on either engine;
//   * a ragged last tile clamps its pixel index for the loads (a valid address; the column it feeds is never stored)
//     and predicates the stores.
#include "common.h"

namespace {

constexpr int kPixTile = 32;   // pixels per wave tile: two 16-pixel MFMA column blocks
constexpr int kWaves = 4;
constexpr int kMaxK = 512;

struct C1Params {
  bf16_t* out;
  const bf16_t* in;
  const bf16_t* w;
  const bf16_t* resid;
  int64_t N;   // pixels
  int K, M;
  int nt;      // streaming stores (large outputs that no residual read revisits)
};

// MF: 16-channel fragments per slab (2 or 4); KC: K-steps loaded together (K % (32 KC) == 0)
template <int MF, int KC>
__global__ __launch_bounds__(256, 4) void conv1x1_kernel(const C1Params p) {
  extern __shared__ uint4 s_w[];   // [16 MF][K / 8 + 1] 16-byte slots
  const int K = p.K, M = p.M;
  const int kslots = K >> 3, rs = kslots + 1;
  const int m0 = blockIdx.y * (16 * MF);
  // four independent 16-byte loads per thread and round (one round trip per 16 KB, not per 4 KB); an index past the slab
  // is clamped to the slab's last slot, which is then copied again (same value, same place: no branch around a load)
  const int wslots = 16 * MF * kslots;
  for (int i0 = threadIdx.x; i0 < wslots; i0 += 4 * 256) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + u * 256, wslots - 1);
      v[u] = *reinterpret_cast<const uint4*>(p.w + (int64_t)m0 * K + (int64_t)i * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + u * 256, wslots - 1);
      s_w[(i / kslots) * rs + i % kslots] = v[u];
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lc = lane >> 4;
  const int co = (lc & 1) ? 16 + 4 * (lc - 1) : 4 * lc;   // channel offset of the lane's 8-channel run inside a fragment pair
  const int64_t ntiles = (p.N + kPixTile - 1) / kPixTile;
  const int ksteps = K >> 5;

  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < ntiles; t += (int64_t)gridDim.x * kWaves) {
    int64_t pix[2];
    const bf16_t* ip[2];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      pix[nf] = t * kPixTile + nf * 16 + lr;
      const int64_t pc = pix[nf] < p.N ? pix[nf] : p.N - 1;   // ragged tile: a valid row, its column is never stored
      ip[nf] = p.in + pc * K + lc * 8;
    }
    uint4 rr[2][MF / 2];
    if (p.resid) {
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const int64_t pc = pix[nf] < p.N ? pix[nf] : p.N - 1;
#pragma unroll
        for (int mp = 0; mp < MF / 2; ++mp)
          rr[nf][mp] = *reinterpret_cast<const uint4*>(p.resid + pc * M + m0 + mp * 32 + co);
      }
    }
    f32x4 acc[MF][2];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < ksteps; k0 += KC) {
      bf16x8 b[KC][2];
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) b[kc][nf] = *reinterpret_cast<const bf16x8*>(ip[nf] + (k0 + kc) * 32);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          union { uint4 u; bf16x8 v; } a;
          a.u = s_w[(mf * 16 + lr) * rs + (k0 + kc) * 4 + lc];
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
            acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b[kc][nf], acc[mf][nf], 0, 0, 0);
        }
      }
    }

#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
      for (int mp = 0; mp < MF / 2; ++mp) {
        float fa[4], fb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          fa[r] = acc[2 * mp][nf][r];
          fb[r] = acc[2 * mp + 1][nf][r];
        }
        vec16<bf16_t> v;
        pack_pair_bf16(fa, fb, lc, v.raw);   // every lane takes part in the exchange
        if (p.resid) {   // added to the ROUNDED product, as the direct engine adds it: the two engines agree bit for bit
          vec16<bf16_t> r;
          r.raw = rr[nf][mp];
#pragma unroll
          for (int j = 0; j < 8; ++j) v.set(j, v.get(j) + r.get(j));
        }
        if (pix[nf] < p.N) {
          bf16_t* q = p.out + pix[nf] * M + m0 + mp * 32 + co;
          if (p.nt) v.store_nt(q); else v.store(q);
        }
      }
    }
  }
}

int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

template <int MF, int KC>
int launch(const C1Params& p, hipStream_t st) {
  const size_t lds = (size_t)16 * MF * (p.K / 8 + 1) * 16;
  static bool attr = false;   // per instantiation: slabs past 64 KB of LDS (K = 512, 64 channels)
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_kernel<MF, KC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            16 * MF * (kMaxK / 8 + 1) * 16) != hipSuccess)
      return DGV2_EINVAL;
    attr = true;
  }
  const int slabs = p.M / (16 * MF);
  const int64_t want = (p.N + kPixTile * kWaves - 1) / (kPixTile * kWaves);
  // resident blocks: four per CU by registers, fewer where the weight slabs fill the 160 KB of LDS
  int per_cu = (int)((160 * 1024) / (lds + 512));
  per_cu = per_cu > 4 ? 4 : per_cu;
  int64_t gx = ((int64_t)device_cus() * per_cu + slabs - 1) / slabs;
  gx = gx < want ? gx : want;
  conv1x1_kernel<MF, KC><<<dim3((unsigned)gx, (unsigned)slabs), 256, lds, st>>>(p);
  DGV2_RETURN_LAST();
}

// out [N, M] = in [N, K] w[M, K]^T (+ resid [N, M])
int conv1x1_run(void* out, const void* in, const void* w, const void* resid, int64_t N, int K, int M, int dtype,
                hipStream_t st) {
  if (!out || !in || !w || N <= 0 || K <= 0 || M <= 0) return DGV2_EINVAL;
  if (dtype != DGV2_BF16 || K % 32 || M % 32 || K > kMaxK || !aligned16(out) || !aligned16(in) || !aligned16(w)
      || (resid && !aligned16(resid)))
    return DGV2_ENOTSUP;
  C1Params p;
  p.out = reinterpret_cast<bf16_t*>(out);
  p.in = reinterpret_cast<const bf16_t*>(in);
  p.w = reinterpret_cast<const bf16_t*>(w);
  p.resid = reinterpret_cast<const bf16_t*>(resid);
  p.N = N; p.K = K; p.M = M;
  p.nt = (!resid && nt_output(N * M * (int64_t)sizeof(bf16_t))) ? 1 : 0;
  const int kc = K % 128 == 0 ? 4 : K % 64 == 0 ? 2 : 1;
  if (M % 64 == 0) {
    if (kc == 4) return launch<4, 4>(p, st);
    if (kc == 2) return launch<4, 2>(p, st);
    return launch<4, 1>(p, st);
  }
  if (kc == 4) return launch<2, 4>(p, st);
  if (kc == 2) return launch<2, 2>(p, st);
  return launch<2, 1>(p, st);
}

}  // namespace

extern "C" int dgv2_conv1x1_fwd(void* y, const void* x, const void* wf, int B, int P, int C, int O, const void* resid,
                                int dtype, void* stream) {
  if (B <= 0 || P <= 0) return DGV2_EINVAL;
  return conv1x1_run(y, x, wf, resid, (int64_t)B * P, C, O, dtype, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dgv2_conv1x1_dgrad(void* gx, const void* gy, const void* wt, int B, int P, int C, int O, const void* resid,
                                  int dtype, void* stream) {
  if (B <= 0 || P <= 0) return DGV2_EINVAL;
  return conv1x1_run(gx, gy, wt, resid, (int64_t)B * P, O, C, dtype, reinterpret_cast<hipStream_t>(stream));
}
