// LiDAR beam upsampling: holding out beams of a scan with the interpolation baselines, and the depth scores of the
// held-out pixels (include/dgv2.h, "Beam upsampling", states the arithmetic; DESIGN.md section 41 the structure and the
// measurements).  gfx950 only.
//   dgv2_beam_split    one thread per pixel: the fitting mask, the scoring mask and (modes 1 / 2) the pixel's value
//                      interpolated between the two observed rows around it.  A thread reads at most five words and
//                      writes four; there is no sum, so nothing depends on the grid.
//   dgv2_depth_score   one 1024-thread block per image, eight float64 sums.
// Order of an image's sums (n pixels, groups of 4 counted from the image's first pixel): thread t owns groups t,
// t + 1024, ...; the pixels of a group are added in index order, group after group, to the thread's eight accumulators;
// the n % 4 tail pixels go one each to threads 0 .. n % 4 - 1, after the groups; a wave folds its 64 totals with the xor
// butterfly 32, 16, ..., 1; the sixteen wave sums are added in wave order.  An image whose three addresses are 16-byte
// aligned reads each group with one 16-byte load per array, any other image reads the SAME groups element by element:
// the order depends on n alone -- not on B, the image's place in the batch or its address.  A pixel whose mask is 0 adds
// nothing (it is skipped, not multiplied: its terms may be NaN).
// Built with -ffp-contract=off (Makefile): every float32 operation below rounds on its own, as the header states it;
// `/` is HIP's correctly rounded float32 division.
#include <math.h>

#include "common.h"

namespace {

constexpr int SPLIT_THREADS = 256;
constexpr int SCORE_THREADS = 1024;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_SUMS = 8;

struct SplitP {
  float *recon, *recon_mask, *obs, *held;
  const float *depth, *valid;
  int H, W, factor, offset;
};

template <int MODE>
__global__ __launch_bounds__(SPLIT_THREADS) void beam_split_kernel(const SplitP p, const int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  if (tid >= total) return;
  const int h = (int)((tid / p.W) % p.H);
  const bool v = p.valid ? p.valid[tid] != 0.f : true;
  const int r = h % p.factor;
  const bool seen = r == p.offset;
  p.obs[tid] = seen && v ? 1.f : 0.f;
  p.held[tid] = !seen && v ? 1.f : 0.f;
  if (MODE == 0) return;
  // the observed rows around h: lo <= h <= hi, both on the lattice offset + k factor; lo == hi == h on an observed row
  const int lo = r >= p.offset ? h - (r - p.offset) : h - (r - p.offset) - p.factor;   // < 0: none
  const int hi = seen ? h : lo + p.factor;                                              // >= H: none
  const int64_t base = tid - (int64_t)h * p.W;   // (b, 0, w)
  float d_lo = 0.f, d_hi = 0.f;
  bool v_lo = false, v_hi = false;
  if (lo >= 0) {
    const int64_t i = base + (int64_t)lo * p.W;
    v_lo = p.valid ? p.valid[i] != 0.f : true;
    d_lo = p.depth[i];
  }
  if (hi < p.H) {
    if (hi == lo) {
      v_hi = v_lo;
      d_hi = d_lo;
    } else {
      const int64_t i = base + (int64_t)hi * p.W;
      v_hi = p.valid ? p.valid[i] != 0.f : true;
      d_hi = p.depth[i];
    }
  }
  float out = 0.f;
  if (MODE == 2) {
    if (v_lo && v_hi) {
      const float t = (float)(h - lo) / (float)p.factor;
      out = hi == lo ? d_lo : d_lo + t * (d_hi - d_lo);
    } else if (v_lo) {
      out = d_lo;
    } else if (v_hi) {
      out = d_hi;
    }
  } else {
    // the nearer row, a tie to lo; a row that does not exist is never the nearer one
    const bool lo_first = lo >= 0 && (hi >= p.H || h - lo <= hi - h);
    if (lo_first) out = v_lo ? d_lo : (v_hi ? d_hi : 0.f);
    else out = v_hi ? d_hi : (v_lo ? d_lo : 0.f);
  }
  p.recon[tid] = out;
  p.recon_mask[tid] = v_lo || v_hi ? 1.f : 0.f;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one pixel's eight addends, each a float32 product with the weight, into the thread's float64 accumulators
__device__ __forceinline__ void score_pixel(double (&acc)[SCORE_SUMS], float ref, float gen, float m) {
  if (m == 0.f) return;
  const float r = ref + 1e-8f, g = gen + 1e-8f;
  const float d = r - g;
  const float dd = d * d;
  const float l = logf(r) - logf(g);
  const float q1 = ref / gen, q2 = gen / ref;   // delta = max(q1, q2); delta < thr iff both are (a NaN: neither)
  acc[0] += (double)(m * (fabsf(d) / r));
  acc[1] += (double)(m * (dd / r));
  acc[2] += (double)(m * dd);
  acc[3] += (double)(m * (l * l));
  acc[4] += (double)(m * (q1 < 1.25f && q2 < 1.25f ? 1.f : 0.f));
  acc[5] += (double)(m * (q1 < 1.5625f && q2 < 1.5625f ? 1.f : 0.f));
  acc[6] += (double)(m * (q1 < 1.953125f && q2 < 1.953125f ? 1.f : 0.f));
  acc[7] += (double)m;
}

__global__ __launch_bounds__(SCORE_THREADS) void depth_score_kernel(double* __restrict__ sums, const float* __restrict__ ref,
                                                                    const float* __restrict__ gen,
                                                                    const float* __restrict__ mask, const int64_t n) {
  __shared__ double red[SCORE_WAVES * SCORE_SUMS];
  const int64_t img = blockIdx.x;
  const float* __restrict__ rp = ref + img * n;
  const float* __restrict__ gp = gen + img * n;
  const float* __restrict__ mp = mask ? mask + img * n : nullptr;
  double acc[SCORE_SUMS];
#pragma unroll
  for (int k = 0; k < SCORE_SUMS; ++k) acc[k] = 0.0;
  const int64_t ng = n / 4;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(rp) | reinterpret_cast<uintptr_t>(gp) | reinterpret_cast<uintptr_t>(mp);
  if ((bits & 15) == 0) {
#pragma unroll 2
    for (int64_t i = threadIdx.x; i < ng; i += SCORE_THREADS) {
      const float4 r4 = reinterpret_cast<const float4*>(rp)[i], g4 = reinterpret_cast<const float4*>(gp)[i];
      const float4 m4 = mp ? reinterpret_cast<const float4*>(mp)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
      score_pixel(acc, r4.x, g4.x, m4.x);
      score_pixel(acc, r4.y, g4.y, m4.y);
      score_pixel(acc, r4.z, g4.z, m4.z);
      score_pixel(acc, r4.w, g4.w, m4.w);
    }
  } else {
    for (int64_t i = threadIdx.x; i < ng; i += SCORE_THREADS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) score_pixel(acc, rp[4 * i + j], gp[4 * i + j], mp ? mp[4 * i + j] : 1.f);
    }
  }
  const int64_t i = ng * 4 + threadIdx.x;
  if (i < n) score_pixel(acc, rp[i], gp[i], mp ? mp[i] : 1.f);
#pragma unroll
  for (int k = 0; k < SCORE_SUMS; ++k) acc[k] = wave_sum_f64(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < SCORE_SUMS; ++k) red[(threadIdx.x >> 6) * SCORE_SUMS + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < SCORE_SUMS) {
    double s = red[threadIdx.x];
    for (int w = 1; w < SCORE_WAVES; ++w) s += red[w * SCORE_SUMS + threadIdx.x];
    sums[img * SCORE_SUMS + threadIdx.x] = s;
  }
}

}  // namespace

extern "C" int dgv2_beam_split(float* recon, float* recon_mask, float* obs, float* held, const float* depth,
                               const float* valid, int B, int H, int W, int factor, int offset, int mode, void* stream) {
  if (!obs || !held || !depth) return DGV2_EINVAL;
  if (B < 1 || H < 1 || W < 1 || factor < 1 || factor > H || offset < 0 || offset >= factor) return DGV2_EINVAL;
  if (mode < 0 || mode > 2 || (mode != 0 && (!recon || !recon_mask))) return DGV2_EINVAL;
  const int64_t total = (int64_t)B * H * W;
  const int64_t grid = (total + SPLIT_THREADS - 1) / SPLIT_THREADS;
  if (grid > 0x7fffffffLL) return DGV2_EINVAL;
  SplitP p;
  p.recon = recon; p.recon_mask = recon_mask; p.obs = obs; p.held = held; p.depth = depth; p.valid = valid;
  p.H = H; p.W = W; p.factor = factor; p.offset = offset;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) beam_split_kernel<0><<<(unsigned)grid, SPLIT_THREADS, 0, st>>>(p, total);
  else if (mode == 1) beam_split_kernel<1><<<(unsigned)grid, SPLIT_THREADS, 0, st>>>(p, total);
  else beam_split_kernel<2><<<(unsigned)grid, SPLIT_THREADS, 0, st>>>(p, total);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_depth_score(double* sums, const float* ref, const float* gen, const float* mask, int B, int64_t n,
                                void* stream) {
  if (!sums || !ref || !gen) return DGV2_EINVAL;
  if (B < 1 || n < 1 || n > 0x7fffffffLL) return DGV2_EINVAL;
  depth_score_kernel<<<(unsigned)B, SCORE_THREADS, 0, (hipStream_t)stream>>>(sums, ref, gen, mask, n);
  DGV2_RETURN_LAST();
}
