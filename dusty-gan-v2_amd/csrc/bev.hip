// Bird's-eye-view rendering of point clouds and the bilinear splat under it (include/dgv2.h, "Bird's-eye view", states
// the arithmetic; DESIGN.md section 37 the structure and the measurements).  gfx950 only.
//
// Three steps on the caller's stream: clear the accumulator, splat, resolve.
//   splat    one thread per (point, slot); slot k < C is colour channel k, slot C (render mode only) the denominator.  The
//            S = C + 1 lanes of a point repeat its projection (a few dozen flops) and then issue at most four atomics,
//            one per bilinear corner; a corner's S adds are S consecutive 64-bit words of acc [B, H, W, S], so a wave
//            instruction covers 64 / S points with one 8 S-byte segment each instead of 64 scattered words.
//   resolve  one thread per output element: num / (den + 1e-8) in double, rounded once to float (raster mode: num).
// The accumulator is 64-bit INTEGER: every addend (|a| <= 1, saturated) is scaled by 2^40 -- exact for a float -- rounded
// to an integer and added with an integer atomic.  Integer addition is associative, so the sums, and with them the
// output bits, depend neither on the arrival order of the atomics nor on the order of the points; N < 2^22 addends of at
// most 2^40 stay below 2^63.
// Built with -ffp-contract=off (Makefile): every operation of the projection below rounds on its own, as the header
// states it.
// A float becomes an index only behind a range comparison on the float itself: a NaN or huge coordinate fails the
// comparison and its point is dropped before any address is formed.
#include <math.h>

#include "common.h"

namespace {

constexpr int BEV_THREADS = 256;
constexpr int BEV_C_MAX = 4;
constexpr int BEV_N_MAX = 1 << 22;       // exclusive
constexpr float BEV_SCALE = 0x1p40f;     // accumulator units per 1.0
constexpr float BEV_W_MIN = 1e-3f;       // a corner with a smaller bilinear weight is dropped
constexpr float BEV_EPS = 1e-8f;

struct BevP {
  float* out;
  long long* acc;
  const float *pts, *val, *R, *t;   // pts: [B,N,3] points (render) or [B,N,2] raster coordinates (raster mode)
  int B, N, C, H, W;
  float focal;
};

// (row, col) raster coordinates, the depth weight e and the keep flag of one point; false: the point adds nothing
template <bool RENDER>
__device__ __forceinline__ bool bev_point(const BevP& p, int64_t pt, float& row, float& col, float& e, bool& keep) {
  if (!RENDER) {
    row = p.pts[pt * 2];
    col = p.pts[pt * 2 + 1];
    e = 1.f;
    keep = true;
    return true;
  }
  const float x = p.pts[pt * 3], y = p.pts[pt * 3 + 1], z = -p.pts[pt * 3 + 2];
  float px = x, py = y, pz = z;
  if (p.R) {   // row vector times matrix
    px = x * p.R[0] + y * p.R[3] + z * p.R[6];
    py = x * p.R[1] + y * p.R[4] + z * p.R[7];
    pz = x * p.R[2] + y * p.R[5] + z * p.R[8];
  }
  if (p.t) {
    px += p.t[0];
    py += p.t[1];
    pz += p.t[2];
  }
  const float size = (float)p.H;
  const float s = fabsf(pz) > BEV_EPS ? 1.f / (pz + BEV_EPS) : 1.f;
  const float ux = (px * s * p.focal + 0.5f) * size, uy = (py * s * p.focal + 0.5f) * size;
  keep = 0.f < ux && ux < size - 1.f && 0.f < uy && uy < size - 1.f;
  row = size - ux;
  col = size - uy;
  const float d = sqrtf(px * px + py * py + pz * pz);
  e = d > BEV_EPS ? expf(-3.f * d) : 0.f;
  return e > 0.f;   // (false for a NaN too)
}

template <bool RENDER>
__global__ __launch_bounds__(BEV_THREADS) void bev_splat_kernel(const BevP p, const int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (tid >= total) return;
  const int S = p.C + (RENDER ? 1 : 0);
  const int64_t pt = tid / S;
  const int k = (int)(tid - pt * S);
  float row, col, e;
  bool keep;
  if (!bev_point<RENDER>(p, pt, row, col, e, keep)) return;
  // the two corner rows are floor(row) and floor(row) + 1: outside this range neither is in the image (NaN: false)
  if (!(row >= -1.f && row < (float)p.H && col >= -1.f && col < (float)p.W)) return;
  float v = 1.f;   // the denominator slot
  if (k < p.C) {
    if (!keep) return;
    v = p.val[pt * p.C + k];
  }
  const float r0f = floorf(row), c0f = floorf(col);
  const int r0 = (int)r0f, c0 = (int)c0f;   // in [-1, H - 1] x [-1, W - 1]
  const float wr[2] = {(r0f + 1.f) - row, row - r0f}, wc[2] = {(c0f + 1.f) - col, col - c0f};
  long long* const acc = p.acc + (int64_t)(pt / p.N) * p.H * p.W * S + k;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + i;
    if (r < 0 || r >= p.H) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + j;
      const float b = wr[i] * wc[j];
      if (c < 0 || c >= p.W || !(b >= BEV_W_MIN)) continue;
      float a = (e * b) * v;
      a = fminf(fmaxf(a, -1.f), 1.f);   // the bound the 2^63 budget rests on (a NaN value becomes -1)
      const long long q = (long long)rintf(a * BEV_SCALE);
      if (q != 0)
        __hip_atomic_fetch_add(acc + ((int64_t)r * p.W + c) * S, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <bool RENDER>
__global__ __launch_bounds__(BEV_THREADS) void bev_resolve_kernel(const BevP p, const int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (tid >= total) return;   // total = B * C * H * W, out is [B, C, H, W]
  const int S = p.C + (RENDER ? 1 : 0);
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = tid % HW, bc = tid / HW;
  const int c = (int)(bc % p.C);
  const long long* const a = p.acc + ((bc / p.C) * HW + pix) * S;
  const double num = (double)a[c] * (1.0 / (double)BEV_SCALE);
  p.out[tid] = RENDER ? (float)(num / ((double)a[p.C] * (1.0 / (double)BEV_SCALE) + (double)BEV_EPS)) : (float)num;
}

template <bool RENDER> int bev_run(const BevP& p, hipStream_t st) {
  const int S = p.C + (RENDER ? 1 : 0);
  const int64_t n_splat = (int64_t)p.B * p.N * S, n_out = (int64_t)p.B * p.C * p.H * p.W;
  const int64_t g_splat = (n_splat + BEV_THREADS - 1) / BEV_THREADS, g_out = (n_out + BEV_THREADS - 1) / BEV_THREADS;
  if (g_splat > 0x7fffffffLL || g_out > 0x7fffffffLL) return DGV2_EINVAL;
  hipError_t e = hipMemsetAsync(p.acc, 0, (size_t)p.B * p.H * p.W * S * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  bev_splat_kernel<RENDER><<<(unsigned)g_splat, BEV_THREADS, 0, st>>>(p, n_splat);
  bev_resolve_kernel<RENDER><<<(unsigned)g_out, BEV_THREADS, 0, st>>>(p, n_out);
  DGV2_RETURN_LAST();
}

}  // namespace

extern "C" int dgv2_bev_render(float* out, int64_t* acc, const float* points, const float* colors, const float* R,
                               const float* t, int B, int N, int C, int size, float focal, void* stream) {
  if (!out || !acc || !points || !colors) return DGV2_EINVAL;
  if (B < 1 || N < 1 || N >= BEV_N_MAX || C < 1 || C > BEV_C_MAX || size < 1) return DGV2_EINVAL;
  BevP p;
  p.out = out; p.acc = reinterpret_cast<long long*>(acc); p.pts = points; p.val = colors; p.R = R; p.t = t;
  p.B = B; p.N = N; p.C = C; p.H = size; p.W = size; p.focal = focal;
  return bev_run<true>(p, (hipStream_t)stream);
}

extern "C" int dgv2_bilinear_splat(float* out, int64_t* acc, const float* coords, const float* values, int B, int N,
                                   int C, int H, int W, void* stream) {
  if (!out || !acc || !coords || !values) return DGV2_EINVAL;
  if (B < 1 || N < 1 || N >= BEV_N_MAX || C < 1 || C > BEV_C_MAX || H < 1 || W < 1) return DGV2_EINVAL;
  BevP p;
  p.out = out; p.acc = reinterpret_cast<long long*>(acc); p.pts = coords; p.val = values; p.R = nullptr; p.t = nullptr;
  p.B = B; p.N = N; p.C = C; p.H = H; p.W = W; p.focal = 1.f;
  return bev_run<false>(p, (hipStream_t)stream);
}
