// Per-pixel body of estimate_surface_normal (reference: gans/geometry.py:38-127), shared by surface_normal_kernel
// (geometry.hip, neighbours from global memory) and frame_points_kernel (frame.hip, neighbours from LDS): both inline
// THIS function, so the same nine points give the same bits in either.
//   the 8 neighbours at distance d in the reference's order, neighbour pairs (k, k+2):
//   mode 0 "closest": the pair with the smallest |p1-a| + |p2-a| (first minimum) gives n = (p1-a) x (p2-a)
//   mode 1 "mean":    n = mean_k (p1_k-a) x (p2_k-a)
//   out = n / (|n| + 1e-8)
#pragma once
#include "common.h"

// One rounding per operation, in the order written.  HIP's __fmul_rn / __fadd_rn / __fsub_rn do not give that: each is
// `x * y` (`+`, `-`) inside a header function, so the operation carries the translation unit's contract flag wherever
// it is inlined, a `#pragma clang fp contract(off)` in the caller does not reach it, and the backend fuses a product
// into the add or subtract that consumes it where it likes.  It chose differently in the two kernels that inline
// surface_normal_px: 1-ulp differences in a fifth of the normals, and the cross product of two identical vectors (a
// clamped row between equal medians) came out as a rounding residue ~1e-10, which n / (|n| + 1e-8) turns into ~1e-2,
// where the reference's float64 has 0.  These forms carry the pragma themselves.
__device__ __forceinline__ float fmul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fadd_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float fsub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ float norm3(float x, float y, float z) {
  // (x^2 + y^2) + z^2 without contraction: the order of the reference's reduction over the last axis
  return sqrtf(fadd_rn(fadd_rn(fmul_rn(x, x), fmul_rn(y, y)), fmul_rn(z, z)));
}

// (ax, ay, az): the pixel's own point.  fetch(dh, dw, x, y, z): the point of the neighbour dh, dw in {-1, 0, 1} steps
// of d away -- the caller owns the topology (replicate rows, circular columns) and where the points live.
template <typename Fetch>
__device__ __forceinline__ void surface_normal_px(float ax, float ay, float az, Fetch fetch, int mode, float& ox,
                                                  float& oy, float& oz) {
  const int dh[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dw[8] = {0, 1, 1, 1, 0, -1, -1, -1};
  float vx[8], vy[8], vz[8], nrm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float px, py, pz;
    fetch(dh[k], dw[k], px, py, pz);
    vx[k] = fsub_rn(px, ax);
    vy[k] = fsub_rn(py, ay);
    vz[k] = fsub_rn(pz, az);
    nrm[k] = norm3(vx[k], vy[k], vz[k]);
  }
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (mode == 0) {
    int best = 0;
    float bd = fadd_rn(nrm[0], nrm[2]);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float dk = fadd_rn(nrm[k], nrm[(k + 2) & 7]);
      if (dk < bd) { bd = dk; best = k; }   // strict: the first minimum wins, as torch.argmin on CPU
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k == best) {
        const int k2 = (k + 2) & 7;
        nx = fsub_rn(fmul_rn(vy[k], vz[k2]), fmul_rn(vz[k], vy[k2]));
        ny = fsub_rn(fmul_rn(vz[k], vx[k2]), fmul_rn(vx[k], vz[k2]));
        nz = fsub_rn(fmul_rn(vx[k], vy[k2]), fmul_rn(vy[k], vx[k2]));
      }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int k2 = (k + 2) & 7;
      nx = fadd_rn(nx, fsub_rn(fmul_rn(vy[k], vz[k2]), fmul_rn(vz[k], vy[k2])));
      ny = fadd_rn(ny, fsub_rn(fmul_rn(vz[k], vx[k2]), fmul_rn(vx[k], vz[k2])));
      nz = fadd_rn(nz, fsub_rn(fmul_rn(vx[k], vy[k2]), fmul_rn(vy[k], vx[k2])));
    }
    nx = nx / 8.f; ny = ny / 8.f; nz = nz / 8.f;
  }
  const float inv = 1.f / fadd_rn(norm3(nx, ny, nz), 1e-8f);
  ox = nx * inv;
  oy = ny * inv;
  oz = nz * inv;
}
