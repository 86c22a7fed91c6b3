// Per-pixel range conversions (reference: gans/coords.py:73-185), shared by coords_kernel (tail_coords.hip) and
// frame_points_kernel (frame.hip): both inline THESE functions, so a pixel converts to the same bits in either.
#pragma once
#include "common.h"

__device__ __forceinline__ float inv_depth_norm_from_depth(float d, float min_d, float max_d) {
  const bool valid = (d >= min_d) && (d <= max_d) && (d > 0.f);
  return valid ? (1.f / (d + 1e-11f)) * min_d : 0.f;
}

__device__ __forceinline__ float depth_from_inv_depth_norm(float x, float min_d, float max_d) {
  const float inv = x / min_d;
  const bool valid = (inv >= 1.f / max_d) && (inv <= 1.f / min_d) && (inv > 0.f);
  return valid ? 1.f / (inv + 1e-11f) : 0.f;
}

// inv_depth_norm -> depth on the way to a point map (coords.py:142-146): the (x > tol) mask on top of get_mask's
__device__ __forceinline__ float depth_from_inv_depth_norm_tol(float x, float min_d, float max_d) {
  return (x > 1e-11f) ? depth_from_inv_depth_norm(x, min_d, max_d) : 0.f;
}

// depth_to_point_map (coords.py:178-185) at one pixel with laser angles (elev, azim)
__device__ __forceinline__ void point_from_depth(float d, float elev, float azim, float& x, float& y, float& z) {
  float se, ce, sa, ca;
  sincosf(elev, &se, &ce);
  sincosf(azim, &sa, &ca);
  x = d * ce * ca;
  y = d * ce * sa;
  z = d * se;
}
