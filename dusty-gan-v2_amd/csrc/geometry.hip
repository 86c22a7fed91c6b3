// Surface normals of a coordinated point map (range image of xyz points).
// Reference: estimate_surface_normal, gans/geometry.py:38-127 -- replicate padding along H, circular along W,
// the 8 neighbours at distance d in the reference's order, neighbour pairs (k, k+2):
//   mode 0 "closest": the pair with the smallest |p1-a| + |p2-a| (first minimum) gives n = (p1-a) x (p2-a)
//   mode 1 "mean":    n = mean_k (p1_k-a) x (p2_k-a)
//   out = n / (|n| + 1e-8)
// The reference gathers three [B,8,H,W,3] tensors with advanced indexing (~30 launches, 25x the input in
// intermediates); here one thread owns a pixel and reads its 9 points (NCHW planes, coalesced along W).
#include "common.h"
#include "normal_dev.h"

namespace {

// The per-pixel arithmetic is surface_normal_px (normal_dev.h), which the one-launch frame kernel (frame.hip) inlines too.
__global__ __launch_bounds__(256) void surface_normal_kernel(float* __restrict__ out, const float* __restrict__ pts,
                                                             int B, int H, int W, int d, int mode) {
  const int64_t total = (int64_t)B * H * W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int w = (int)(i % W);
  const int h = (int)((i / W) % H);
  const int b = (int)(i / ((int64_t)W * H));
  const int64_t plane = (int64_t)H * W;
  const float* pb = pts + (int64_t)b * 3 * plane;
  const float ax = pb[(int64_t)h * W + w], ay = pb[plane + (int64_t)h * W + w], az = pb[2 * plane + (int64_t)h * W + w];
  float nx, ny, nz;
  surface_normal_px(
      ax, ay, az,
      [&](int dh, int dw, float& x, float& y, float& z) {
        const int hh = min(max(h + dh * d, 0), H - 1);
        int ww = (w + dw * d) % W;
        ww = ww < 0 ? ww + W : ww;
        const int64_t o = (int64_t)hh * W + ww;
        x = pb[o];
        y = pb[plane + o];
        z = pb[2 * plane + o];
      },
      mode, nx, ny, nz);
  float* ob = out + (int64_t)b * 3 * plane + (int64_t)h * W + w;
  ob[0] = nx;
  ob[plane] = ny;
  ob[2 * plane] = nz;
}

}  // namespace

// points / out fp32 [B, 3, H, W] (NCHW as in the module API); d >= 1 (d < W); mode 0 = "closest", 1 = "mean".
extern "C" int dgv2_surface_normal(float* out, const float* points, int B, int H, int W, int d, int mode, void* stream) {
  if (!out || !points || B <= 0 || H <= 0 || W <= 0 || d < 1 || d >= W || (mode != 0 && mode != 1)) return DGV2_EINVAL;
  const int64_t total = (int64_t)B * H * W;
  if (total >= (1LL << 39)) return DGV2_EINVAL;
  surface_normal_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(out, points, B, H, W, d, mode);
  DGV2_RETURN_LAST();
}
