// Frame post-processing of a latent walk (reference: demo_interpolation.py:20-34, 79-86; gans/utils.py:167-191).
//
//  * dgv2_frame_points: generator image -> point cloud + normal colours in ONE launch.  Per pixel, in the reference's
//    order: x = (image + 1) / 2; inv_depth_norm -> point_map (coords_dev.h, the functions of dgv2_coords_convert mode
//    2); 3x3 median of each coordinate; points = median / max_depth; normals of points (d = 2, "closest", replicate
//    rows, circular columns: normal_dev.h, the function of dgv2_surface_normal); colours = (-n, NaN -> 0, + 1) / 2.
//    The tensor-op form is ten launches over [B,3,H,W] intermediates plus a [B,27,H*W] unfold and a sort.
//
//    A block owns a TH x TW tile of one frame and works in LOGICAL coordinates (lh, lw) around it, which may lie
//    outside the image; a logical pixel stands for the image pixel (clamp(lh, 0, H-1), lw mod W) -- the topology of
//    the normal's neighbours, and of every other stencil of this library.
//      stage 1  raw[i][j]: the converted point of logical pixel (h0-3+i, w0-3+j), tile + halo 3;
//      stage 2  med[i][j]: points (median / max_depth) of logical pixel (h0-2+i, w0-2+j), tile + halo 2: the median AT
//               THE MAPPED PIXEL (ph, pw), over ITS window (ph+dy, pw+dx).  Under border 0 a window position outside
//               the image is 0.0 whatever the raw stage holds there -- so the normal's neighbour at a clamped row or a
//               wrapped column sees the true image edge, not a median over a padded copy of the raw map.  Under
//               border 1 the window itself follows the clamp / wrap, which is what the raw stage holds;
//      stage 3  normals of the tile from med, both outputs in point-set layout.
//    Why stage 2 finds its window in raw: columns, lw + dx is staged (|dx| <= 1 inside halo 3) and (lw + dx) mod W =
//    (pw + dx) mod W.  Rows, the window is read at logical rows ph + dy: ph = clamp(lh) lies in [h0 - 2, h0 + TH + 1]
//    (lh < 0 only for h0 = 0, where ph = 0; lh >= H only where H - 1 >= h0), so ph + dy is inside the staged rows
//    [h0 - 3, h0 + TH + 3), and that row holds clamp(ph + dy).  No case needs H or W to reach the halo or the tile:
//    W = 3, H = 1 run the same code.
//    A nine-value selection has a unique middle: the median is an input value bit for bit (two zeros of opposite sign
//    compare equal; which one is selected is not defined, as with a sort).
//
//  * dgv2_colorize: idx = (long) clamp(x * N, 0, N - 1), out[b, :, h, w] = lut[idx] (a gather; NaN -> entry 0).
#include "common.h"
#include "coords_dev.h"
#include "normal_dev.h"

namespace {

constexpr int TH = 8, TW = 64, NT = 256, D = 2;
constexpr int RH = TH + 6, RW = TW + 6;   // raw points: tile + halo 3
constexpr int MH = TH + 4, MW = TW + 4;   // medians: tile + halo 2

__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// median of nine by the 19-exchange selection network (Paeth, Graphics Gems I, "Median finding on a 3x3 grid")
__device__ __forceinline__ float median9(float (&p)[9]) {
  cswap(p[1], p[2]); cswap(p[4], p[5]); cswap(p[7], p[8]);
  cswap(p[0], p[1]); cswap(p[3], p[4]); cswap(p[6], p[7]);
  cswap(p[1], p[2]); cswap(p[4], p[5]); cswap(p[7], p[8]);
  cswap(p[0], p[3]); cswap(p[5], p[8]); cswap(p[4], p[7]);
  cswap(p[3], p[6]); cswap(p[1], p[4]); cswap(p[2], p[5]);
  cswap(p[4], p[7]); cswap(p[4], p[2]); cswap(p[6], p[4]);
  cswap(p[4], p[2]);
  return p[4];
}

__global__ __launch_bounds__(NT) void frame_points_kernel(float* __restrict__ points, float* __restrict__ colors,
                                                          const float* __restrict__ image,
                                                          const float* __restrict__ angle, int H, int W, int tiles_h,
                                                          int tiles_w, float min_d, float max_d, float inv_max_d,
                                                          int border) {
  __shared__ float raw[3][RH][RW];
  __shared__ float med[3][MH][MW];
  const int tile = blockIdx.x % (tiles_h * tiles_w);
  const int64_t b = blockIdx.x / (tiles_h * tiles_w);
  const int h0 = (tile / tiles_w) * TH, w0 = (tile % tiles_w) * TW;
  const int HW = H * W;   // < 2^31 (checked by the entry)
  const float* img = image + b * HW;

  for (int idx = threadIdx.x; idx < RH * RW; idx += NT) {
    const int i = idx / RW, j = idx % RW;
    const int ph = min(max(h0 - 3 + i, 0), H - 1), pw = floormod(w0 - 3 + j, W);
    const int p = ph * W + pw;
    const float x = fmul_rn(fadd_rn(img[p], 1.f), 0.5f);   // tanh_to_sigmoid: (image + 1) / 2
    const float d = depth_from_inv_depth_norm_tol(x, min_d, max_d);
    point_from_depth(d, angle[p], angle[HW + p], raw[0][i][j], raw[1][i][j], raw[2][i][j]);
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < MH * MW; idx += NT) {
    const int i = idx / MW, j = idx % MW;
    const int ph = min(max(h0 - 2 + i, 0), H - 1), pw = floormod(w0 - 2 + j, W);
    const int ri = ph - (h0 - 3), rj = j + 1;   // the mapped pixel's row, the logical pixel's column, in raw
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = ph + t / 3 - 1, ww = pw + t % 3 - 1;
      in[t] = border != 0 || (hh >= 0 && hh < H && ww >= 0 && ww < W);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = in[t] ? raw[c][ri + t / 3 - 1][rj + t % 3 - 1] : 0.f;
      // x / max_depth as the tensor op evaluates it on the device: times the fp32 reciprocal of the scalar
      med[c][i][j] = fmul_rn(median9(v), inv_max_d);
    }
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < TH * TW; idx += NT) {
    const int r = idx / TW, c = idx % TW;
    const int h = h0 + r, w = w0 + c;
    if (h >= H || w >= W) continue;
    const float ax = med[0][r + 2][c + 2], ay = med[1][r + 2][c + 2], az = med[2][r + 2][c + 2];
    float n[3];
    surface_normal_px(
        ax, ay, az,
        [&](int dh, int dw, float& x, float& y, float& z) {
          x = med[0][r + 2 + dh * D][c + 2 + dw * D];
          y = med[1][r + 2 + dh * D][c + 2 + dw * D];
          z = med[2][r + 2 + dh * D][c + 2 + dw * D];
        },
        0, n[0], n[1], n[2]);
    const int64_t o = (b * HW + (int64_t)h * W + w) * 3;
    points[o + 0] = ax;
    points[o + 1] = ay;
    points[o + 2] = az;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = -n[k];
      v = (v != v) ? 0.f : v;
      colors[o + k] = fmul_rn(fadd_rn(v, 1.f), 0.5f);
    }
  }
}

__global__ void colorize_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ lut,
                                int64_t total, int HW, int n_colors) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const float v = fminf(fmaxf(fmul_rn(x[t], (float)n_colors), 0.f), (float)(n_colors - 1));
    const int idx = (v != v) ? 0 : (int)v;   // truncation after the clamp
    const int64_t b = t / HW;
    float* o = out + b * 3 * HW + (t - b * HW);
    o[0] = lut[idx * 3 + 0];
    o[HW] = lut[idx * 3 + 1];
    o[2 * (int64_t)HW] = lut[idx * 3 + 2];
  }
}

}  // namespace

// image fp32 [B,1,H,W] in [-1,1], angle fp32 [1,2,H,W] -> points, colors fp32 [B,H*W,3]; border 0 "zeros", 1 "ring".
extern "C" int dgv2_frame_points(float* points, float* colors, const float* image, const float* angle, int B, int H,
                                 int W, float min_depth, float max_depth, int border, void* stream) {
  if (!points || !colors || !image || !angle || B <= 0 || H <= 0 || W <= 0 || D >= W || (border != 0 && border != 1))
    return DGV2_EINVAL;
  if ((int64_t)H * W >= (1LL << 31) / 3) return DGV2_EINVAL;
  const int tiles_h = (H + TH - 1) / TH, tiles_w = (W + TW - 1) / TW;
  const int64_t blocks = (int64_t)B * tiles_h * tiles_w;
  if (blocks >= (1LL << 31)) return DGV2_EINVAL;
  frame_points_kernel<<<(unsigned)blocks, NT, 0, (hipStream_t)stream>>>(points, colors, image, angle, H, W, tiles_h,
                                                                        tiles_w, min_depth, max_depth,
                                                                        1.0f / max_depth, border);
  DGV2_RETURN_LAST();
}

// x fp32 [B,H,W], lut fp32 [n_colors,3] -> out fp32 [B,3,H,W]
extern "C" int dgv2_colorize(float* out, const float* x, const float* lut, int B, int H, int W, int n_colors,
                             void* stream) {
  if (!out || !x || !lut || B <= 0 || H <= 0 || W <= 0 || n_colors <= 0) return DGV2_EINVAL;
  if ((int64_t)H * W >= (1LL << 31) / 3) return DGV2_EINVAL;
  const int64_t total = (int64_t)B * H * W;
  colorize_kernel<<<grid_for(total, 256), 256, 0, (hipStream_t)stream>>>(out, x, lut, total, H * W, n_colors);
  DGV2_RETURN_LAST();
}
