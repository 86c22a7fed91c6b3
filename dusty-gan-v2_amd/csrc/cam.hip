// Evaluation-mode context-aggregation module (CAM) of SqueezeSegV2 as ONE launch (include/dgv2.h, "Context
// aggregation module", states the arithmetic; DESIGN.md section 35 the structure and the measurements).  gfx950 only.
//
// A block of four waves owns TH x TW = 8 x 32 pixels of one sample, one pixel per thread.  Two phases:
//   A  the squeezed vector a[Cr] of every pixel.  The channels go through LDS in chunks of CC = 8, so LDS use does not
//      grow with C.  Per chunk: the tile plus its 3-pixel halo (14 x 38 per channel, -inf outside the image) is
//      written to LDS as float; a row pass leaves the maximum of 7 consecutive columns (14 x 32 per channel: a thread
//      reads 10 values with two 16-byte and one 8-byte LDS loads and writes 4 maxima); after a barrier every thread
//      takes the maximum of its 7 rows (conflict-free 4-byte reads: a half-wave is one tile row) and feeds it to its Cr
//      fmaf chains.  The pooled map lives in LDS and registers only.  The global loads of the next CAM_PF = 3 chunks
//      are in flight during the passes of the current one and wait in registers (their offsets are computed once per
//      block): the model's shapes give a compute unit one or two blocks, which hide a load only behind later loads.
//   B  for every channel, the gate from a[] (Cr fmafs, one exp, one divide) times x, re-read from L2 sixteen channels
//      at a time with the next sixteen in flight, and the one store.
// W1 / W2 / b2 are staged once per block in LDS as float32 (8.7 KB at C = 128, Cr = 8) and read at wave-uniform
// addresses (broadcasts).
// No atomics, no workspace; every output element is one c-ordered then j-ordered fmaf chain of its own pixel, so the
// bits depend neither on the grid nor on the batch.  max() is exact in every dtype, so holding the tile as float in
// LDS loses nothing; a and the gate stay float32, y is rounded once.
#include <math.h>

#include "common.h"

namespace {

typedef _Float16 f16_t;

constexpr int CAM_TH = 8, CAM_TW = 32, CAM_R = 3, CAM_CC = 8;
constexpr int CAM_THREADS = CAM_TH * CAM_TW;
constexpr int CAM_XH = CAM_TH + 2 * CAM_R;   // 14 haloed rows
constexpr int CAM_XW = CAM_TW + 2 * CAM_R;   // 38 haloed columns
constexpr int CAM_XP = 40;                   // LDS row pitch in floats: 16-byte aligned rows
constexpr int CAM_XS = CAM_CC * CAM_XH * CAM_XP;                       // floats of the haloed chunk image
constexpr int CAM_NLOAD = (CAM_XS + CAM_THREADS - 1) / CAM_THREADS;    // image slots per thread (pitch columns included)
constexpr int CAM_ROW_ITEMS = CAM_CC * CAM_XH * (CAM_TW / 4);          // (image row, group of 4 columns)
constexpr int CAM_CB = 16;                   // channels per batch of phase B (C is a multiple of 16)
constexpr int CAM_PF = 3;                    // chunks whose global loads are in flight ahead of the passes
constexpr int CAM_C_MAX = 128, CAM_CR_MAX = 8;

struct CamP {
  void* y;
  const void* x;
  const float *w1, *b1, *w2, *b2;
  int B, C, H, W, tiles_x, tiles_y;
};

template <typename T, int CR>
__global__ __launch_bounds__(CAM_THREADS) void cam_fwd_kernel(const CamP p) {
  constexpr int TH = CAM_TH, TW = CAM_TW, R = CAM_R, CC = CAM_CC, XH = CAM_XH, XW = CAM_XW, XP = CAM_XP;
  __shared__ __attribute__((aligned(16))) float xs[CAM_XS];
  __shared__ __attribute__((aligned(16))) float rm[CC * XH * TW];
  // the parameters, staged once per block: read from global memory at the point of use they are vector loads the
  // compiler must order against the stores of y (it cannot know they do not overlap), one exposed latency per channel
  __shared__ __attribute__((aligned(16))) float w1t[CAM_C_MAX * CR];   // [c][j]: a channel's Cr weights are contiguous
  __shared__ __attribute__((aligned(16))) float w2s[CAM_C_MAX * CR];   // [c][j], the tensor's own layout
  __shared__ float b2s[CAM_C_MAX];

  const int t = threadIdx.x;
  const int C = p.C, H = p.H, W = p.W;
  const int HW = H * W;   // C * H * W < 2^31 (checked by the entry): offsets inside a sample are ints

  int blk = blockIdx.x;
  const int tx = blk % p.tiles_x;
  blk /= p.tiles_x;
  const int ty = blk % p.tiles_y, b = blk / p.tiles_y;
  const int oh0 = ty * TH, ow0 = tx * TW;

  const T* __restrict__ const x = reinterpret_cast<const T*>(p.x) + (int64_t)b * C * HW;
  T* __restrict__ const y = reinterpret_cast<T*>(p.y) + (int64_t)b * C * HW;

  for (int i = t; i < C * CR; i += CAM_THREADS) {
    const int j = i / C, c = i - j * C;
    w1t[c * CR + j] = p.w1[i];
    w2s[i] = p.w2[i];
  }
  for (int c = t; c < C; c += CAM_THREADS) b2s[c] = p.b2[c];
  // (visible to every thread after the first chunk's barriers, before their first use)

  // slot i of this thread in the chunk image -> its offset from the chunk's first channel, -1 outside the image
  int off[CAM_NLOAD];
#pragma unroll
  for (int i = 0; i < CAM_NLOAD; ++i) {
    const int idx = t + i * CAM_THREADS;
    const int c = idx / (XH * XP), rem = idx - c * (XH * XP);
    const int rr = rem / XP, cc = rem - rr * XP;
    const int ih = oh0 - R + rr, iw = ow0 - R + cc;
    const bool in = idx < CAM_XS && cc < XW && ih >= 0 && ih < H && iw >= 0 && iw < W;
    off[i] = in ? c * HW + ih * W + iw : -1;
  }

  // the chunks' global loads run CAM_PF chunks ahead and wait in registers: with one or two blocks on a compute unit a
  // chunk's passes are far shorter than a load's latency, which a block can only hide behind its own later loads
  float nx[CAM_PF][CAM_NLOAD];
  auto prefetch = [&](float (&dst)[CAM_NLOAD], int c0) {
    const T* const xc = x + (int64_t)c0 * HW;
#pragma unroll
    for (int i = 0; i < CAM_NLOAD; ++i) {
      // an unconditional load from a clamped (valid) offset and a select: a guarded load is a branch per slot, and the
      // slots' loads would no longer be in flight together
      const float v = (float)xc[off[i] >= 0 ? off[i] : 0];
      dst[i] = off[i] >= 0 ? v : -INFINITY;
    }
  };

  const int r = t / TW, col = t - r * TW;
  float acc[CR];
#pragma unroll
  for (int j = 0; j < CR; ++j) acc[j] = 0.f;

  // ---- phase A ---------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int s = 0; s < CAM_PF; ++s)
    if (s * CC < C) prefetch(nx[s], s * CC);
  for (int cg = 0; cg < C; cg += CAM_PF * CC) {
#pragma unroll
    for (int s = 0; s < CAM_PF; ++s) {
      const int c0 = cg + s * CC;
      if (c0 >= C) break;   // block-uniform: the barriers below are reached by all threads or by none
      // xs was last read in the previous chunk's row pass, which every thread left through that chunk's second barrier
#pragma unroll
      for (int i = 0; i < CAM_NLOAD; ++i) {
        const int idx = t + i * CAM_THREADS;
        if (idx < CAM_XS) xs[idx] = nx[s][i];
      }
      __syncthreads();
      if (c0 + CAM_PF * CC < C) prefetch(nx[s], c0 + CAM_PF * CC);
      // row pass: rm[line][w] = max of xs[line][w .. w + 6]
      for (int it = t; it < CAM_ROW_ITEMS; it += CAM_THREADS) {
        const int line = it / (TW / 4), q = it - line * (TW / 4);
        const float* const src = xs + line * XP + 4 * q;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
        const float2 v2 = *reinterpret_cast<const float2*>(src + 8);
        const float mid = fmaxf(fmaxf(v0[3], v1[0]), fmaxf(v1[1], v1[2]));   // columns 3..6: in all four windows
        f32x4 o;
        o[0] = fmaxf(fmaxf(v0[0], v0[1]), fmaxf(v0[2], mid));
        o[1] = fmaxf(fmaxf(v0[1], v0[2]), fmaxf(mid, v1[3]));
        o[2] = fmaxf(fmaxf(v0[2], mid), fmaxf(v1[3], v2.x));
        o[3] = fmaxf(fmaxf(mid, v1[3]), fmaxf(v2.x, v2.y));
        *reinterpret_cast<f32x4*>(rm + line * TW + 4 * q) = o;
      }
      __syncthreads();
      // column pass and the first 1x1 conv, channels in increasing order
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        const float* const src = rm + (c * XH + r) * TW + col;
        float m = src[0];
#pragma unroll
        for (int k = 1; k < 2 * R + 1; ++k) m = fmaxf(m, src[k * TW]);
#pragma unroll
        for (int j = 0; j < CR; ++j) acc[j] = fmaf(w1t[(c0 + c) * CR + j], m, acc[j]);
      }
      // rm is next written after the next chunk's first barrier
    }
  }

  // ---- phase B ---------------------------------------------------------------------------------------------------------
  const int oh = oh0 + r, ow = ow0 + col;
  if (oh >= H || ow >= W) return;   // no barrier below
#pragma unroll
  for (int j = 0; j < CR; ++j) acc[j] = fmaxf(acc[j] + p.b1[j], 0.f);
  const int pix = oh * W + ow;
  // CAM_CB channels at a time, the next batch's loads in flight while this one is computed and stored
  float xv[2][CAM_CB];
  auto load_batch = [&](float (&dst)[CAM_CB], int c0) {
#pragma unroll
    for (int u = 0; u < CAM_CB; ++u) dst[u] = (float)x[(c0 + u) * HW + pix];
  };
  auto gate_batch = [&](const float (&src)[CAM_CB], int c0) {
#pragma unroll
    for (int u = 0; u < CAM_CB; ++u) {
      const int c = c0 + u;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < CR; ++j) s = fmaf(w2s[c * CR + j], acc[j], s);
      s += b2s[c];
      const float g = 1.0f / (1.0f + expf(-s));
      y[c * HW + pix] = (T)(src[u] * g);
    }
  };
  load_batch(xv[0], 0);
  for (int c0 = 0; c0 < C; c0 += 2 * CAM_CB) {
    const bool second = c0 + CAM_CB < C;
    if (second) load_batch(xv[1], c0 + CAM_CB);
    gate_batch(xv[0], c0);
    if (second) {
      if (c0 + 2 * CAM_CB < C) load_batch(xv[0], c0 + 2 * CAM_CB);
      gate_batch(xv[1], c0 + CAM_CB);
    }
  }
}

template <typename T, int CR> int cam_launch_cr(const CamP& p, hipStream_t st) {
  const int64_t blocks = (int64_t)p.tiles_x * p.tiles_y * p.B;
  if (blocks > 0x7fffffffLL) return DGV2_EINVAL;
  cam_fwd_kernel<T, CR><<<(unsigned)blocks, CAM_THREADS, 0, st>>>(p);
  DGV2_RETURN_LAST();
}

template <typename T> int cam_launch(const CamP& p, int Cr, hipStream_t st) {
  switch (Cr) {
    case 1: return cam_launch_cr<T, 1>(p, st);
    case 2: return cam_launch_cr<T, 2>(p, st);
    case 3: return cam_launch_cr<T, 3>(p, st);
    case 4: return cam_launch_cr<T, 4>(p, st);
    case 5: return cam_launch_cr<T, 5>(p, st);
    case 6: return cam_launch_cr<T, 6>(p, st);
    case 7: return cam_launch_cr<T, 7>(p, st);
    case 8: return cam_launch_cr<T, 8>(p, st);
  }
  return DGV2_EINVAL;
}

}  // namespace

extern "C" int dgv2_cam_fwd(void* y, const void* x, const float* w1, const float* b1, const float* w2, const float* b2,
                            int B, int C, int Cr, int H, int W, int dtype, void* stream) {
  if (!y || !x || !w1 || !b1 || !w2 || !b2) return DGV2_EINVAL;
  if (B < 1 || H < 1 || W < 1) return DGV2_EINVAL;
  if (C < 16 || C > CAM_C_MAX || C % 16 || Cr < 1 || Cr > CAM_CR_MAX) return DGV2_EINVAL;
  if ((int64_t)C * H * W > 0x7fffffffLL) return DGV2_EINVAL;   // offsets inside a sample are ints
  CamP p;
  p.y = y; p.x = x; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2;
  p.B = B; p.C = C; p.H = H; p.W = W;
  p.tiles_x = (W + CAM_TW - 1) / CAM_TW;
  p.tiles_y = (H + CAM_TH - 1) / CAM_TH;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DGV2_F32) return cam_launch<float>(p, Cr, st);
  if (dtype == DGV2_BF16) return cam_launch<bf16_t>(p, Cr, st);
  if (dtype == DGV2_F16) return cam_launch<f16_t>(p, Cr, st);
  return DGV2_EINVAL;
}
