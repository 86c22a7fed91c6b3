// GAN inversion (reference: gans/inversion.py, demo_inversion.py, gans/coords.py:88-185, ops/fourier.py:77-82):
//  * multi-scale masked loss: target pyramid (once per target), forward, backward;
//  * input gradient of the range conversion (dgv2_coords_convert, modes 0-3);
//  * angle gradient of the positional encoding.
//
// The loss works on images of a few ten thousand pixels: the reference spends ~40 launches each way on them, and an
// inversion step is launch-bound exactly there.  Every loss kernel here is ONE launch for any number of levels: one
// block per sample walks the levels, the pyramid level it has just written is read back after a __syncthreads (the
// block is the only reader and writer of its sample), and the per-sample sums are block reductions in a fixed order --
// no atomics, run-to-run bit-identical.  Ring convention of ops.Pad(1, "replicate", ring=True): circular along W,
// replicate along H; a 3x3 stride-2 window of an [H,W] level gives [(H+1)/2, (W+1)/2].
#include <limits.h>

#include "common.h"

namespace {

constexpr int MSML_THREADS = 1024;
constexpr int MSML_MAX_LEVELS = 16;

__host__ __device__ __forceinline__ int half_up(int n) { return (n + 1) >> 1; }

// blur [1,2,1] x [1,2,1] / 16
__device__ __forceinline__ float blur_tap(int i, int j) { return (float)((i == 1 ? 2 : 1) * (j == 1 ? 2 : 1)) * 0.0625f; }

__device__ __forceinline__ int ring_row(int h, int H) { return h < 0 ? 0 : (h >= H ? H - 1 : h); }
__device__ __forceinline__ int ring_col(int w, int W) { return w < 0 ? w + W : (w >= W ? w - W : w); }

// block_sum of common.h, with the result broadcast to every thread and `red` free for the next call on return
__device__ __forceinline__ float block_sum_all(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  __syncthreads();
  return s;
}

// blurpool(x * mask)[ho, wo] * norm over one channel plane x [H,W] with mask [H,W]
__device__ __forceinline__ float blurpool_masked(const float* x, const float* mask, int H, int W, int ho, int wo) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int h = ring_row(2 * ho - 1 + i, H);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int w = ring_col(2 * wo - 1 + j, W);
      acc += blur_tap(i, j) * (x[h * W + w] * mask[h * W + w]);
    }
  }
  return acc;
}

// Target pyramid (reference: MultiScaleMaskedLoss.forward / update_mask / blurpool, gans/inversion.py:45-76).
// refp: levels of ref, [B,C,Hi,Wi] each, level after level; maskp / normp: [B,Hi,Wi] each, level after level
// (normp's level i holds the norm that SCALES level i, i.e. update_mask of level i-1; its level 0 is not used);
// invm [L,B] = 1 / (sum(mask_i) + 1e-8).
__global__ __launch_bounds__(MSML_THREADS) void msml_prepare_kernel(float* refp, float* maskp, float* normp,
                                                                     float* __restrict__ invm,
                                                                     const float* __restrict__ ref,
                                                                     const float* __restrict__ mask, int B, int C, int H,
                                                                     int W, int L) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  int64_t offR = 0, offM = 0;
  int Hi = H, Wi = W;
  for (int p = threadIdx.x; p < C * H * W; p += blockDim.x) refp[(int64_t)b * C * H * W + p] = ref[(int64_t)b * C * H * W + p];
  for (int p = threadIdx.x; p < H * W; p += blockDim.x) maskp[(int64_t)b * H * W + p] = mask[(int64_t)b * H * W + p];
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int HW = Hi * Wi;
    const float* m = maskp + offM + (int64_t)b * HW;
    const float* r = refp + offR + (int64_t)b * C * HW;
    float s = 0.f;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) s += m[p];
    s = block_sum_all(s, red);
    if (threadIdx.x == 0) invm[l * B + b] = 1.f / (s + 1e-8f);
    if (l + 1 == L) break;
    const int Ho = half_up(Hi), Wo = half_up(Wi), HWo = Ho * Wo;
    const int64_t offRn = offR + (int64_t)B * C * HW, offMn = offM + (int64_t)B * HW;
    float* mn = maskp + offMn + (int64_t)b * HWo;
    float* nn = normp + offMn + (int64_t)b * HWo;
    float* rn = refp + offRn + (int64_t)b * C * HWo;
    for (int p = threadIdx.x; p < HWo; p += blockDim.x) {
      const int ho = p / Wo, wo = p % Wo;
      float cnt = 0.f;
      for (int i = 0; i < 3; ++i) {
        const int h = ring_row(2 * ho - 1 + i, Hi);
        for (int j = 0; j < 3; ++j) cnt += m[h * Wi + ring_col(2 * wo - 1 + j, Wi)];
      }
      const float norm = (1.f / (cnt == 0.f ? 1.f : cnt)) * 9.f;
      mn[p] = cnt == 0.f ? 0.f : 1.f;
      nn[p] = norm;
      for (int c = 0; c < C; ++c) rn[c * HWo + p] = blurpool_masked(r + c * HW, m, Hi, Wi, ho, wo) * norm;
    }
    __syncthreads();   // the next level reads what this block has just written
    offR = offRn;
    offM = offMn;
    Hi = Ho;
    Wi = Wo;
  }
}

// masked_loss's summand (gans/inversion.py:23-27) for one pixel: metric 0 = l1, 1 = mse
template <int METRIC, int RELATIVE>
__device__ __forceinline__ float diss(float ref, float gen, float mask) {
  const float d = ref - gen;
  float v = METRIC == 0 ? fabsf(d) : d * d;
  if (RELATIVE) v = (v * mask) / (ref + 1e-11f);
  return v * mask;
}
// ... and its derivative w.r.t. gen
template <int METRIC, int RELATIVE>
__device__ __forceinline__ float diss_grad(float ref, float gen, float mask) {
  const float d = gen - ref;
  float v = METRIC == 0 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d;
  if (RELATIVE) v = (v * mask) / (ref + 1e-11f);
  return v * mask;
}

// loss [B]; genp: levels 1 .. L-1 of the generated pyramid ([B,C,Hi,Wi] each, level after level, level 1 first)
template <int METRIC, int RELATIVE>
__global__ __launch_bounds__(MSML_THREADS) void msml_fwd_kernel(float* __restrict__ loss, float* genp,
                                                                 const float* __restrict__ gen,
                                                                 const float* __restrict__ refp,
                                                                 const float* __restrict__ maskp,
                                                                 const float* __restrict__ normp,
                                                                 const float* __restrict__ invm, int B, int C, int H,
                                                                 int W, int L) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  int64_t offR = 0, offM = 0;
  int Hi = H, Wi = W;
  float total = 0.f;
  const float* g = gen + (int64_t)b * C * H * W;
  for (int l = 0; l < L; ++l) {
    const int HW = Hi * Wi;
    const float* m = maskp + offM + (int64_t)b * HW;
    const float* r = refp + offR + (int64_t)b * C * HW;
    float s = 0.f;
    for (int p = threadIdx.x; p < C * HW; p += blockDim.x) s += diss<METRIC, RELATIVE>(r[p], g[p], m[p % HW]);
    total += block_sum_all(s, red) * invm[l * B + b];
    if (l + 1 == L) break;
    const int Ho = half_up(Hi), Wo = half_up(Wi), HWo = Ho * Wo;
    const int64_t offRn = offR + (int64_t)B * C * HW, offMn = offM + (int64_t)B * HW;
    const float* nn = normp + offMn + (int64_t)b * HWo;
    // level l+1 of genp sits at level l+1's offset in the ref layout less the size of level 0
    float* gn = genp + (offRn - (int64_t)B * C * H * W) + (int64_t)b * C * HWo;
    for (int p = threadIdx.x; p < C * HWo; p += blockDim.x) {
      const int c = p / HWo, q = p % HWo;
      gn[p] = blurpool_masked(g + c * HW, m, Hi, Wi, q / Wo, q % Wo) * nn[q];
    }
    __syncthreads();
    g = gn;
    offR = offRn;
    offM = offMn;
    Hi = Ho;
    Wi = Wo;
  }
  if (threadIdx.x == 0) loss[b] = total;
}

// ggen [B,C,H,W] = gloss[b] * d loss[b] / d gen; gp: scratch with genp's layout for the gradients of levels 1 .. L-1.
// Walks the levels from the coarsest: g_i = own term + mask_i * blur^T(norm_{i+1} * g_{i+1}), gathered per input pixel
// (the taps of every window that covers it, with the replicate / circular edges folded back).
template <int METRIC, int RELATIVE>
__global__ __launch_bounds__(MSML_THREADS) void msml_bwd_kernel(float* __restrict__ ggen, float* gp,
                                                                 const float* __restrict__ gloss,
                                                                 const float* __restrict__ gen,
                                                                 const float* __restrict__ genp,
                                                                 const float* __restrict__ refp,
                                                                 const float* __restrict__ maskp,
                                                                 const float* __restrict__ normp,
                                                                 const float* __restrict__ invm, int B, int C, int H,
                                                                 int W, int L) {
  const int b = blockIdx.x;
  int Hs[MSML_MAX_LEVELS], Ws[MSML_MAX_LEVELS];
  int64_t offRs[MSML_MAX_LEVELS], offMs[MSML_MAX_LEVELS];
  {
    int Hi = H, Wi = W;
    int64_t offR = 0, offM = 0;
    for (int l = 0; l < L; ++l) {
      Hs[l] = Hi;
      Ws[l] = Wi;
      offRs[l] = offR;
      offMs[l] = offM;
      offR += (int64_t)B * C * Hi * Wi;
      offM += (int64_t)B * Hi * Wi;
      Hi = half_up(Hi);
      Wi = half_up(Wi);
    }
  }
  const float go = gloss[b];
  const int64_t lvl0 = (int64_t)B * C * H * W;
  for (int l = L - 1; l >= 0; --l) {
    const int Hi = Hs[l], Wi = Ws[l], HW = Hi * Wi;
    const float* m = maskp + offMs[l] + (int64_t)b * HW;
    const float* r = refp + offRs[l] + (int64_t)b * C * HW;
    const float* g = l == 0 ? gen + (int64_t)b * C * HW : genp + (offRs[l] - lvl0) + (int64_t)b * C * HW;
    float* out = l == 0 ? ggen + (int64_t)b * C * HW : gp + (offRs[l] - lvl0) + (int64_t)b * C * HW;
    const float wl = go * invm[l * B + b];
    const bool up = l + 1 < L;
    const int Ho = half_up(Hi), Wo = half_up(Wi), HWo = Ho * Wo;
    const float* gu = up ? gp + (offRs[l + 1] - lvl0) + (int64_t)b * C * HWo : nullptr;
    const float* nu = up ? normp + offMs[l + 1] + (int64_t)b * HWo : nullptr;
    for (int p = threadIdx.x; p < C * HW; p += blockDim.x) {
      const int c = p / HW, q = p % HW, h = q / Wi, w = q % Wi;
      const float mk = m[q];
      float v = wl * diss_grad<METRIC, RELATIVE>(r[p], g[p], mk);
      if (up) {
        // unpadded positions that fold back onto (h, w): itself, -1 for the first and H (W) for the last row (column)
        const int rows[3] = {h, h == 0 ? -1 : INT_MIN, h == Hi - 1 ? Hi : INT_MIN};
        const int cols[3] = {w, w == Wi - 1 ? -1 : INT_MIN, w == 0 ? Wi : INT_MIN};
        float acc = 0.f;
        for (int a = 0; a < 3; ++a) {
          if (rows[a] == INT_MIN) continue;
          for (int i = 0; i < 3; ++i) {
            const int t = rows[a] + 1 - i;   // = 2 ho
            if (t < 0 || (t & 1) || (t >> 1) >= Ho) continue;
            const int ho = t >> 1;
            for (int e = 0; e < 3; ++e) {
              if (cols[e] == INT_MIN) continue;
              for (int j = 0; j < 3; ++j) {
                const int u = cols[e] + 1 - j;   // = 2 wo
                if (u < 0 || (u & 1) || (u >> 1) >= Wo) continue;
                const int o = ho * Wo + (u >> 1);
                acc += blur_tap(i, j) * (gu[c * HWo + o] * nu[o]);
              }
            }
          }
        }
        v += acc * mk;
      }
      out[p] = v;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Input gradient of coords_kernel (tail_coords.hip), term by term as autograd differentiates gans/coords.py:88-185:
// the validity masks are constants, d(1/(x+tol)) = -1/(x+tol)^2.
__global__ void coords_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gout, const float* __restrict__ in,
                                  const float* __restrict__ mask, const float* __restrict__ angle, int B, int HW,
                                  float min_d, float max_d, int mode) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const float x = in[t];
    if (mode == 0) {
      const bool valid = (x >= min_d) && (x <= max_d) && (x > 0.f);
      const float q = 1.f / (x + 1e-11f);
      float d = valid ? -(q * q) * min_d : 0.f;
      if (mask) d *= 2.f * mask[t];
      gx[t] = gout[t] * d;
      continue;
    }
    float dd = 1.f;   // d depth / d x
    if (mode != 3) {
      const float inv = x / min_d;
      bool valid = (inv >= 1.f / max_d) && (inv <= 1.f / min_d) && (inv > 0.f);
      if (mode == 2) valid = valid && (x > 1e-11f);
      const float q = 1.f / (inv + 1e-11f);
      dd = valid ? -(q * q) / min_d : 0.f;
    }
    if (mode == 1) {
      gx[t] = gout[t] * dd;
    } else {
      const int p = (int)(t % HW);
      const int64_t b = t / HW;
      float se, ce, sa, ca;
      sincosf(angle[p], &se, &ce);
      sincosf(angle[HW + p], &sa, &ca);
      const float* g = gout + b * 3 * HW + p;
      gx[t] = (g[0] * (ce * ca) + g[HW] * (ce * sa) + g[2 * (int64_t)HW] * se) * dd;
    }
  }
}

// ---------------------------------------------------------------------------
// Angle gradient of fourier_kernel (fourier.hip): G lanes of a wave share a pixel (G a power of two <= 64), each walks
// 16-byte pieces of the gradient row's sin half and the matching pieces of its cos half, the phases are recomputed, and
// one xor-shuffle reduction over the G lanes leaves the pixel's two sums.  VEC = 0: element loads (rows whose
// c0 / F / ld / base do not allow 16-byte pieces).
template <typename T, int VEC>
__global__ void fourier_bwd_kernel(float* __restrict__ g_angle, const T* __restrict__ g, const float* __restrict__ angle,
                                   const float* __restrict__ shift, const float* __restrict__ freqs,
                                   const float* __restrict__ phase, int B, int Ba, int HW, int F, int ld, int c0, int G) {
  constexpr int VN = VEC ? vec16<T>::N : 1;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (G - 1);
  const int per_wave = 64 / G;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t total = (int64_t)B * HW;
  const int64_t rounds = (total + per_wave - 1) / per_wave;
  for (int64_t it = wave; it < rounds; it += nwaves) {   // uniform per wave: the shuffles below see all 64 lanes
    const int64_t bp = it * per_wave + lane / G;
    const bool live = bp < total;
    float ge = 0.f, ga = 0.f;
    if (live) {
      const int p = (int)(bp % HW);
      const int b = (int)(bp / HW);
      const int ba = Ba == 1 ? 0 : b;
      const float elev = angle[((int64_t)ba * 2 + 0) * HW + p];
      float azim = angle[((int64_t)ba * 2 + 1) * HW + p];
      if (shift) azim += shift[b];
      const T* row = g + bp * ld + c0;
      for (int f0 = sub * VN; f0 < F; f0 += G * VN) {
        float gs[VN], gc[VN];
        if (VEC) {
          vec16<T> vs, vc;
          vs.load(row + f0);
          vc.load(row + F + f0);
#pragma unroll
          for (int k = 0; k < VN; ++k) {
            gs[k] = vs.get(k);
            gc[k] = vc.get(k);
          }
        } else {
          gs[0] = to_f32(row[f0]);
          gc[0] = to_f32(row[F + f0]);
        }
#pragma unroll
        for (int k = 0; k < VN; ++k) {
          const int f = f0 + k;
          const float fe = freqs[2 * f], fa = freqs[2 * f + 1];
          const float c = fe * elev + fa * azim + phase[f];
          float s, cs;
          sincosf(c, &s, &cs);
          const float d = gs[k] * cs - gc[k] * s;
          ge = fmaf(fe, d, ge);
          ga = fmaf(fa, d, ga);
        }
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
      ge += __shfl_xor(ge, o, 64);
      ga += __shfl_xor(ga, o, 64);
    }
    if (live && sub == 0) {
      const int p = (int)(bp % HW);
      const int64_t b = bp / HW;
      g_angle[(b * 2 + 0) * HW + p] = ge;
      g_angle[(b * 2 + 1) * HW + p] = ga;
    }
  }
}

bool msml_args_ok(int B, int C, int H, int W, int L) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || L < 1 || L > MSML_MAX_LEVELS) return false;
  if ((int64_t)C * H * W > (int64_t)1 << 30) return false;
  // every level that is pooled needs two columns at least (one circular wrap per window)
  for (int l = 0; l + 1 < L; ++l) {
    if (W < 2) return false;
    H = half_up(H);
    W = half_up(W);
  }
  return true;
}

}  // namespace

extern "C" int dgv2_msml_prepare(float* refp, float* maskp, float* normp, float* invm, const float* ref,
                                 const float* mask, int B, int C, int H, int W, int L, void* stream) {
  if (!refp || !maskp || !normp || !invm || !ref || !mask || !msml_args_ok(B, C, H, W, L)) return DGV2_EINVAL;
  msml_prepare_kernel<<<B, MSML_THREADS, 0, (hipStream_t)stream>>>(refp, maskp, normp, invm, ref, mask, B, C, H, W, L);
  DGV2_RETURN_LAST();
}

#define MSML_DISPATCH(kernel, ...)                                                         \
  do {                                                                                     \
    if (metric == 0 && relative) kernel<0, 1><<<B, MSML_THREADS, 0, st>>>(__VA_ARGS__);    \
    else if (metric == 0) kernel<0, 0><<<B, MSML_THREADS, 0, st>>>(__VA_ARGS__);           \
    else if (relative) kernel<1, 1><<<B, MSML_THREADS, 0, st>>>(__VA_ARGS__);              \
    else kernel<1, 0><<<B, MSML_THREADS, 0, st>>>(__VA_ARGS__);                            \
  } while (0)

extern "C" int dgv2_msml_fwd(float* loss, float* genp, const float* gen, const float* refp, const float* maskp,
                             const float* normp, const float* invm, int B, int C, int H, int W, int L, int metric,
                             int relative, void* stream) {
  if (!loss || !gen || !refp || !maskp || !normp || !invm || !msml_args_ok(B, C, H, W, L)) return DGV2_EINVAL;
  if ((L > 1 && !genp) || metric < 0 || metric > 1) return DGV2_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  MSML_DISPATCH(msml_fwd_kernel, loss, genp, gen, refp, maskp, normp, invm, B, C, H, W, L);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_msml_bwd(float* ggen, float* gscratch, const float* gloss, const float* gen, const float* genp,
                             const float* refp, const float* maskp, const float* normp, const float* invm, int B, int C,
                             int H, int W, int L, int metric, int relative, void* stream) {
  if (!ggen || !gloss || !gen || !refp || !maskp || !normp || !invm || !msml_args_ok(B, C, H, W, L)) return DGV2_EINVAL;
  if ((L > 1 && (!genp || !gscratch)) || metric < 0 || metric > 1) return DGV2_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  MSML_DISPATCH(msml_bwd_kernel, ggen, gscratch, gloss, gen, genp, refp, maskp, normp, invm, B, C, H, W, L);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_coords_convert_bwd(float* gx, const float* gout, const float* in, const float* mask,
                                       const float* angle, int B, int H, int W, float min_depth, float max_depth,
                                       int mode, void* stream) {
  if (!gx || !gout || !in || B <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 3) return DGV2_EINVAL;
  if (mode >= 2 && !angle) return DGV2_EINVAL;
  const int64_t total = (int64_t)B * H * W;
  coords_bwd_kernel<<<grid_for(total, 256), 256, 0, (hipStream_t)stream>>>(gx, gout, in, mask, angle, B, H * W,
                                                                          min_depth, max_depth, mode);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_fourier_feature_bwd(float* g_angle, const void* g, const float* angle, const float* shift,
                                        const float* freqs, const float* phase, int B, int Ba, int H, int W, int F,
                                        int ld, int c0, int dtype, void* stream) {
  if (!g_angle || !g || !angle || !freqs || !phase || B <= 0 || H <= 0 || W <= 0 || F <= 0) return DGV2_EINVAL;
  if ((Ba != 1 && Ba != B) || c0 < 0 || ld < c0 + 2 * F) return DGV2_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W;
  DGV2_DISPATCH_DTYPE(dtype, {
    constexpr int VN = vec16<T>::N;
    const bool vec = aligned16(g) && F % VN == 0 && c0 % VN == 0 && ld % VN == 0;
    const int pieces = vec ? F / VN : F;
    int G = 1;
    while (G < 64 && G < pieces) G <<= 1;
    const int64_t waves = (total + 64 / G - 1) / (64 / G);
    const int grid = grid_for(waves * 64, 256, 256 * 32);
    if (vec)
      fourier_bwd_kernel<T, 1><<<grid, 256, 0, st>>>(g_angle, (const T*)g, angle, shift, freqs, phase, B, Ba, H * W, F,
                                                     ld, c0, G);
    else
      fourier_bwd_kernel<T, 0><<<grid, 256, 0, st>>>(g_angle, (const T*)g, angle, shift, freqs, phase, B, Ba, H * W, F,
                                                     ld, c0, G);
  });
  DGV2_RETURN_LAST();
}
