// CRF-RNN mean-field refinement of the range-image segmentation models (reference: semseg/models/crf_as_rnn.py:110-132;
// the formulas are in include/dgv2.h).  fp32, NCHW, plain HIP: a memory-bound stencil.
//
//  * A block owns a TH x TW pixel tile of one sample and stages the tile plus a halo of (kh/2, kw/2) in LDS: the C
//    softmax probabilities (computed while staging), xyz and the mask; positions outside the image hold 0, which is
//    what the reference's unfold / conv2d padding contributes.  The three stencils then read LDS only; the bilateral
//    weight exp(-|xyz(p+n) - xyz(p)|^2 / (2 theta_c^2)) is recomputed per tap from the staged xyz: no [B,C,K,HW]
//    tensor exists.  TW = 64 for C <= 4 and 32 above, so the widest stage (the gather of the backward: 3C + 4 planes
//    at kh = 5, kw = 9) stays below 64 KiB of LDS.
//  * forward: one launch per iteration; iteration t reads Q_t and writes Q_{t+1}; Q_1 .. Q_{n-1} land in the caller's
//    `qsave`, which is all the backward needs (Q_0 is the unary).
//  * backward, per iteration in reverse, two launches: crf_backward_fields_kernel recomputes S, L, A from Q_t, forms
//    dT = -M^T dQ', writes the fields dS = ws dT, dL = wa dT A, m dA = m wa dT L and leaves the block's partial sums of
//    the parameter gradients in scratch (plain stores); crf_backward_gather_kernel applies the gather stencil to the
//    fields (beta is symmetric: beta_c(p, n) = beta_c(p + n, -n)) and the softmax backward.  One finishing launch sums
//    the partials of every block and iteration in a fixed order: no float atomics, bit-identical run to run.
#include "common.h"

namespace {

constexpr int CMAX = 8, KH_MAX = 5, KW_MAX = 9, TH = 8, NT = 256;

template <int C> struct Tile { static constexpr int TW = C <= 4 ? 64 : 32; };

struct Geo {
  int H, W, kh, kw, tiles_h, tiles_w;
};

// the block's tile and its staged region [h0 - ph, h0 + TH + ph) x [w0 - pw, w0 + TW + pw)
struct Blk {
  int64_t b;
  int h0, w0, ph, pw, RW, NP;
};

template <int TW> __device__ __forceinline__ Blk block_of(const Geo& g) {
  Blk k;
  const int tiles = g.tiles_h * g.tiles_w, tile = blockIdx.x % tiles;
  k.b = blockIdx.x / tiles;
  k.h0 = (tile / g.tiles_w) * TH;
  k.w0 = (tile % g.tiles_w) * TW;
  k.ph = g.kh / 2;
  k.pw = g.kw / 2;
  k.RW = TW + g.kw - 1;
  k.NP = (TH + g.kh - 1) * k.RW;
  return k;
}

// image offset of staged position idx, or -1 outside the image
__device__ __forceinline__ int staged_pixel(const Blk& k, const Geo& g, int idx) {
  const int h = k.h0 - k.ph + idx / k.RW, w = k.w0 - k.pw + idx % k.RW;
  return (h >= 0 && h < g.H && w >= 0 && w < g.W) ? h * g.W + w : -1;
}

// softmax over the C planes q[0], q[HW], ..
template <int C> __device__ __forceinline__ void softmax_at(float (&p)[C], const float* __restrict__ q, int64_t HW) {
  float mx = q[0];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = q[c * HW];
    mx = fmaxf(mx, p[c]);
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = expf(p[c] - mx);
    s += p[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = p[c] / s;
}

// sx [3][NP], sm [NP] <- xyz, mask of sample b; sp [C][NP] <- softmax(q) (q == nullptr: not staged)
template <int C>
__device__ __forceinline__ void stage_inputs(float* sp, float* sx, float* sm, const float* __restrict__ q,
                                             const float* __restrict__ xyz, const float* __restrict__ mask,
                                             const Blk& k, const Geo& g) {
  const int64_t HW = (int64_t)g.H * g.W;
  const float* xb = xyz + k.b * 3 * HW;
  const float* mb = mask + k.b * HW;
  for (int idx = threadIdx.x; idx < k.NP; idx += NT) {
    const int p = staged_pixel(k, g, idx);
    sx[idx] = p >= 0 ? xb[p] : 0.f;
    sx[k.NP + idx] = p >= 0 ? xb[HW + p] : 0.f;
    sx[2 * k.NP + idx] = p >= 0 ? xb[2 * HW + p] : 0.f;
    sm[idx] = p >= 0 ? mb[p] : 0.f;
    if (q) {
      float v[C];
      if (p >= 0) softmax_at<C>(v, q + k.b * C * HW + p, HW);
#pragma unroll
      for (int c = 0; c < C; ++c) sp[c * k.NP + idx] = p >= 0 ? v[c] : 0.f;
    }
  }
}

// coef[c] = -1 / (2 theta_beta[c]^2); returns whether every class has the same one (the layer's default: a scalar
// theta_beta), in which case a tap's bilateral weight is evaluated once instead of C times -- the same value
template <int C> __device__ __forceinline__ bool beta_coef(float (&coef)[C], const float* __restrict__ theta_beta) {
  bool same = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    coef[c] = -1.f / (2.f * theta_beta[c] * theta_beta[c]);
    same = same && theta_beta[c] == theta_beta[0];
  }
  return same;
}

// S, L, A of tile pixel (r, col) from the staged probabilities; kg / ka are the [C,C,kh,kw] buffers (diagonal read)
template <int C, bool SAME>
__device__ __forceinline__ void message_passing(float (&S)[C], float (&L)[C], float (&A)[C], const float* sp,
                                                const float* sx, const float* sm, const Blk& k, const Geo& g, int r,
                                                int col, const float* __restrict__ kg, const float* __restrict__ ka,
                                                const float (&coef)[C]) {
  const int K = g.kh * g.kw, ctr = (r + k.ph) * k.RW + col + k.pw;
  const float x0 = sx[ctr], y0 = sx[k.NP + ctr], z0 = sx[2 * k.NP + ctr];
#pragma unroll
  for (int c = 0; c < C; ++c) S[c] = L[c] = A[c] = 0.f;
  for (int dy = 0; dy < g.kh; ++dy)
    for (int dx = 0; dx < g.kw; ++dx) {
      const int pos = (r + dy) * k.RW + col + dx, n = dy * g.kw + dx;
      const float ex = sx[pos] - x0, ey = sx[k.NP + pos] - y0, ez = sx[2 * k.NP + pos] - z0;
      const float d2 = ex * ex + ey * ey + ez * ez, mn = sm[pos];
      const bool centre = pos == ctr;
      const float beta0 = SAME ? expf(d2 * coef[0]) : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float p = sp[c * k.NP + pos], beta = SAME ? beta0 : expf(d2 * coef[c]);
        S[c] = fmaf(kg[(C + 1) * K * c + n], p, S[c]);
        L[c] = fmaf(ka[(C + 1) * K * c + n], p, L[c]);
        A[c] += centre ? 0.f : beta * mn * p;   // the centre is not a neighbour
      }
    }
  const float m0 = sm[ctr];
#pragma unroll
  for (int c = 0; c < C; ++c) A[c] *= m0;
}

template <int C>
__global__ __launch_bounds__(NT) void crf_forward_kernel(float* __restrict__ q_out, const float* __restrict__ q_in,
                                                         const float* __restrict__ unary,
                                                         const float* __restrict__ xyz, const float* __restrict__ mask,
                                                         const float* __restrict__ kg, const float* __restrict__ ka,
                                                         const float* __restrict__ theta_beta,
                                                         const float* __restrict__ ws, const float* __restrict__ wa,
                                                         const float* __restrict__ compat, Geo g) {
  constexpr int TW = Tile<C>::TW;
  extern __shared__ __align__(16) float smem[];
  const Blk k = block_of<TW>(g);
  float *sp = smem, *sx = sp + C * k.NP, *sm = sx + 3 * k.NP;
  stage_inputs<C>(sp, sx, sm, q_in, xyz, mask, k, g);
  float coef[C];
  const bool same = beta_coef<C>(coef, theta_beta);
  __syncthreads();

  const int64_t HW = (int64_t)g.H * g.W;
  for (int idx = threadIdx.x; idx < TH * TW; idx += NT) {
    const int r = idx / TW, col = idx % TW, h = k.h0 + r, w = k.w0 + col;
    if (h >= g.H || w >= g.W) continue;
    float S[C], L[C], A[C], T[C];
    if (same) message_passing<C, true>(S, L, A, sp, sx, sm, k, g, r, col, kg, ka, coef);
    else message_passing<C, false>(S, L, A, sp, sx, sm, k, g, r, col, kg, ka, coef);
#pragma unroll
    for (int c = 0; c < C; ++c) T[c] = ws[c] * S[c] + wa[c] * A[c] * L[c];
    const int64_t o = k.b * C * HW + (int64_t)h * g.W + w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float pair = 0.f;
#pragma unroll
      for (int d = 0; d < C; ++d) pair = fmaf(compat[c * C + d], T[d], pair);
      q_out[o + c * HW] = unary[o + c * HW] - pair;
    }
  }
}

// First backward launch of an iteration.  dq: the cotangent of the iteration's output.  Writes fields [3][B,C,H,W] =
// dS, dL, m dA, the block's partial sums part[blockIdx][2C + C*C] = (dws, dwa, dM), and g_unary (+)= dq.
template <int C>
__global__ __launch_bounds__(NT) void crf_backward_fields_kernel(
    float* __restrict__ fields, float* __restrict__ part, float* __restrict__ g_unary, int accumulate,
    const float* __restrict__ dq, const float* __restrict__ q_in, const float* __restrict__ xyz,
    const float* __restrict__ mask, const float* __restrict__ kg, const float* __restrict__ ka,
    const float* __restrict__ theta_beta, const float* __restrict__ ws, const float* __restrict__ wa,
    const float* __restrict__ compat, int64_t plane, Geo g) {
  constexpr int TW = Tile<C>::TW, NOUT = 2 * C + C * C;
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[NT / 64][NOUT];
  const Blk k = block_of<TW>(g);
  float *sp = smem, *sx = sp + C * k.NP, *sm = sx + 3 * k.NP;
  stage_inputs<C>(sp, sx, sm, q_in, xyz, mask, k, g);
  float coef[C];
  const bool same = beta_coef<C>(coef, theta_beta);
  __syncthreads();

  float acc[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) acc[i] = 0.f;
  const int64_t HW = (int64_t)g.H * g.W;
  for (int idx = threadIdx.x; idx < TH * TW; idx += NT) {
    const int r = idx / TW, col = idx % TW, h = k.h0 + r, w = k.w0 + col;
    if (h >= g.H || w >= g.W) continue;
    float S[C], L[C], A[C], G[C], dT[C];
    if (same) message_passing<C, true>(S, L, A, sp, sx, sm, k, g, r, col, kg, ka, coef);
    else message_passing<C, false>(S, L, A, sp, sx, sm, k, g, r, col, kg, ka, coef);
    const int64_t o = k.b * C * HW + (int64_t)h * g.W + w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      G[c] = dq[o + c * HW];
      g_unary[o + c * HW] = accumulate ? g_unary[o + c * HW] + G[c] : G[c];
    }
    const float m0 = sm[(r + k.ph) * k.RW + col + k.pw];
#pragma unroll
    for (int d = 0; d < C; ++d) {
      float t = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) t = fmaf(compat[c * C + d], G[c], t);
      dT[d] = -t;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float AL = A[c] * L[c], T = ws[c] * S[c] + wa[c] * AL;
      acc[c] = fmaf(dT[c], S[c], acc[c]);
      acc[C + c] = fmaf(dT[c], AL, acc[C + c]);
#pragma unroll
      for (int e = 0; e < C; ++e) acc[2 * C + e * C + c] = fmaf(-G[e], T, acc[2 * C + e * C + c]);   // dM[e, c]
      fields[o + c * HW] = ws[c] * dT[c];
      fields[plane + o + c * HW] = wa[c] * dT[c] * A[c];
      fields[2 * plane + o + c * HW] = m0 * (wa[c] * dT[c] * L[c]);
    }
  }
  // fixed-order block sum: butterflies inside a wave, then the waves in order
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const float v = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NOUT) {
    float s = 0.f;
    for (int wv = 0; wv < NT / 64; ++wv) s += red[wv][threadIdx.x];
    part[(int64_t)blockIdx.x * NOUT + threadIdx.x] = s;
  }
}

// Second backward launch: dP = gather stencil of the fields, dQ = P (dP - sum_c P dP) with P = softmax(q_in);
// dq_out (+)= dQ.
template <int C>
__global__ __launch_bounds__(NT) void crf_backward_gather_kernel(
    float* __restrict__ dq_out, int accumulate, const float* __restrict__ fields, const float* __restrict__ q_in,
    const float* __restrict__ xyz, const float* __restrict__ mask, const float* __restrict__ kg,
    const float* __restrict__ ka, const float* __restrict__ theta_beta, int64_t plane, Geo g) {
  constexpr int TW = Tile<C>::TW;
  extern __shared__ __align__(16) float smem[];
  const Blk k = block_of<TW>(g);
  float *sf = smem, *sx = sf + 3 * C * k.NP, *sm = sx + 3 * k.NP;
  stage_inputs<C>(nullptr, sx, sm, nullptr, xyz, mask, k, g);
  const int64_t HW = (int64_t)g.H * g.W;
  for (int idx = threadIdx.x; idx < k.NP; idx += NT) {
    const int p = staged_pixel(k, g, idx);
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
      for (int c = 0; c < C; ++c)
        sf[(f * C + c) * k.NP + idx] = p >= 0 ? fields[f * plane + (k.b * C + c) * HW + p] : 0.f;
  }
  float coef[C];
  const bool same = beta_coef<C>(coef, theta_beta);
  __syncthreads();

  const int K = g.kh * g.kw;
  for (int idx = threadIdx.x; idx < TH * TW; idx += NT) {
    const int r = idx / TW, col = idx % TW, h = k.h0 + r, w = k.w0 + col;
    if (h >= g.H || w >= g.W) continue;
    const int ctr = (r + k.ph) * k.RW + col + k.pw;
    const float x0 = sx[ctr], y0 = sx[k.NP + ctr], z0 = sx[2 * k.NP + ctr];
    float dP[C], dB[C], P[C];
#pragma unroll
    for (int c = 0; c < C; ++c) dP[c] = dB[c] = 0.f;
    for (int dy = 0; dy < g.kh; ++dy)
      for (int dx = 0; dx < g.kw; ++dx) {
        const int pos = (r + dy) * k.RW + col + dx, nf = K - 1 - (dy * g.kw + dx);   // the tap that reaches back
        const float ex = sx[pos] - x0, ey = sx[k.NP + pos] - y0, ez = sx[2 * k.NP + pos] - z0;
        const float d2 = ex * ex + ey * ey + ez * ez;
        const bool centre = pos == ctr;
        float beta[C];
        if (same) {
          const float beta0 = expf(d2 * coef[0]);
#pragma unroll
          for (int c = 0; c < C; ++c) beta[c] = beta0;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) beta[c] = expf(d2 * coef[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          dP[c] = fmaf(kg[(C + 1) * K * c + nf], sf[c * k.NP + pos], dP[c]);
          dP[c] = fmaf(ka[(C + 1) * K * c + nf], sf[(C + c) * k.NP + pos], dP[c]);
          dB[c] += centre ? 0.f : beta[c] * sf[(2 * C + c) * k.NP + pos];
        }
      }
    const float m0 = sm[ctr];
    const int64_t o = k.b * C * HW + (int64_t)h * g.W + w;
    softmax_at<C>(P, q_in + o, HW);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      dP[c] = fmaf(m0, dB[c], dP[c]);
      dot = fmaf(P[c], dP[c], dot);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = P[c] * (dP[c] - dot);
      dq_out[o + c * HW] = accumulate ? dq_out[o + c * HW] + v : v;
    }
  }
}

// out[o] = sum of part[i][o] over the n_part partials: 256 strided running sums, then block_sum's fixed order
__global__ __launch_bounds__(NT) void crf_param_finish_kernel(float* __restrict__ g_ws, float* __restrict__ g_wa,
                                                             float* __restrict__ g_compat,
                                                             const float* __restrict__ part, int64_t n_part, int C) {
  __shared__ float red[16];
  const int nout = 2 * C + C * C, o = blockIdx.x;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n_part; i += NT) s += part[i * nout + o];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    if (o < C) g_ws[o] = s;
    else if (o < 2 * C) g_wa[o - C] = s;
    else g_compat[o - 2 * C] = s;
  }
}

struct Plan {
  Geo g;
  int64_t blocks, bchw;
  int TW;
};

bool plan_for(Plan& p, int B, int C, int H, int W, int kh, int kw, int num_iters) {
  if (B <= 0 || C < 1 || C > CMAX || H <= 0 || W <= 0 || num_iters < 1) return false;
  if (kh < 1 || kh > KH_MAX || kw < 1 || kw > KW_MAX || kh % 2 == 0 || kw % 2 == 0) return false;
  if ((int64_t)H * W >= (1LL << 31)) return false;
  p.TW = C <= 4 ? Tile<1>::TW : Tile<CMAX>::TW;
  p.g = Geo{H, W, kh, kw, (H + TH - 1) / TH, (W + p.TW - 1) / p.TW};
  p.blocks = (int64_t)B * p.g.tiles_h * p.g.tiles_w;
  p.bchw = (int64_t)B * C * H * W;
  return p.blocks < (1LL << 31) && p.bchw < (1LL << 40);
}

// bytes of dynamic LDS for `planes` staged planes
size_t lds_bytes(const Plan& p, int planes) {
  return sizeof(float) * planes * (size_t)(TH + p.g.kh - 1) * (p.TW + p.g.kw - 1);
}

int64_t scratch_elems_for(const Plan& p, int C, int num_iters) {
  return 4 * p.bchw + (int64_t)num_iters * p.blocks * (2 * C + C * C);
}

#define CRF_DISPATCH_C(C_, ...)            \
  switch (C_) {                            \
    case 1: { constexpr int CC = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int CC = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int CC = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int CC = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int CC = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int CC = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int CC = 7; __VA_ARGS__; } break; \
    case 8: { constexpr int CC = 8; __VA_ARGS__; } break; \
    default: return DGV2_EINVAL;           \
  }

}  // namespace

extern "C" int dgv2_crf_rnn_forward(float* out, float* qsave, const float* unary, const float* xyz, const float* mask,
                                    const float* kernel_gamma, const float* kernel_alpha, const float* theta_beta,
                                    const float* weight_smoothness, const float* weight_appearance,
                                    const float* compat, int B, int C, int H, int W, int kh, int kw, int num_iters,
                                    void* stream) {
  Plan p;
  if (!out || !unary || !xyz || !mask || !kernel_gamma || !kernel_alpha || !theta_beta || !weight_smoothness ||
      !weight_appearance || !compat || !plan_for(p, B, C, H, W, kh, kw, num_iters) || (num_iters > 1 && !qsave))
    return DGV2_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const size_t lds = lds_bytes(p, C + 4);
  for (int t = 0; t < num_iters; ++t) {
    const float* q_in = t == 0 ? unary : qsave + (int64_t)(t - 1) * p.bchw;
    float* q_out = t == num_iters - 1 ? out : qsave + (int64_t)t * p.bchw;
    CRF_DISPATCH_C(C, crf_forward_kernel<CC><<<(unsigned)p.blocks, NT, lds, st>>>(
                          q_out, q_in, unary, xyz, mask, kernel_gamma, kernel_alpha, theta_beta, weight_smoothness,
                          weight_appearance, compat, p.g));
  }
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_crf_rnn_backward_scratch(int64_t* elems, int B, int C, int H, int W, int num_iters) {
  Plan p;
  if (!elems || !plan_for(p, B, C, H, W, 1, 1, num_iters)) return DGV2_EINVAL;
  *elems = scratch_elems_for(p, C, num_iters);
  return 0;
}

extern "C" int dgv2_crf_rnn_backward(float* g_unary, float* g_weight_smoothness, float* g_weight_appearance,
                                     float* g_compat, float* scratch, int64_t scratch_elems, const float* g_out,
                                     const float* qsave, const float* unary, const float* xyz, const float* mask,
                                     const float* kernel_gamma, const float* kernel_alpha, const float* theta_beta,
                                     const float* weight_smoothness, const float* weight_appearance,
                                     const float* compat, int B, int C, int H, int W, int kh, int kw, int num_iters,
                                     void* stream) {
  Plan p;
  if (!g_unary || !g_weight_smoothness || !g_weight_appearance || !g_compat || !scratch || !g_out || !unary || !xyz ||
      !mask || !kernel_gamma || !kernel_alpha || !theta_beta || !weight_smoothness || !weight_appearance || !compat ||
      !plan_for(p, B, C, H, W, kh, kw, num_iters) || (num_iters > 1 && !qsave))
    return DGV2_EINVAL;
  if (scratch_elems < scratch_elems_for(p, C, num_iters)) return DGV2_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const int nout = 2 * C + C * C;
  float *fields = scratch, *gq = scratch + 3 * p.bchw, *part = scratch + 4 * p.bchw;
  const size_t lds_fields = lds_bytes(p, C + 4), lds_gather = lds_bytes(p, 3 * C + 4);
  for (int t = num_iters - 1; t >= 0; --t) {
    const float* q_in = t == 0 ? unary : qsave + (int64_t)(t - 1) * p.bchw;
    const float* dq = t == num_iters - 1 ? g_out : gq;
    float* part_t = part + (int64_t)t * p.blocks * nout;
    // the last iteration's input cotangent joins g_unary; the others become the next dq
    float* dq_out = t == 0 ? g_unary : gq;
    CRF_DISPATCH_C(C, {
      crf_backward_fields_kernel<CC><<<(unsigned)p.blocks, NT, lds_fields, st>>>(
          fields, part_t, g_unary, t != num_iters - 1, dq, q_in, xyz, mask, kernel_gamma, kernel_alpha, theta_beta,
          weight_smoothness, weight_appearance, compat, p.bchw, p.g);
      crf_backward_gather_kernel<CC><<<(unsigned)p.blocks, NT, lds_gather, st>>>(
          dq_out, t == 0, fields, q_in, xyz, mask, kernel_gamma, kernel_alpha, theta_beta, p.bchw, p.g);
    });
  }
  crf_param_finish_kernel<<<nout, NT, 0, st>>>(g_weight_smoothness, g_weight_appearance, g_compat, part,
                                               (int64_t)num_iters * p.blocks, C);
  DGV2_RETURN_LAST();
}
