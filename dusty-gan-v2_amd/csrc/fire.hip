// Evaluation-mode Fire module of the SqueezeSeg trunks as ONE launch (include/dgv2.h, "Fire module", states the
// arithmetic; DESIGN.md section 31 the structure and the measurements).  gfx950 only.
//
// A block of eight waves owns TH x 32 output pixels of one sample.  Three stages, a barrier between them:
//   1  squeeze:  s = N_s(relu(W_s x + b_s)) for the tile plus its one-pixel halo, x read from HBM as the MFMA's B
//      operand, the result written to LDS as [pixel][Cs] in the activations' dtype; positions outside the image are 0.
//   1b (up only) transposed conv as a GEMM over K = 4 Cs (tap, channel): the B operand of output column w' and tap k is
//      s at w = (w' + 1 - k) / 2 where that is an integer inside [0, W), else 0.  u = relu(. + b_d) into a second LDS
//      image, 0 outside the image (the 3x3's zero padding applies to u, not to x).
//   2  both expands as GEMMs out of the u image (K = Cs and K = 9 Cs); bias, ReLU, affine, the
//      optional skip, and the one store of the block's slice of the concatenated output.
// D[channel][pixel] orientation everywhere: the weights are the A operand (read from the module's float32 tensors, L1 /
// L2-served, converted in registers), the activations the B operand, so that a store instruction covers 16 consecutive
// pixels of 4 channels.  Operands are 16-byte K-chunks: 8 values for the 16 x 16 x 32 bf16 / f16 MFMA, 4 values fed to
// four exact 16 x 16 x 4 f32 MFMAs (both operands agree on the k a lane holds, which is all the MFMA asks).
// No atomics, no scratch; every output element is one k-ordered chain, so the bits do not depend on the grid.
#include "common.h"

namespace {

typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

constexpr int FIRE_TW = 32;   // output columns per block
constexpr int FIRE_SW = 18;   // squeezed columns an up-sampling block needs: w' in [ow0 - 1, ow0 + 32] -> w in [ow0/2 - 1, ow0/2 + 16]
constexpr int FIRE_WAVES = 8;
constexpr int FIRE_THREADS = 64 * FIRE_WAVES;

struct FireBN {
  const float *g, *b, *m, *v;
  float eps;
};

struct FireP {
  void* y;
  const void *x, *skip;
  const float *ws, *bs, *wd, *bd, *w1, *b1, *w3, *b3;
  FireBN ns, n1, n3;
  int B, Cin, Cs, E1, E3, H, W, up, tiles_x, tiles_y;
};

union Chunk {
  uint4 u;
  float f[4];
  bf16x8 b;
  f16x8 h;
  bf16_t be[8];
  f16_t he[8];
};

__device__ __forceinline__ void chunk_set(Chunk& c, int j, float v, float*) { c.f[j] = v; }
__device__ __forceinline__ void chunk_set(Chunk& c, int j, float v, bf16_t*) { c.be[j] = (bf16_t)v; }
__device__ __forceinline__ void chunk_set(Chunk& c, int j, float v, f16_t*) { c.he[j] = (f16_t)v; }

__device__ __forceinline__ void mma(f32x4& acc, const Chunk& a, const Chunk& b, float*) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.f[j], b.f[j], acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, const Chunk& a, const Chunk& b, bf16_t*) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.b, b.b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, const Chunk& a, const Chunk& b, f16_t*) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h, b.h, acc, 0, 0, 0);
}

// The A chunk of output channel row `p` (K-contiguous float32 weights: the two 1x1 convs) at k-block kb: KE consecutive
// floats as 16-byte loads (kb is a multiple of 4 and every row a multiple of 16 floats long).  Zero beyond K.
template <typename T>
__device__ __forceinline__ Chunk load_a_row(const float* __restrict__ p, int kb, int K) {
  constexpr int KE = 16 / sizeof(T);
  Chunk a;
  a.u = make_uint4(0u, 0u, 0u, 0u);
  if (kb < K) {
#pragma unroll
    for (int q = 0; q < KE / 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + kb + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) chunk_set(a, 4 * q + j, v[j], (T*)nullptr);
    }
  }
  return a;
}

// KE input channels x NTAP taps of one output channel, for weights whose taps are contiguous: `p` points at (channel
// c0, tap 0), channel c at p + c * cstride.  With cstride == NTAP (the 3x3 conv: [E3][Cs][9]) the block is one run of
// KE * 9 floats, read as 16-byte loads: a lane touches three or four cache lines where nine strided k-steps touch 8 each.
template <int KE, int NTAP> struct ABlock {
  float v[KE][NTAP];
};
template <int KE>
__device__ __forceinline__ void load_block9(ABlock<KE, 9>& blk, const float* __restrict__ p, bool valid) {
  float raw[KE * 9];
#pragma unroll
  for (int q = 0; q < KE * 9 / 4; ++q) {
    const f32x4 v = valid ? *reinterpret_cast<const f32x4*>(p + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[4 * q + j] = v[j];
  }
#pragma unroll
  for (int c = 0; c < KE; ++c)
#pragma unroll
    for (int t = 0; t < 9; ++t) blk.v[c][t] = raw[c * 9 + t];
}
template <int KE>
__device__ __forceinline__ void load_block4(ABlock<KE, 4>& blk, const float* __restrict__ p, int64_t cstride, bool valid) {
#pragma unroll
  for (int c = 0; c < KE; ++c) {
    const f32x4 v = valid ? *reinterpret_cast<const f32x4*>(p + c * cstride) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) blk.v[c][t] = v[t];
  }
}
template <typename T, int KE, int NTAP>
__device__ __forceinline__ Chunk block_tap(const ABlock<KE, NTAP>& blk, int t) {
  Chunk a;
  a.u = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int c = 0; c < KE; ++c) chunk_set(a, c, blk.v[c][t], (T*)nullptr);
  return a;
}

__device__ __forceinline__ float bn_apply(float v, const FireBN& n, int c) {
  if (n.g == nullptr) return v;
  const float sc = n.g[c] * (1.0f / sqrtf(n.v[c] + n.eps));
  return (v - n.m[c]) * sc + n.b[c];
}

// four consecutive channels of one pixel into an LDS image
__device__ __forceinline__ void lds_put4(unsigned char* at, const float (&v)[4], float*) {
  *reinterpret_cast<f32x4*>(at) = f32x4{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ void lds_put4(unsigned char* at, const float (&v)[4], bf16_t*) {
  union { uint2 u; bf16_t e[4]; } q;
#pragma unroll
  for (int r = 0; r < 4; ++r) q.e[r] = (bf16_t)v[r];
  *reinterpret_cast<uint2*>(at) = q.u;
}
__device__ __forceinline__ void lds_put4(unsigned char* at, const float (&v)[4], f16_t*) {
  union { uint2 u; f16_t e[4]; } q;
#pragma unroll
  for (int r = 0; r < 4; ++r) q.e[r] = (f16_t)v[r];
  *reinterpret_cast<uint2*>(at) = q.u;
}

template <typename T, int TH>
__global__ __launch_bounds__(FIRE_THREADS) void fire_fwd_kernel(const FireP p) {
  constexpr int TW = FIRE_TW, UH = TH + 2, UW = TW + 2, SW = FIRE_SW, NW = FIRE_WAVES;
  constexpr int KE = 16 / sizeof(T), KS = 4 * KE;
  constexpr int NB = ((UH * UW + 15) / 16 + NW - 1) / NW;   // pixel tiles of the haloed image per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char fire_lds[];
  T* const tag = nullptr;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int Cin = p.Cin, Cs = p.Cs, H = p.H, W = p.W;
  const int Wout = p.up ? 2 * W : W;
  const int64_t HW = (int64_t)H * W;

  int t = blockIdx.x;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, b = t / p.tiles_y;
  const int oh0 = ty * TH, ow0 = tx * TW;

  const int pstride = Cs * (int)sizeof(T) + 16;   // bytes per pixel of an LDS image: 16 of padding against bank conflicts
  unsigned char* const u_lds = fire_lds;
  unsigned char* const s_lds = fire_lds + UH * UW * pstride;   // up only
  const int MS = Cs >> 4;

  // ---- stage 1: squeeze --------------------------------------------------------------------------------------------
  // a wave owns the pixel tiles wave, wave + NW, ... and walks K once for all of them: a weight chunk is loaded once
  // per k-step and 16-channel tile and feeds NB MFMAs
  {
    unsigned char* const dst = p.up ? s_lds : u_lds;
    const int PW = p.up ? SW : UW, NP = UH * PW;
    const int c0 = p.up ? (ow0 >> 1) - 1 : ow0 - 1;
    const T* const x = reinterpret_cast<const T*>(p.x) + (int64_t)b * Cin * HW;
    const T* xp[NB];
    bool in[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int pp = (wave + n * NW) * 16 + lr;
      const int row = pp / PW, col = pp - row * PW;
      const int ih = oh0 - 1 + row, iw = c0 + col;
      in[n] = pp < NP && ih >= 0 && ih < H && iw >= 0 && iw < W;
      xp[n] = x + (in[n] ? (int64_t)ih * W + iw : 0);
    }
    if (wave * 16 < NP) {
      f32x4 acc[4][NB];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < Cin; k0 += KS) {
        const int kb = k0 + KE * lq;
        Chunk bf[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          bf[n].u = make_uint4(0u, 0u, 0u, 0u);
          if (in[n] && kb < Cin) {
            if constexpr (sizeof(T) == 4) {
#pragma unroll
              for (int j = 0; j < KE; ++j) bf[n].f[j] = (float)xp[n][(int64_t)(kb + j) * HW];
            } else {
              union { T e[8]; uint4 u; } q;
#pragma unroll
              for (int j = 0; j < KE; ++j) q.e[j] = xp[n][(int64_t)(kb + j) * HW];
              bf[n].u = q.u;
            }
          }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m < MS) {
            const Chunk af = load_a_row<T>(p.ws + (int64_t)(m * 16 + lr) * Cin, kb, Cin);
#pragma unroll
            for (int n = 0; n < NB; ++n) mma(acc[m][n], af, bf[n], tag);
          }
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int pp = (wave + n * NW) * 16 + lr;
        if (pp < NP) {
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (m < MS) {
              float v[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int c = m * 16 + lq * 4 + r;
                v[r] = in[n] ? bn_apply(fmaxf(acc[m][n][r] + p.bs[c], 0.f), p.ns, c) : 0.f;
              }
              lds_put4(dst + pp * pstride + (m * 16 + lq * 4) * (int)sizeof(T), v, tag);
            }
        }
      }
    }
  }
  __syncthreads();

  // ---- stage 1b: transposed conv (1,4), stride (1,2), padding (0,1) -------------------------------------------------
  // k runs over (channel block, tap, channel in block): the four taps of a (ci, co) pair are one 16-byte load
  if (p.up) {
    constexpr int NP = UH * UW;
    const int c0 = (ow0 >> 1) - 1;
    for (int nt = wave; nt * 16 < NP; nt += NW) {
      const int pp = nt * 16 + lr;
      const int row = pp / UW, col = pp - row * UW;
      const int oh = oh0 - 1 + row, ow = ow0 - 1 + col;
      const bool in = pp < NP && oh >= 0 && oh < H && ow >= 0 && ow < Wout;
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int cb0 = 0; cb0 < Cs; cb0 += KS) {
        const int cb = cb0 + KE * lq;
        const bool kin = cb < Cs;
        Chunk bf[4];
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
          bf[tap].u = make_uint4(0u, 0u, 0u, 0u);
          const int e = ow + 1 - tap;             // = 2 w where the tap lands on an input column
          const int sc = (e >> 1) - c0;           // column of the s image; rows / columns outside the image hold 0
          if (in && kin && (e & 1) == 0 && sc >= 0 && sc < SW)
            bf[tap].u = *reinterpret_cast<const uint4*>(s_lds + (row * SW + sc) * pstride + cb * (int)sizeof(T));
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m < MS) {
            ABlock<KE, 4> blk;
            load_block4<KE>(blk, p.wd + ((int64_t)(kin ? cb : 0) * Cs + m * 16 + lr) * 4, (int64_t)Cs * 4, kin);
#pragma unroll
            for (int tap = 0; tap < 4; ++tap) mma(acc[m], block_tap<T, KE, 4>(blk, tap), bf[tap], tag);
          }
      }
      if (pp < NP) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m < MS) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = in ? fmaxf(acc[m][r] + p.bd[m * 16 + lq * 4 + r], 0.f) : 0.f;
            lds_put4(u_lds + pp * pstride + (m * 16 + lq * 4) * (int)sizeof(T), v, tag);
          }
      }
    }
    __syncthreads();
  }

  // ---- stage 2: both expands, epilogue, store ------------------------------------------------------------------------
  // items = (16-channel tile, half of the block's pixel tiles); the nine-tap tiles first, dealt round the waves.
  // The 3x3's k runs over (channel block, tap, channel in block): a lane's KE x 9 weights are one contiguous run.
  constexpr int NT = TH * TW / 16, NH = NT / 2;
  const int M1 = p.E1 >> 4, M3 = p.E3 >> 4, Cout = p.E1 + p.E3;
  const T* const skip = p.skip ? reinterpret_cast<const T*>(p.skip) + (int64_t)b * Cout * H * Wout : nullptr;
  T* const y = reinterpret_cast<T*>(p.y) + (int64_t)b * Cout * H * Wout;
  for (int it = wave; it < 2 * (M1 + M3); it += NW) {
    const bool is3 = it < 2 * M3;
    const int j = is3 ? it : it - 2 * M3;
    const int mt = j >> 1, half = j & 1;
    const int oc = mt * 16 + lr;
    f32x4 acc[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (is3) {
      for (int cb0 = 0; cb0 < Cs; cb0 += KS) {
        const int cb = cb0 + KE * lq;
        const bool kin = cb < Cs;
        ABlock<KE, 9> blk;
        load_block9<KE>(blk, p.w3 + ((int64_t)oc * Cs + (kin ? cb : 0)) * 9, kin);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3, dx = tap % 3;
          const Chunk af = block_tap<T, KE, 9>(blk, tap);
#pragma unroll
          for (int n = 0; n < NH; ++n) {
            const int nt = half * NH + n;
            const int r = nt >> 1, c = (nt & 1) * 16 + lr;
            Chunk bf;
            bf.u = make_uint4(0u, 0u, 0u, 0u);
            if (kin) bf.u = *reinterpret_cast<const uint4*>(u_lds + ((r + dy) * UW + c + dx) * pstride + cb * (int)sizeof(T));
            mma(acc[n], af, bf, tag);
          }
        }
      }
    } else {
      for (int k0 = 0; k0 < Cs; k0 += KS) {
        const int kb = k0 + KE * lq;
        const Chunk af = load_a_row<T>(p.w1 + (int64_t)oc * Cs, kb, Cs);
#pragma unroll
        for (int n = 0; n < NH; ++n) {
          const int nt = half * NH + n;
          const int r = nt >> 1, c = (nt & 1) * 16 + lr;
          Chunk bf;
          bf.u = make_uint4(0u, 0u, 0u, 0u);
          if (kb < Cs) bf.u = *reinterpret_cast<const uint4*>(u_lds + ((r + 1) * UW + c + 1) * pstride + kb * (int)sizeof(T));
          mma(acc[n], af, bf, tag);
        }
      }
    }
    const float* const bias = is3 ? p.b3 : p.b1;
    const FireBN& bn = is3 ? p.n3 : p.n1;
#pragma unroll
    for (int n = 0; n < NH; ++n) {
      const int nt = half * NH + n;
      const int oh = oh0 + (nt >> 1), ow = ow0 + (nt & 1) * 16 + lr;
      if (oh < H && ow < Wout) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = mt * 16 + lq * 4 + r;                // channel within its expand
          const int64_t o = ((int64_t)(is3 ? p.E1 + c : c) * H + oh) * Wout + ow;
          float v = bn_apply(fmaxf(acc[n][r] + bias[c], 0.f), bn, c);
          if (skip) v += (float)skip[o];
          y[o] = (T)v;
        }
      }
    }
  }
}

bool bn_ok(const FireBN& n) {
  const int k = (n.g != nullptr) + (n.b != nullptr) + (n.m != nullptr) + (n.v != nullptr);
  return k == 0 || k == 4;
}

template <typename T, int TH> int fire_launch(FireP p, hipStream_t st) {
  const int Wout = p.up ? 2 * p.W : p.W;
  const int64_t tx = (Wout + FIRE_TW - 1) / FIRE_TW, ty = (p.H + TH - 1) / TH;
  const int64_t blocks = tx * ty * p.B;
  if (blocks > 0x7fffffffLL) return DGV2_EINVAL;
  p.tiles_x = (int)tx;
  p.tiles_y = (int)ty;
  const int pstride = p.Cs * (int)sizeof(T) + 16;
  const size_t lds = (size_t)(TH + 2) * pstride * ((FIRE_TW + 2) + (p.up ? FIRE_SW : 0));
  if (lds > 65536) return DGV2_EINVAL;
  fire_fwd_kernel<T, TH><<<(unsigned)blocks, FIRE_THREADS, lds, st>>>(p);
  DGV2_RETURN_LAST();
}

}  // namespace

extern "C" int dgv2_fire_fwd(void* y, const void* x, const void* skip, const float* w_s, const float* b_s,
                             const float* g_s, const float* beta_s, const float* mean_s, const float* var_s,
                             const float* w_d, const float* b_d, const float* w_1, const float* b_1, const float* g_1,
                             const float* beta_1, const float* mean_1, const float* var_1, const float* w_3,
                             const float* b_3, const float* g_3, const float* beta_3, const float* mean_3,
                             const float* var_3, float eps_s, float eps_1, float eps_3, int B, int Cin, int Cs, int E1,
                             int E3, int H, int W, int up, int dtype, void* stream) {
  if (!y || !x || !w_s || !b_s || !w_1 || !b_1 || !w_3 || !b_3) return DGV2_EINVAL;
  if (up != 0 && up != 1) return DGV2_EINVAL;
  if (up ? (!w_d || !b_d) : (w_d || b_d)) return DGV2_EINVAL;
  if (B < 1 || H < 1 || W < 1 || W > (1 << 29)) return DGV2_EINVAL;
  if (Cin < 16 || Cin > 512 || Cin % 16 || Cs < 16 || Cs > 64 || Cs % 16) return DGV2_EINVAL;
  if (E1 < 16 || E1 > 256 || E1 % 16 || E3 < 16 || E3 > 256 || E3 % 16) return DGV2_EINVAL;
  FireP p;
  p.y = y; p.x = x; p.skip = skip;
  p.ws = w_s; p.bs = b_s; p.wd = w_d; p.bd = b_d; p.w1 = w_1; p.b1 = b_1; p.w3 = w_3; p.b3 = b_3;
  p.ns = FireBN{g_s, beta_s, mean_s, var_s, eps_s};
  p.n1 = FireBN{g_1, beta_1, mean_1, var_1, eps_1};
  p.n3 = FireBN{g_3, beta_3, mean_3, var_3, eps_3};
  if (!bn_ok(p.ns) || !bn_ok(p.n1) || !bn_ok(p.n3)) return DGV2_EINVAL;
  // the weights are read with 16-byte loads
  if (!aligned16(w_s) || !aligned16(w_1) || !aligned16(w_3) || (up && !aligned16(w_d))) return DGV2_EINVAL;
  if (!(eps_s >= 0.f) || !(eps_1 >= 0.f) || !(eps_3 >= 0.f)) return DGV2_EINVAL;
  p.B = B; p.Cin = Cin; p.Cs = Cs; p.E1 = E1; p.E3 = E3; p.H = H; p.W = W; p.up = up;
  p.tiles_x = p.tiles_y = 0;
  hipStream_t st = (hipStream_t)stream;
  // the float32 images are twice as wide per pixel: two output rows per block keep them inside 64 KiB at Cs = 64
  if (dtype == DGV2_F32) return fire_launch<float, 2>(p, st);
  if (dtype == DGV2_BF16) return fire_launch<bf16_t, 4>(p, st);
  if (dtype == DGV2_F16) return fire_launch<f16_t, 4>(p, st);
  return DGV2_EINVAL;
}
