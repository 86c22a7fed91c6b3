// Training objective of the range-image segmentation models: masked focal loss, predictions and training confusion
// counts in one pass over the logits, and the logits' gradient in another (reference: FocalLoss.forward,
// semseg/models/loss.py:13-21, under masked_loss, train_semseg.py:194-197, with the argmax and the masked sums of its
// lines 270-273 and 290-296; include/dgv2.h states the arithmetic).
//
// A thread owns PX = 4 consecutive pixels of the flattened [B*H*W] pixel list, whatever the logits' dtype and whatever
// the pointers' alignment: with 16-byte aligned pointers and H*W a multiple of 4 it reads a class plane with one 16-byte
// (fp32) or 8-byte (bf16 / fp16) load and writes its outputs with 16-byte stores, otherwise element by element -- the
// pixel -> (block, thread, turn) map, and with it the order of every float sum, depends on the pixel count alone.  That
// and -ffp-contract=off (Makefile) make the results of the two paths, and of a half-precision tensor and its fp32 cast,
// the same bits.
//
// C <= 4 and C <= 8 keep a pixel's logits in registers (the planes are read from HBM once); 8 < C <= 32 walk the planes
// twice (max / argmax, then the sums; the backward a third time for the gradient), the re-reads hitting the lines the
// block has just pulled into L2.
//
// The float sums: a thread adds its pixels in order, a block folds its threads in a fixed tree and stores {sum m L,
// sum m} into scratch[2 * block]; a second launch of ONE block folds those in a fixed order and divides.  No float
// atomics.  The confusion counts go through an LDS histogram with integer atomics as in segcount.hip.
#include "common.h"

namespace {

// The forward ends with one 64-bit atomic per non-empty bin and block on the same (C+1)^2 words, which serialise at
// the memory side: two blocks per CU, as segcount.hip.  The grid is the same with and without `conf`, so
// that the loss is the same bits either way.  The backward has no atomics and fills the chip.
constexpr int NT = 256, PX = 4, C_MAX = 32, LDS_WORDS = 4096, FWD_BLOCKS = 512, BWD_BLOCKS = 2048;

typedef _Float16 f16_t;
__device__ __forceinline__ float px_f32(float v) { return v; }
__device__ __forceinline__ float px_f32(bf16_t v) { return (float)v; }
__device__ __forceinline__ float px_f32(f16_t v) { return (float)v; }
// fp32 -> T, round to nearest even
template <typename T> __device__ __forceinline__ T px_from(float v) { return (T)v; }
// The empty asm keeps the compiler from folding the product that made v into the conversion (v_fma_mixlo_f16 rounds
// a * b to half ONCE, whatever -ffp-contract says): the gradient is the fp32 gradient rounded to half, bit for bit.
template <> __device__ __forceinline__ f16_t px_from<f16_t>(float v) {
  asm("" : "+v"(v));
  return (f16_t)v;
}

template <typename T> struct px4 {
  union {
    T e[PX];
    float4 v16;   // sizeof(T) == 4
    uint2 v8;     // sizeof(T) == 2
  };
};

struct Shape {
  int64_t n, hw;   // pixels, pixels per sample
  int C, vec;
};

// element offsets of the group's pixels into class plane 0 of their samples; cnt pixels exist
struct Group {
  int64_t off[PX];
  int64_t first;
  int cnt;
};

__device__ __forceinline__ Group group_of(int64_t g, const Shape& s) {
  Group r;
  r.first = g * PX;
  r.cnt = (int)(s.n - r.first < PX ? s.n - r.first : PX);
  if (s.vec) {   // hw % PX == 0: the group lies in one sample
    const int64_t b = r.first / s.hw;
    const int64_t o = b * s.C * s.hw + (r.first - b * s.hw);
#pragma unroll
    for (int k = 0; k < PX; ++k) r.off[k] = o + k;
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int64_t i = r.first + (k < r.cnt ? k : 0), b = i / s.hw;
      r.off[k] = b * s.C * s.hw + (i - b * s.hw);
    }
  }
  return r;
}

template <typename T>
__device__ __forceinline__ void load_plane(const T* __restrict__ logit, const Group& g, const Shape& s, int c, T (&raw)[PX]) {
  const int64_t plane = (int64_t)c * s.hw;
  if (s.vec) {
    px4<T> t;
    if constexpr (sizeof(T) == 4) t.v16 = *reinterpret_cast<const float4*>(logit + g.off[0] + plane);
    else t.v8 = *reinterpret_cast<const uint2*>(logit + g.off[0] + plane);
#pragma unroll
    for (int k = 0; k < PX; ++k) raw[k] = t.e[k];
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) raw[k] = k < g.cnt ? logit[g.off[k] + plane] : (T)0.f;
  }
}

template <typename T>
__device__ __forceinline__ void store_plane(T* __restrict__ out, const Group& g, const Shape& s, int c, const float (&v)[PX]) {
  const int64_t plane = (int64_t)c * s.hw;
  px4<T> t;
#pragma unroll
  for (int k = 0; k < PX; ++k) t.e[k] = px_from<T>(v[k]);
  if (s.vec) {
    if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(out + g.off[0] + plane) = t.v16;
    else *reinterpret_cast<uint2*>(out + g.off[0] + plane) = t.v8;
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k)
      if (k < g.cnt) out[g.off[k] + plane] = t.e[k];
  }
}

__device__ __forceinline__ void load_label_mask(const int64_t* __restrict__ label, const float* __restrict__ mask,
                                                const Group& g, const Shape& s, int64_t (&y)[PX], float (&m)[PX]) {
  if (s.vec) {
    const longlong2 a = reinterpret_cast<const longlong2*>(label + g.first)[0], b = reinterpret_cast<const longlong2*>(label + g.first)[1];
    y[0] = a.x; y[1] = a.y; y[2] = b.x; y[3] = b.y;
    float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
    if (mask) w = *reinterpret_cast<const float4*>(mask + g.first);
    m[0] = w.x; m[1] = w.y; m[2] = w.z; m[3] = w.w;
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      y[k] = k < g.cnt ? label[g.first + k] : -1;
      m[k] = k < g.cnt ? (mask ? mask[g.first + k] : 1.f) : 0.f;
    }
  }
}

// What one pixel's softmax leaves behind: max, lowest index of the max, sum exp(z - max) over all classes and over
// the classes other than the label (1 - p_y = others / sum without cancellation), the label's logit.
struct Soft {
  float mx, sum, others, zy;
  int best;
};

// (1 - p_y)^(gamma - 1) and (1 - p_y)^gamma; gamma == 0 is decided by the callers
__device__ __forceinline__ void focal_powers(float q, float gamma, float& qm1, float& qg) {
  if (gamma == 1.f) {
    qm1 = 1.f;
    qg = q;
  } else if (gamma == 2.f) {
    qm1 = q;
    qg = q * q;
  } else {
    qm1 = powf(q, gamma - 1.f);
    qg = qm1 * q;
  }
}

// Runs the class loops of one group.  CT > 0: the planes are loaded once into registers (C <= CT); CT == 0: every
// walk re-loads them.
template <int CT> constexpr int unroll_of = CT > 0 ? CT : 1;
#define SEGLOSS_FOR_C(c) _Pragma("unroll unroll_of<CT>") for (int c = 0; c < (CT > 0 ? CT : s.C); ++c) if (CT == 0 || c < s.C)

template <typename T, int CT> struct Planes {
  T z[CT > 0 ? CT : 1][PX];
  const T* __restrict__ logit;
  __device__ __forceinline__ void init(const T* p, const Group& g, const Shape& s) {
    logit = p;
    if constexpr (CT > 0) {
      SEGLOSS_FOR_C(c) load_plane(logit, g, s, c, z[c]);
    }
  }
  __device__ __forceinline__ void get(const Group& g, const Shape& s, int c, T (&raw)[PX]) const {
    if constexpr (CT > 0) {
#pragma unroll
      for (int k = 0; k < PX; ++k) raw[k] = z[c][k];
    } else {
      load_plane(logit, g, s, c, raw);
    }
  }
};

template <typename T, int CT>
__device__ __forceinline__ void softmax_of(const Planes<T, CT>& pl, const Group& g, const Shape& s, const int64_t (&y)[PX],
                                           Soft (&sm)[PX]) {
  T raw[PX];
  // the comparison runs on the values' own dtype: the conversion to fp32 is exact and monotonic
#pragma unroll
  for (int k = 0; k < PX; ++k) sm[k] = Soft{0.f, 0.f, 0.f, 0.f, 0};
  SEGLOSS_FOR_C(c) {
    pl.get(g, s, c, raw);
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const float z = px_f32(raw[k]);
      if (c == 0 || z > sm[k].mx) {
        sm[k].mx = z;
        sm[k].best = c;
      }
    }
  }
  SEGLOSS_FOR_C(c) {
    pl.get(g, s, c, raw);
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const float z = px_f32(raw[k]), e = expf(z - sm[k].mx);
      sm[k].sum += e;
      if (y[k] == c) sm[k].zy = z;
      else sm[k].others += e;
    }
  }
}

__device__ __forceinline__ int bin_of(int64_t v, int C) { return (v >= 0 && v < C) ? (int)v : C; }

struct FwdArgs {
  float* loss_map;
  int64_t* pred;
  unsigned long long* conf;
  float* partial;   // [2 * gridDim.x] or NULL
  const void* logit;
  const int64_t* label;
  const float* mask;
  const float* alpha;
  Shape s;
  float gamma;
  int copies;
};

template <typename T, int CT> __global__ __launch_bounds__(NT) void seg_loss_fwd_kernel(FwdArgs a) {
  __shared__ unsigned hist[LDS_WORDS];
  __shared__ float red[2][NT / DGV2_WAVE];
  const Shape s = a.s;
  const int bins = (s.C + 1) * (s.C + 1), mine = threadIdx.x & (a.copies - 1);
  if (a.conf) {
    for (int i = threadIdx.x; i < bins * a.copies; i += NT) hist[i] = 0u;
    __syncthreads();
  }
  const T* logit = static_cast<const T*>(a.logit);
  const int64_t groups = (s.n + PX - 1) / PX, stride = (int64_t)gridDim.x * NT;
  float num = 0.f, den = 0.f;
  for (int64_t gi = (int64_t)blockIdx.x * NT + threadIdx.x; gi < groups; gi += stride) {
    const Group g = group_of(gi, s);
    int64_t y[PX];
    float m[PX];
    load_label_mask(a.label, a.mask, g, s, y, m);
    Planes<T, CT> pl;
    pl.init(logit, g, s);
    Soft sm[PX];
    softmax_of(pl, g, s, y, sm);
    float L[PX];
    int64_t p[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const bool in_range = y[k] >= 0 && y[k] < s.C;
      float w = 1.f;
      if (a.gamma != 0.f) {
        float qm1;
        focal_powers(sm[k].others / sm[k].sum, a.gamma, qm1, w);
      }
      const float nlp = logf(sm[k].sum) - (sm[k].zy - sm[k].mx);   // -log p_y >= 0
      const float ay = in_range && a.alpha ? a.alpha[y[k]] : 1.f;
      L[k] = in_range ? ay * (w * nlp) : 0.f;
      const bool keep = m[k] != 0.f;
      p[k] = keep ? sm[k].best : 0;
      if (k < g.cnt) {
        num += m[k] * L[k];
        den += m[k];
        if (a.conf) atomicAdd(&hist[((keep ? bin_of(y[k], s.C) : 0) * (s.C + 1) + (int)p[k]) * a.copies + mine], 1u);
      }
    }
    if (a.loss_map) {
      if (s.vec) {
        *reinterpret_cast<float4*>(a.loss_map + g.first) = make_float4(L[0], L[1], L[2], L[3]);
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
          if (k < g.cnt) a.loss_map[g.first + k] = L[k];
      }
    }
    if (a.pred) {
      if (s.vec) {
        longlong2 lo, hi;
        lo.x = p[0]; lo.y = p[1]; hi.x = p[2]; hi.y = p[3];
        reinterpret_cast<longlong2*>(a.pred + g.first)[0] = lo;
        reinterpret_cast<longlong2*>(a.pred + g.first)[1] = hi;
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
          if (k < g.cnt) a.pred[g.first + k] = p[k];
      }
    }
  }
  if (a.partial) {   // fixed tree: lanes of a wave, then the block's waves in order
    num = wave_sum(num);
    den = wave_sum(den);
    if ((threadIdx.x & (DGV2_WAVE - 1)) == 0) {
      red[0][threadIdx.x / DGV2_WAVE] = num;
      red[1][threadIdx.x / DGV2_WAVE] = den;
    }
  }
  __syncthreads();
  if (a.partial && threadIdx.x == 0) {
    float sn = 0.f, sd = 0.f;
    for (int i = 0; i < NT / DGV2_WAVE; ++i) {
      sn += red[0][i];
      sd += red[1][i];
    }
    a.partial[2 * blockIdx.x] = sn;
    a.partial[2 * blockIdx.x + 1] = sd;
  }
  if (a.conf) {
    for (int bin = threadIdx.x; bin < bins; bin += NT) {
      unsigned long long c = 0;
      for (int r = 0; r < a.copies; ++r) c += hist[bin * a.copies + r];
      if (c) atomicAdd(&a.conf[bin], c);
    }
  }
}

// sums = {num / den, num, den} from the blocks' partials: thread t adds blocks t, t + NT, ... in order, then the tree
__global__ __launch_bounds__(NT) void seg_loss_fold_kernel(float* __restrict__ sums, const float* __restrict__ partial, int blocks) {
  __shared__ float red[2][NT / DGV2_WAVE];
  float num = 0.f, den = 0.f;
  for (int i = threadIdx.x; i < blocks; i += NT) {
    num += partial[2 * i];
    den += partial[2 * i + 1];
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if ((threadIdx.x & (DGV2_WAVE - 1)) == 0) {
    red[0][threadIdx.x / DGV2_WAVE] = num;
    red[1][threadIdx.x / DGV2_WAVE] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sn = 0.f, sd = 0.f;
    for (int i = 0; i < NT / DGV2_WAVE; ++i) {
      sn += red[0][i];
      sd += red[1][i];
    }
    sums[0] = sn / sd;   // 0 / 0 = NaN where nothing is masked in, as the reference
    sums[1] = sn;
    sums[2] = sd;
  }
}

struct BwdArgs {
  void* g_logit;
  const void* logit;
  const int64_t* label;
  const float* mask;
  const float* alpha;
  const float* gout;   // one value, or [n] when per_pixel
  const float* sums;
  Shape s;
  float gamma;
  int per_pixel;
};

template <typename T, int CT> __global__ __launch_bounds__(NT) void seg_loss_bwd_kernel(BwdArgs a) {
  const Shape s = a.s;
  const T* logit = static_cast<const T*>(a.logit);
  T* g_logit = static_cast<T*>(a.g_logit);
  const int64_t groups = (s.n + PX - 1) / PX, stride = (int64_t)gridDim.x * NT;
  float up = 0.f, den = 1.f;
  if (!a.per_pixel) {
    up = a.gout[0];
    den = a.sums[2];
  }
  for (int64_t gi = (int64_t)blockIdx.x * NT + threadIdx.x; gi < groups; gi += stride) {
    const Group g = group_of(gi, s);
    int64_t y[PX];
    float m[PX];
    load_label_mask(a.label, a.per_pixel ? a.gout : a.mask, g, s, y, m);   // per pixel: m is gout(q)
    Planes<T, CT> pl;
    pl.init(logit, g, s);
    Soft sm[PX];
    softmax_of(pl, g, s, y, sm);
    float coef[PX], q[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const bool in_range = y[k] >= 0 && y[k] < s.C;
      q[k] = sm[k].others / sm[k].sum;
      float t = 1.f;
      if (a.gamma != 0.f) {
        float qm1, qg;
        focal_powers(q[k], a.gamma, qm1, qg);
        const float nlp = logf(sm[k].sum) - (sm[k].zy - sm[k].mx), py = expf(sm[k].zy - sm[k].mx) / sm[k].sum;
        t = ((a.gamma * py) * qm1) * nlp + qg;   // -(gamma p_y (1-p_y)^(gamma-1) log p_y - (1-p_y)^gamma)
      }
      const float scale = a.per_pixel ? m[k] : (up * m[k]) / den;
      const float ay = in_range && a.alpha ? a.alpha[y[k]] : 1.f;
      coef[k] = in_range ? scale * (ay * t) : 0.f;
    }
    T raw[PX];
    SEGLOSS_FOR_C(c) {
      pl.get(g, s, c, raw);
      float gz[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        const float pj = expf(px_f32(raw[k]) - sm[k].mx) / sm[k].sum;
        // a_y (p_j - delta_jy) t, with 1 - p_y taken from the other classes' sum; a label outside [0, C): coef = 0
        gz[k] = coef[k] * (y[k] == c ? -q[k] : pj);
      }
      store_plane(g_logit, g, s, c, gz);
    }
  }
}

bool gamma_ok(float gamma) { return gamma == 0.f || gamma >= 1.f; }   // NaN fails both

int64_t fwd_grid(int64_t n) { return grid_for((n + PX - 1) / PX, NT, FWD_BLOCKS); }

template <typename T> void launch_fwd(const FwdArgs& a, int grid, hipStream_t st) {
  if (a.s.C <= 4) seg_loss_fwd_kernel<T, 4><<<grid, NT, 0, st>>>(a);
  else if (a.s.C <= 8) seg_loss_fwd_kernel<T, 8><<<grid, NT, 0, st>>>(a);
  else seg_loss_fwd_kernel<T, 0><<<grid, NT, 0, st>>>(a);
}

template <typename T> void launch_bwd(const BwdArgs& a, int grid, hipStream_t st) {
  if (a.s.C <= 4) seg_loss_bwd_kernel<T, 4><<<grid, NT, 0, st>>>(a);
  else if (a.s.C <= 8) seg_loss_bwd_kernel<T, 8><<<grid, NT, 0, st>>>(a);
  else seg_loss_bwd_kernel<T, 0><<<grid, NT, 0, st>>>(a);
}

bool shape_ok(int B, int C, int H, int W, int dtype, float gamma) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || C > C_MAX) return false;
  if (dtype != DGV2_F32 && dtype != DGV2_BF16 && dtype != DGV2_F16) return false;
  if ((int64_t)B * H * W >= (1LL << 40)) return false;
  return gamma_ok(gamma);
}

}  // namespace

extern "C" int dgv2_seg_loss_scratch(int64_t* elems, int B, int H, int W) {
  if (!elems || B < 1 || H < 1 || W < 1 || (int64_t)B * H * W >= (1LL << 40)) return DGV2_EINVAL;
  *elems = 2 * fwd_grid((int64_t)B * H * W);
  return 0;
}

extern "C" int dgv2_seg_loss_forward(float* loss_map, int64_t* pred, int64_t* conf, float* sums, float* scratch,
                                     int64_t scratch_elems, const void* logit, const int64_t* label, const float* mask,
                                     const float* alpha, int B, int C, int H, int W, float gamma, int dtype,
                                     void* stream) {
  if (!logit || !label || !(loss_map || pred || conf || sums) || !shape_ok(B, C, H, W, dtype, gamma)) return DGV2_EINVAL;
  const int64_t hw = (int64_t)H * W, n = B * hw;
  const int grid = (int)fwd_grid(n);
  if (sums && (!scratch || scratch_elems < 2 * (int64_t)grid)) return DGV2_EINVAL;
  FwdArgs a;
  a.loss_map = loss_map;
  a.pred = pred;
  a.conf = reinterpret_cast<unsigned long long*>(conf);
  a.partial = sums ? scratch : nullptr;
  a.logit = logit;
  a.label = label;
  a.mask = mask;
  a.alpha = alpha;
  a.s.n = n;
  a.s.hw = hw;
  a.s.C = C;
  a.s.vec = hw % PX == 0 && aligned16(logit) && aligned16(label) && aligned16(mask) && aligned16(loss_map) && aligned16(pred);
  a.gamma = gamma;
  const int bins = (C + 1) * (C + 1);
  a.copies = 1;
  while (a.copies < 64 && 2 * a.copies * bins <= LDS_WORDS) a.copies *= 2;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DGV2_F32) launch_fwd<float>(a, grid, st);
  else if (dtype == DGV2_BF16) launch_fwd<bf16_t>(a, grid, st);
  else launch_fwd<f16_t>(a, grid, st);
  if (sums) seg_loss_fold_kernel<<<1, NT, 0, st>>>(sums, scratch, grid);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_seg_loss_backward(void* g_logit, const void* logit, const int64_t* label, const float* mask,
                                      const float* alpha, const float* gout, const float* sums, int B, int C, int H,
                                      int W, float gamma, int dtype, int per_pixel, void* stream) {
  if (!g_logit || !logit || !label || !gout || (per_pixel != 0 && per_pixel != 1) || (!per_pixel && !sums) ||
      !shape_ok(B, C, H, W, dtype, gamma))
    return DGV2_EINVAL;
  const int64_t hw = (int64_t)H * W, n = B * hw;
  BwdArgs a;
  a.g_logit = g_logit;
  a.logit = logit;
  a.label = label;
  a.mask = mask;
  a.alpha = alpha;
  a.gout = gout;
  a.sums = sums;
  a.s.n = n;
  a.s.hw = hw;
  a.s.C = C;
  a.s.vec = hw % PX == 0 && aligned16(logit) && aligned16(g_logit) && aligned16(label) && (per_pixel ? aligned16(gout) : aligned16(mask));
  a.gamma = gamma;
  a.per_pixel = per_pixel;
  const int grid = grid_for((n + PX - 1) / PX, NT, BWD_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DGV2_F32) launch_bwd<float>(a, grid, st);
  else if (dtype == DGV2_BF16) launch_bwd<bf16_t>(a, grid, st);
  else launch_bwd<f16_t>(a, grid, st);
  DGV2_RETURN_LAST();
}
