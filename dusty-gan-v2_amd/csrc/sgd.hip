// The optimizer tail of the segmentation models' training step (reference: train_semseg.py:201-212 the SGD, 278-283
// GradScaler.unscale_ / clip_grad_norm_ / step / update, 360-362 the schedule that sets lr) over a LIST of parameter
// tensors: torch.optim.SGD with momentum and weight decay (dampening 0, no Nesterov), the global-norm clip and the loss
// scale folded into one factor.  As in adam.hip the parameters, gradients and momentum buffers of torch's own optimizer
// state stay separate tensors whose addresses travel by value in the kernel arguments: every launch is
// hipGraph-capturable, nothing is read on the host, and the optimizer's state_dict keeps torch's layout.
//   dgv2_sumsq_list  partials[l*64 + x] = sum of g[l][i]^2 over block x's share      (72 tensors per launch)
//   dgv2_clip_prep   sum = the partials added in double;  s = loss scale (1 without);  norm = sqrt(sum) / s
//                    sc = (norm, min(1, max_norm / (norm + 1e-6)) / s, overflow, s)  and GradScaler.update on the device
//   dgv2_sgd_step    d = sc[1] g + wd p;  m = mu m + d;  p -= lr m                    (72 tensors per launch; in double, rounded once)
// No atomics; every sum has a fixed order, so the bits repeat from run to run.  The Makefile compiles this file with
// -ffp-contract=off: the 16-byte and the element-wise path of a kernel must round alike, so the only fused
// multiply-adds are the ones written out in the sum of squares.
#include "common.h"

namespace {

constexpr int SG_MAX = 72;
constexpr int SG_THREADS = 256;
// the kernels index with int and step by up to 256 blocks x 256 threads: lengths this close to 2^31 are refused
constexpr int SG_N_MAX = DGV2_SGD_N_MAX;
static_assert(DGV2_SUMSQ_PARTS == 64, "the partials layout of dgv2_sumsq_list is part of the ABI");

struct SumsqArgs {
  const float* g[SG_MAX];
  int n[SG_MAX];
};

struct SgdArgs {
  float* p[SG_MAX];
  const float* g[SG_MAX];
  float* m[SG_MAX];
  int n[SG_MAX];
};

// Block (x, l) owns the 4-element groups q = x*256 + t, + 64*256, ... of tensor l and the tail elements
// (n & ~3) + x*256 + t (at most one per thread).  A thread adds its squares in index order; the 16-byte path and the
// element-wise path (a pointer off a 16-byte boundary) walk the SAME groups, so the bits depend on n alone.
__global__ __launch_bounds__(SG_THREADS) void sumsq_list_kernel(SumsqArgs a, float* __restrict__ partials) {
  __shared__ float red[16];
  const int l = blockIdx.y;
  const int n = a.n[l];
  const float* __restrict__ g = a.g[l];
  const int n4 = n >> 2;
  const int stride = DGV2_SUMSQ_PARTS * SG_THREADS;
  float acc = 0.f;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    for (int q = blockIdx.x * SG_THREADS + threadIdx.x; q < n4; q += stride) {
      const float4 v = reinterpret_cast<const float4*>(g)[q];
      acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
    }
  } else {
    for (int q = blockIdx.x * SG_THREADS + threadIdx.x; q < n4; q += stride) {
      const float* v = g + 4 * (int64_t)q;
      acc = fmaf(v[0], v[0], acc); acc = fmaf(v[1], v[1], acc); acc = fmaf(v[2], v[2], acc); acc = fmaf(v[3], v[3], acc);
    }
  }
  const int64_t i = ((int64_t)n4 << 2) + blockIdx.x * SG_THREADS + threadIdx.x;
  if (i < n) acc = fmaf(g[i], g[i], acc);
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) partials[l * DGV2_SUMSQ_PARTS + blockIdx.x] = s;
}

// One block.  Thread t adds the partials t, t + 256, ... in index order, in double; the 256 sums fold in a fixed tree.
// (The squares are fp32 values and there are at most a few ten thousand of them: in double the order of the additions
// moves the sum by parts in 1e-13, far below the fp32 rounding of sc; the fixed order is for repeatable bits.)
__global__ __launch_bounds__(SG_THREADS) void clip_prep_kernel(const float* __restrict__ partials, int count, float max_norm,
                                                               float* __restrict__ scale_state, float growth, float backoff,
                                                               int growth_interval, float* __restrict__ sc) {
  __shared__ double red[SG_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += SG_THREADS) acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = SG_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double sum = red[0];
  const double s = scale_state ? (double)scale_state[0] : 1.0;
  const double norm = sqrt(sum) / s;
  double coef = 1.0;
  if (max_norm > 0.f) {
    coef = (double)max_norm / (norm + 1e-6);
    coef = coef > 1.0 ? 1.0 : coef;   // a NaN norm stays NaN, as torch.clamp(max=1) leaves it
  }
  const bool overflow = scale_state && !(fabs(sum) <= 1.7976931348623157e308);
  sc[0] = (float)norm;
  sc[1] = (float)(coef / s);
  sc[2] = overflow ? 1.f : 0.f;
  sc[3] = (float)s;
  if (scale_state) {   // GradScaler.update
    if (overflow) {
      scale_state[0] = scale_state[0] * backoff;
      scale_state[1] = 0.f;
    } else {
      const float tracker = scale_state[1] + 1.f;
      if (tracker == (float)growth_interval) {
        scale_state[0] = scale_state[0] * growth;
        scale_state[1] = 0.f;
      } else {
        scale_state[1] = tracker;
      }
    }
  }
}

// MOM0 (momentum == 0): p -= lr d; the momentum buffers are neither read nor written (NULL allowed).
template <bool MOM0>
__global__ __launch_bounds__(SG_THREADS) void sgd_step_kernel(SgdArgs a, const float* __restrict__ sc, float lr, float mu,
                                                              float wd) {
  if (sc[2] != 0.f) return;   // overflow under a loss scale: GradScaler.step skips the optimizer
  const float f = sc[1];
  const int l = blockIdx.y;
  const int n = a.n[l];
  float* __restrict__ p = a.p[l];
  const float* __restrict__ g = a.g[l];
  float* __restrict__ m = a.m[l];
  // The update is evaluated in double from the fp32 operands and rounded once per stored value.  In fp32 the two
  // sums cancel often enough to matter -- a small gradient against the decay of a large weight, a gradient against the
  // decayed momentum -- and the error then scales with the terms, not with the result: over 166k elements the fp32
  // chain missed the bounds of DESIGN 34.2 (8 ulp of the RESULTS' magnitudes) on a handful.  The kernel moves 20 bytes
  // per element; its dozen double operations are far below the fp64 rate that traffic could feed.
  auto upd = [&](float& pp, float gg, float& mm) {
    const double d = (double)f * (double)gg + (double)wd * (double)pp;
    const double mn = MOM0 ? d : (double)mu * (double)mm + d;
    mm = (float)mn;
    pp = (float)((double)pp - (double)lr * mn);
  };
  uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
  if constexpr (!MOM0) bits |= reinterpret_cast<uintptr_t>(m);
  const int stride = gridDim.x * SG_THREADS;
  int first = blockIdx.x * SG_THREADS + threadIdx.x;   // first element of the element-wise loop
  if ((bits & 15) == 0) {
    const int n4 = n >> 2;
    for (int i = first; i < n4; i += stride) {
      float4 pp = reinterpret_cast<float4*>(p)[i];
      const float4 gg = reinterpret_cast<const float4*>(g)[i];
      float4 mm = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (!MOM0) mm = reinterpret_cast<float4*>(m)[i];
      upd(pp.x, gg.x, mm.x); upd(pp.y, gg.y, mm.y); upd(pp.z, gg.z, mm.z); upd(pp.w, gg.w, mm.w);
      reinterpret_cast<float4*>(p)[i] = pp;
      if constexpr (!MOM0) reinterpret_cast<float4*>(m)[i] = mm;
    }
    first += n4 << 2;
  }
  for (int i = first; i < n; i += stride) {
    float mm = 0.f;
    if constexpr (!MOM0) mm = m[i];
    upd(p[i], g[i], mm);
    if constexpr (!MOM0) m[i] = mm;
  }
}

}  // namespace

extern "C" int dgv2_sumsq_list(const float* const* g, const int* n, int L, float* partials, void* stream) {
  if (!g || !n || !partials || L < 1 || L > SG_MAX) return DGV2_EINVAL;
  SumsqArgs a;
  for (int l = 0; l < L; ++l) {
    if (!g[l] || n[l] < 0 || n[l] > SG_N_MAX) return DGV2_EINVAL;
    a.g[l] = g[l]; a.n[l] = n[l];
  }
  sumsq_list_kernel<<<dim3(DGV2_SUMSQ_PARTS, L), SG_THREADS, 0, (hipStream_t)stream>>>(a, partials);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_clip_prep(const float* partials, int count, float max_norm, float* scale_state, float growth,
                              float backoff, int growth_interval, float* sc, void* stream) {
  if (!partials || !sc || count < 1) return DGV2_EINVAL;
  clip_prep_kernel<<<1, SG_THREADS, 0, (hipStream_t)stream>>>(partials, count, max_norm, scale_state, growth, backoff,
                                                              growth_interval, sc);
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_sgd_step(float* const* p, const float* const* g, float* const* m, const int* n, int L, const float* sc,
                             float lr, float momentum, float weight_decay, void* stream) {
  const bool mom0 = momentum == 0.f;
  if (!p || !g || !n || !sc || (!m && !mom0) || L < 1 || L > SG_MAX) return DGV2_EINVAL;
  SgdArgs a;
  int nmax = 0;
  for (int l = 0; l < L; ++l) {
    if (!p[l] || !g[l] || n[l] < 0 || n[l] > SG_N_MAX || (!mom0 && !m[l])) return DGV2_EINVAL;
    a.p[l] = p[l]; a.g[l] = g[l]; a.m[l] = (m && !mom0) ? m[l] : nullptr; a.n[l] = n[l];
    nmax = n[l] > nmax ? n[l] : nmax;
  }
  dim3 grid(grid_for(nmax / 4 + 1, SG_THREADS, 256), L);
  if (mom0) sgd_step_kernel<true><<<grid, SG_THREADS, 0, (hipStream_t)stream>>>(a, sc, lr, momentum, weight_decay);
  else sgd_step_kernel<false><<<grid, SG_THREADS, 0, (hipStream_t)stream>>>(a, sc, lr, momentum, weight_decay);
  DGV2_RETURN_LAST();
}
