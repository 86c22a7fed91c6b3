// Synchronised batch norm of the segmentation models' data-parallel training (reference: train_semseg.py:172-174,
// SyncBatchNorm.convert_sync_batchnorm over the BatchNorm2d of semseg/models/common.py).  include/dgv2.h "Synchronised
// batch norm" states the arithmetic; this file states who adds what.
//   dgv2_bn_partials       part[b][c] = (sum x, sum x^2) of one (sample, channel) plane, float64
//   dgv2_bn_apply          fold of the gathered partials per channel, y, saved statistics, running buffers
//   dgv2_bn_bwd_partials   part[b][c] = (sum dy, sum dy xhat) of one plane, float64
//   dgv2_bn_bwd_apply      fold, dx, and the local dweight / dbias
// One 256-thread block per plane in all four.  The planes of the model are 8 KB to 128 KB (fp32); three to eight blocks
// are resident per CU (46 to 136 registers) and a thread keeps four 16-byte loads outstanding, so a CU has 48 to 128 KB
// of loads in flight -- above what it needs to stream from HBM -- while the kernels stay one plane = one order of additions: nothing
// about a plane's sum depends on B, the grid, or which other planes exist.  Planes of a few elements waste most of
// a block, and those tensors are a few KB.
// Order of a plane's sums (P elements, G = 16 / sizeof(T) elements per group, groups counted from the plane's first
// element): thread t owns groups t, t + 256, ...; element j of a group goes to the thread's accumulator j, in
// increasing group order; the P % G tail elements go one each to accumulator 0 of threads 0 .. P % G - 1, after the
// groups; the thread's total is ((a0 + a1) + a2) + ...; a wave folds its 64 totals with the xor butterfly 32, 16, ...,
// 1; the four wave sums are added in wave order.  A plane whose address is 16-byte aligned reads each group with one
// 16-byte load, any other plane reads the SAME groups element by element: the order depends on P and the dtype alone.
// The Makefile compiles this file with -ffp-contract=off: the two paths and the three dtypes must round alike.
#include "common.h"

namespace {

typedef _Float16 f16_t;
constexpr int BN_THREADS = 256;

__device__ __forceinline__ double to_f64(float v) { return (double)v; }
__device__ __forceinline__ double to_f64(bf16_t v) { return (double)(float)v; }
__device__ __forceinline__ double to_f64(f16_t v) { return (double)(float)v; }
// results leave as float32 (one rounding); the 16-bit dtypes round that float once more, as a float32 kernel would
template <typename T> __device__ __forceinline__ T from_f64(double v) { return (T)(float)v; }

template <typename T> struct Group {
  static constexpr int G = 16 / sizeof(T);
  union {
    uint4 raw;
    T e[16 / sizeof(T)];
  };
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the block's two sums, valid in thread 0; red: 2 * (BN_THREADS / 64) doubles of LDS
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x >> 6)] = a;
    red[2 * (threadIdx.x >> 6) + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0];
    b = red[1];
    for (int w = 1; w < BN_THREADS / 64; ++w) {
      a += red[2 * w];
      b += red[2 * w + 1];
    }
  }
}

// BWD = false: (sum x, sum x^2).  BWD = true: (sum dy, sum dy xhat), xhat = (x - mean) invstd in double.
template <typename T, bool BWD>
__global__ __launch_bounds__(BN_THREADS) void bn_partials_kernel(double* __restrict__ part, const T* __restrict__ x,
                                                                 const T* __restrict__ dy, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, int C, int64_t P) {
  constexpr int G = Group<T>::G;
  __shared__ double red[2 * (BN_THREADS / 64)];
  const int64_t plane = blockIdx.x;
  const T* __restrict__ xp = x + plane * P;
  const T* __restrict__ dp = BWD ? dy + plane * P : nullptr;
  double mu = 0.0, is = 0.0;
  if constexpr (BWD) {
    const int c = (int)(plane % C);
    mu = (double)mean[c];
    is = (double)invstd[c];
  }
  double a[G], q[G];
#pragma unroll
  for (int j = 0; j < G; ++j) a[j] = q[j] = 0.0;
  auto add = [&](int j, T xv, T dv) {
    const double xd = to_f64(xv);
    if constexpr (BWD) {
      const double dd = to_f64(dv);
      const double xh = (xd - mu) * is;
      a[j] += dd;
      q[j] += dd * xh;
    } else {
      a[j] += xd;
      q[j] += xd * xd;   // exact product of two fp32 (or narrower) values
    }
  };
  const int64_t ng = P / G;
  uintptr_t bits = reinterpret_cast<uintptr_t>(xp);
  if constexpr (BWD) bits |= reinterpret_cast<uintptr_t>(dp);
  if ((bits & 15) == 0) {
#pragma unroll 4
    for (int64_t g = threadIdx.x; g < ng; g += BN_THREADS) {
      Group<T> xv, dv;
      xv.raw = reinterpret_cast<const uint4*>(xp)[g];
      if constexpr (BWD) dv.raw = reinterpret_cast<const uint4*>(dp)[g];
      else dv.raw = xv.raw;
#pragma unroll
      for (int j = 0; j < G; ++j) add(j, xv.e[j], dv.e[j]);
    }
  } else {
    for (int64_t g = threadIdx.x; g < ng; g += BN_THREADS) {
#pragma unroll
      for (int j = 0; j < G; ++j) add(j, xp[g * G + j], BWD ? dp[g * G + j] : xp[g * G + j]);
    }
  }
  const int64_t i = ng * G + threadIdx.x;
  if (i < P) add(0, xp[i], BWD ? dp[i] : xp[i]);
  double s = a[0], s2 = q[0];
#pragma unroll
  for (int j = 1; j < G; ++j) {
    s += a[j];
    s2 += q[j];
  }
  block_sum2(s, s2, red);
  if (threadIdx.x == 0) {
    part[2 * plane] = s;
    part[2 * plane + 1] = s2;
  }
}

// Folds part[first .. first + n) [c] in index order into thread 0's (s, q).  The block loads up to BN_THREADS entries
// at a time into LDS (one latency instead of n dependent ones); thread 0 adds them one after the other.
__device__ __forceinline__ void fold_channel(double& s, double& q, const double* __restrict__ part, int first, int n, int C,
                                             int c, double* sh) {
  s = 0.0;
  q = 0.0;
  for (int base = 0; base < n; base += BN_THREADS) {
    const int m = n - base < BN_THREADS ? n - base : BN_THREADS;
    if ((int)threadIdx.x < m) {
      const int64_t o = 2 * ((int64_t)(first + base + (int)threadIdx.x) * C + c);
      sh[2 * threadIdx.x] = part[o];
      sh[2 * threadIdx.x + 1] = part[o + 1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 0; k < m; ++k) {
        s += sh[2 * k];
        q += sh[2 * k + 1];
      }
    }
    __syncthreads();
  }
}

// v(x element, dy element) -> output element, over the block's plane: 16-byte loads and stores where all planes are
// 16-byte aligned, element by element otherwise and for the tail; the results do not depend on the path.
template <typename T, bool TWO, typename F>
__device__ __forceinline__ void map_plane(T* __restrict__ op, const T* __restrict__ xp, const T* __restrict__ dp, int64_t P, F f) {
  constexpr int G = Group<T>::G;
  uintptr_t bits = reinterpret_cast<uintptr_t>(op) | reinterpret_cast<uintptr_t>(xp);
  if constexpr (TWO) bits |= reinterpret_cast<uintptr_t>(dp);
  int64_t done = 0;
  if ((bits & 15) == 0) {
    const int64_t ng = P / G;
#pragma unroll 4
    for (int64_t g = threadIdx.x; g < ng; g += BN_THREADS) {
      Group<T> xv, dv, ov;
      xv.raw = reinterpret_cast<const uint4*>(xp)[g];
      if constexpr (TWO) dv.raw = reinterpret_cast<const uint4*>(dp)[g];
      else dv.raw = xv.raw;
#pragma unroll
      for (int j = 0; j < G; ++j) ov.e[j] = f(xv.e[j], dv.e[j]);
      reinterpret_cast<uint4*>(op)[g] = ov.raw;
    }
    done = ng * G;
  }
  for (int64_t i = done + threadIdx.x; i < P; i += BN_THREADS) op[i] = f(xp[i], TWO ? dp[i] : xp[i]);
}

template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(T* __restrict__ y, float* __restrict__ save_mean,
                                                              float* __restrict__ save_invstd, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var, int64_t* __restrict__ nbt,
                                                              const T* __restrict__ x, const double* __restrict__ part,
                                                              const float* __restrict__ weight, const float* __restrict__ bias,
                                                              int Btot, int C, int64_t P, float eps, float momentum) {
  __shared__ double sh[2 * BN_THREADS];
  __shared__ double stat[2];
  const int64_t plane = blockIdx.x;
  const int c = (int)(plane % C);
  double s, q;
  fold_channel(s, q, part, 0, Btot, C, c, sh);
  if (threadIdx.x == 0) {
    const double n = (double)Btot * (double)P;
    const double mean = s / n;
    double var = q / n - mean * mean;
    if (var < 0.0) var = 0.0;   // (a NaN stays a NaN)
    const double invstd = 1.0 / sqrt(var + (double)eps);
    stat[0] = mean;
    stat[1] = invstd;
    if (plane < C) {   // sample 0's block of the channel is the designated one
      save_mean[c] = (float)mean;
      save_invstd[c] = (float)invstd;
      if (running_mean) {
        // momentum < 0: the cumulative average, whose factor is 1 / num_batches_tracked AFTER this batch was counted --
        // the caller counts it before the launch in that mode (blocks of other channels read the word)
        const double f = momentum >= 0.f ? (double)momentum : 1.0 / (double)nbt[0];
        running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * mean);
        running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * (var * (n / (n - 1.0))));
      }
      if (plane == 0 && nbt && momentum >= 0.f) nbt[0] += 1;
    }
  }
  __syncthreads();
  const double mean = stat[0];
  const double scale = stat[1] * (weight ? (double)weight[c] : 1.0);
  const double shift = bias ? (double)bias[c] : 0.0;
  map_plane<T, false>(y + plane * P, x + plane * P, static_cast<const T*>(nullptr), P,
                      [&](T xv, T) { return from_f64<T>((to_f64(xv) - mean) * scale + shift); });
}

template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(T* __restrict__ dx, float* __restrict__ dweight,
                                                                  float* __restrict__ dbias, const T* __restrict__ dy,
                                                                  const T* __restrict__ x, const double* __restrict__ part,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                  const float* __restrict__ weight, int B, int Btot, int b_off,
                                                                  int C, int64_t P) {
  __shared__ double sh[2 * BN_THREADS];
  __shared__ double stat[2];
  const int64_t plane = blockIdx.x;
  const int c = (int)(plane % C);
  double s, q;
  fold_channel(s, q, part, 0, Btot, C, c, sh);
  if (threadIdx.x == 0) {
    const double n = (double)Btot * (double)P;
    stat[0] = s / n;
    stat[1] = q / n;
  }
  if (plane < C && (dweight || dbias)) {   // the local samples' sums, folded on their own in index order
    fold_channel(s, q, part, b_off, B, C, c, sh);
    if (threadIdx.x == 0) {
      if (dbias) dbias[c] = (float)s;
      if (dweight) dweight[c] = (float)q;
    }
  }
  __syncthreads();
  const double m1 = stat[0], m2 = stat[1];
  const double mu = (double)mean[c], is = (double)invstd[c];
  const double k = is * (weight ? (double)weight[c] : 1.0);
  map_plane<T, true>(dx + plane * P, x + plane * P, dy + plane * P, P, [&](T xv, T dv) {
    const double xh = (to_f64(xv) - mu) * is;
    return from_f64<T>(k * ((to_f64(dv) - m1) - xh * m2));
  });
}

bool geometry_ok(int B, int C, int H, int W) {
  return B >= 1 && C >= 1 && H >= 1 && W >= 1 && (int64_t)B * C <= 2147483647LL && (int64_t)H * W <= 2147483647LL;
}

bool dtype_ok(int dtype) { return dtype == DGV2_F32 || dtype == DGV2_BF16 || dtype == DGV2_F16; }

}  // namespace

#define BN_DISPATCH(dtype, ...)              \
  do {                                       \
    if ((dtype) == DGV2_F32) {               \
      typedef float T;                       \
      __VA_ARGS__;                           \
    } else if ((dtype) == DGV2_BF16) {       \
      typedef bf16_t T;                      \
      __VA_ARGS__;                           \
    } else {                                 \
      typedef f16_t T;                       \
      __VA_ARGS__;                           \
    }                                        \
  } while (0)

extern "C" int dgv2_bn_partials(double* part, const void* x, int B, int C, int H, int W, int dtype, void* stream) {
  if (!part || !x || !geometry_ok(B, C, H, W) || !dtype_ok(dtype)) return DGV2_EINVAL;
  const int64_t P = (int64_t)H * W;
  BN_DISPATCH(dtype, (bn_partials_kernel<T, false><<<B * C, BN_THREADS, 0, (hipStream_t)stream>>>(
                         part, (const T*)x, (const T*)nullptr, nullptr, nullptr, C, P)));
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_bn_apply(void* y, float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, const void* x, const double* part, const float* weight,
                             const float* bias, int B, int Btot, int C, int H, int W, float eps, float momentum, int dtype,
                             void* stream) {
  if (!y || !save_mean || !save_invstd || !x || !part || !geometry_ok(B, C, H, W) || !dtype_ok(dtype)) return DGV2_EINVAL;
  if (Btot < B || (int64_t)Btot * C > 2147483647LL || (int64_t)Btot * H * W < 2) return DGV2_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return DGV2_EINVAL;
  if (!(eps >= 0.f) || momentum != momentum) return DGV2_EINVAL;
  if (momentum < 0.f && running_mean && !num_batches_tracked) return DGV2_EINVAL;
  const int64_t P = (int64_t)H * W;
  BN_DISPATCH(dtype, (bn_apply_kernel<T><<<B * C, BN_THREADS, 0, (hipStream_t)stream>>>(
                         (T*)y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, (const T*)x, part,
                         weight, bias, Btot, C, P, eps, momentum)));
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_bn_bwd_partials(double* part, const void* dy, const void* x, const float* mean, const float* invstd,
                                    int B, int C, int H, int W, int dtype, void* stream) {
  if (!part || !dy || !x || !mean || !invstd || !geometry_ok(B, C, H, W) || !dtype_ok(dtype)) return DGV2_EINVAL;
  const int64_t P = (int64_t)H * W;
  BN_DISPATCH(dtype, (bn_partials_kernel<T, true><<<B * C, BN_THREADS, 0, (hipStream_t)stream>>>(
                         part, (const T*)x, (const T*)dy, mean, invstd, C, P)));
  DGV2_RETURN_LAST();
}

extern "C" int dgv2_bn_bwd_apply(void* dx, float* dweight, float* dbias, const void* dy, const void* x, const double* part,
                                 const float* mean, const float* invstd, const float* weight, int B, int Btot, int b_off,
                                 int C, int H, int W, int dtype, void* stream) {
  if (!dx || !dy || !x || !part || !mean || !invstd || !geometry_ok(B, C, H, W) || !dtype_ok(dtype)) return DGV2_EINVAL;
  if (b_off < 0 || (int64_t)b_off + B > Btot || (int64_t)Btot * C > 2147483647LL || (int64_t)Btot * H * W < 2)
    return DGV2_EINVAL;
  const int64_t P = (int64_t)H * W;
  BN_DISPATCH(dtype, (bn_bwd_apply_kernel<T><<<B * C, BN_THREADS, 0, (hipStream_t)stream>>>(
                         (T*)dx, dweight, dbias, (const T*)dy, (const T*)x, part, mean, invstd, weight, B, Btot, b_off, C, P)));
  DGV2_RETURN_LAST();
}
