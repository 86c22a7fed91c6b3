// Latent fitting (reference: gans/inversion.py:10-20,81-90, demo_inversion.py:147-152): everything a stage-1 inversion
// step does after backward() -- the geocross term of the "w+" styles and its gradient, the total loss, the learning-rate
// schedule, Adam on the latent and the sensor phase, the hypersphere projection, the step counter -- in ONE launch.
//
// The reference spends about 50 launches on these few KB (geocross_loss and its autograd, torch.optim.Adam, LambdaLR's
// Python float, a host-side append of the loss), and the Python float keeps the step out of a hipGraph.  Here every
// scalar of the step is derived from a device-resident counter, one per sample.
//
// One block per sample, no atomics, no workspace, no dependence between samples: a sample's bits depend neither on B
// nor on its place in the batch.  The sample's z [N,D] is read once into LDS.  Reductions follow inversion.hip: strided
// partial per lane, xor shuffle, wave partials added in order.
#include "common.h"

namespace {

constexpr int LAT_THREADS = 512;
constexpr int LAT_WAVES = LAT_THREADS / 64;
constexpr int LAT_JC = 64;           // styles whose pair coefficients are staged at a time
constexpr int LAT_MAX_ND = 16384;    // floats of one sample's z held in LDS

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

// the scalar factors of one step, in double (torch.optim.Adam's Python floats), rounded once for the element-wise part
struct AdamScalars {
  float one_minus_b1, b2, one_minus_b2, step_size, bias2_sqrt, eps;
};

// torch.optim.Adam (no weight decay, no amsgrad), operation by operation in float32:
//   m.lerp_(g, 1 - b1);  v.mul_(b2).addcmul_(g, g, value = 1 - b2);  denom = v.sqrt() / sqrt(1 - b2^t) + eps;
//   p.addcdiv_(m, denom, value = -lr / (1 - b1^t))
__device__ __forceinline__ float adam_elem(float p, float g, float* __restrict__ m, float* __restrict__ v,
                                           const AdamScalars& s) {
  const float mn = *m + s.one_minus_b1 * (g - *m);
  const float vn = *v * s.b2 + s.one_minus_b2 * (g * g);
  *m = mn;
  *v = vn;
  const float denom = sqrtf(vn) / s.bias2_sqrt + s.eps;
  return p - s.step_size * (mn / denom);
}

__global__ __launch_bounds__(LAT_THREADS) void latent_step_kernel(
    float* __restrict__ z, float* __restrict__ g_z, float* __restrict__ m_z, float* __restrict__ v_z,
    float* __restrict__ phase, const float* __restrict__ g_phase, float* __restrict__ m_p, float* __restrict__ v_p,
    int* __restrict__ step, const float* __restrict__ loss_terms, float* __restrict__ loss_log, float* __restrict__ geo,
    int B, int N, int D, int num_steps, float lr0, float rampup, float rampdown, float beta1, float beta2, float eps,
    float geo_coef, int hypersphere) {
  extern __shared__ float lat_lds[];   // xs [N*D]: the sample's z as it came in;  row [D]: a style row in flight
  __shared__ float red[16];
  __shared__ float wa[LAT_JC], wb[LAT_JC], th3[LAT_JC];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = step[b];
  if (k < 0 || k >= num_steps) return;   // a finished sample: an over-replayed graph changes nothing (block-uniform)

  float* xs = lat_lds;
  float* row = lat_lds + N * D;
  const int64_t base = (int64_t)b * N * D;
  for (int p = tid; p < N * D; p += LAT_THREADS) xs[p] = z[base + p];

  // schedule and bias corrections, in double
  AdamScalars s;
  {
    const double t = (double)k / (double)num_steps;
    double gamma = fmin(1.0, (1.0 - t) / (double)rampdown);
    gamma = 0.5 - 0.5 * cos(gamma * 3.141592653589793);
    gamma = gamma * (rampup > 0.f ? fmin(1.0, t / (double)rampup) : 1.0);
    const double lr = (double)lr0 * gamma;
    const double bias1 = 1.0 - pow((double)beta1, (double)(k + 1));
    const double bias2 = 1.0 - pow((double)beta2, (double)(k + 1));
    s.one_minus_b1 = (float)(1.0 - (double)beta1);
    s.b2 = beta2;
    s.one_minus_b2 = (float)(1.0 - (double)beta2);
    s.step_size = (float)(lr / bias1);
    s.bias2_sqrt = (float)sqrt(bias2);
    s.eps = eps;
  }
  if (phase && tid < 2) {
    const int q = b * 2 + tid;
    phase[q] = adam_elem(phase[q], g_phase[q], m_p + q, v_p + q, s);
  }
  __syncthreads();   // xs is complete

  const bool geo_on = geo_coef != 0.f;
  // d/dx_i of geo_coef * mean_ij theta_ij^3 = geo_coef * (2 / N^2) * sum_j [wa_ij (x_i - x_j) - wb_ij (x_i + x_j)]
  const float gscale = (float)((double)geo_coef * 2.0 / ((double)N * (double)N));
  double geo_sum = 0.0;   // thread 0: theta^3 over the ordered pairs, row by row, j ascending

  for (int i = 0; i < N; ++i) {
    const float* xi = xs + i * D;
    if (geo_on) {
      for (int j0 = 0; j0 < N; j0 += LAT_JC) {
        const int jn = min(LAT_JC, N - j0);
        for (int jj = wave; jj < jn; jj += LAT_WAVES) {   // wave-uniform
          const float* xj = xs + (j0 + jj) * D;
          float sd = 0.f, ss = 0.f;
          for (int d = lane; d < D; d += 64) {
            const float a = xi[d] - xj[d], c = xi[d] + xj[d];   // from the differences: exactly 0 for equal styles
            sd += a * a;
            ss += c * c;
          }
          sd = wave_sum(sd);
          ss = wave_sum(ss);
          if (lane == 0) {
            const float A2 = sd + 1e-9f, B2 = ss + 1e-9f;
            const float A = sqrtf(A2), Bq = sqrtf(B2);
            const float th = atan2f(A, Bq);
            const float den = A * A + Bq * Bq;
            const float t2 = 3.f * (th * th);
            wa[jj] = t2 * (Bq / (den * A));
            wb[jj] = t2 * (A / (den * Bq));
            th3[jj] = (th * th) * th;
          }
        }
        __syncthreads();
        if (tid == 0)
          for (int jj = 0; jj < jn; ++jj) geo_sum += (double)th3[jj];
        for (int d = tid; d < D; d += LAT_THREADS) {
          float acc = j0 == 0 ? 0.f : row[d];
          const float x = xi[d];
          for (int jj = 0; jj < jn; ++jj) {
            const float y = xs[(j0 + jj) * D + d];
            acc += wa[jj] * (x - y) - wb[jj] * (x + y);
          }
          row[d] = acc;
        }
        __syncthreads();   // the coefficients are overwritten by the next chunk / row
      }
    }
    float sq = 0.f;
    for (int d = tid; d < D; d += LAT_THREADS) {
      const int64_t idx = base + (int64_t)i * D + d;
      float g = g_z[idx];
      if (geo_on) {
        g += gscale * row[d];
        g_z[idx] = g;
      }
      const float pn = adam_elem(xi[d], g, m_z + idx, v_z + idx, s);
      if (hypersphere) {
        row[d] = pn;
        sq += pn * pn;
      } else {
        z[idx] = pn;
      }
    }
    if (hypersphere) {   // SphericalOptimizer: row / sqrt(mean(row^2) + 1e-9)
      const float tot = block_sum_all(sq, red);
      const float r = sqrtf(tot / (float)D + 1e-9f);
      for (int d = tid; d < D; d += LAT_THREADS) z[base + (int64_t)i * D + d] = row[d] / r;
    }
  }

  if (tid == 0) {
    const float gv = geo_on ? (float)(geo_sum / ((double)N * (double)N)) : 0.f;
    geo[b] = gv;
    loss_log[(int64_t)k * B + b] = loss_terms[b] + geo_coef * gv;
    step[b] = k + 1;
  }
}

}  // namespace

extern "C" int dgv2_latent_step(float* z, float* g_z, float* m_z, float* v_z, float* phase, const float* g_phase,
                                float* m_p, float* v_p, int* step, const float* loss_terms, float* loss_log, float* geo,
                                int B, int N, int D, int num_steps, float lr0, float rampup_ratio, float rampdown_ratio,
                                float beta1, float beta2, float eps, float geo_coef, int hypersphere, void* stream) {
  if (!z || !g_z || !m_z || !v_z || !step || !loss_terms || !loss_log || !geo) return DGV2_EINVAL;
  if (B < 1 || N < 1 || D < 1 || num_steps < 1) return DGV2_EINVAL;
  if ((int64_t)N * D > LAT_MAX_ND) return DGV2_EINVAL;
  if (geo_coef != 0.f && N < 2) return DGV2_EINVAL;
  const int nphase = (phase != nullptr) + (g_phase != nullptr) + (m_p != nullptr) + (v_p != nullptr);
  if (nphase != 0 && nphase != 4) return DGV2_EINVAL;
  const bool needs_row = geo_coef != 0.f || hypersphere;
  const size_t lds = ((size_t)N * D + (needs_row ? (size_t)D : 0)) * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)latent_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)hipErrorUnknown;
  }
  latent_step_kernel<<<B, LAT_THREADS, lds, (hipStream_t)stream>>>(z, g_z, m_z, v_z, phase, g_phase, m_p, v_p, step,
                                                                  loss_terms, loss_log, geo, B, N, D, num_steps, lr0,
                                                                  rampup_ratio, rampdown_ratio, beta1, beta2, eps,
                                                                  geo_coef, hypersphere);
  DGV2_RETURN_LAST();
}
