// Confusion counts of a segmentation evaluation (reference: the per-class tp / fp / fn loop of test_semseg.py:23-42
// over preds * mask, label * mask of its lines 136-137; include/dgv2.h states the contract).  One launch.
//
// A block counts its share of the pixels into an LDS histogram of (C+1)^2 bins with integer atomics and then adds the
// non-empty bins into `conf` with 64-bit integer atomics: integer sums do not depend on the order, so the counts are
// bit-identical from run to run.  With few classes every lane of a wave hits the same handful of bins, so the LDS
// histogram is kept in R copies (R a power of two, as many as fit 16 KiB, at most one per lane) selected by the lane
// and interleaved bin-major; the copies are summed when the block flushes.
#include "common.h"

namespace {

// Every block ends with one 64-bit atomic per non-empty bin on the same (C+1)^2 words, which serialise at the memory
// side: two blocks per CU keep the loads in flight without queueing thousands of atomics on a handful of addresses
// (1 M pixels, C = 4: 38.3 us with up to 2048 blocks, 12.6 us with 512).
constexpr int NT = 256, C_MAX = 32, LDS_WORDS = 4096, MAX_BLOCKS = 512;

__device__ __forceinline__ int bin_of(int64_t v, int C) { return (v >= 0 && v < C) ? (int)v : C; }

__global__ __launch_bounds__(NT) void seg_confusion_kernel(unsigned long long* __restrict__ conf,
                                                           const int64_t* __restrict__ label,
                                                           const int64_t* __restrict__ pred,
                                                           const float* __restrict__ mask, int64_t n, int C, int copies,
                                                           int pairs_ok) {
  __shared__ unsigned hist[LDS_WORDS];
  const int bins = (C + 1) * (C + 1), mine = threadIdx.x & (copies - 1);
  for (int i = threadIdx.x; i < bins * copies; i += NT) hist[i] = 0u;
  __syncthreads();

  auto count = [&](int64_t l, int64_t p, bool keep) {
    const int row = keep ? bin_of(l, C) : 0, col = keep ? bin_of(p, C) : 0;
    atomicAdd(&hist[(row * (C + 1) + col) * copies + mine], 1u);
  };
  const int64_t stride = (int64_t)gridDim.x * NT, first = (int64_t)blockIdx.x * NT + threadIdx.x;
  // 16-byte loads of two labels / two predictions where the pointers allow it; the odd last element goes below
  const int64_t n_pairs = pairs_ok ? n / 2 : 0;
#pragma unroll 4
  for (int64_t i = first; i < n_pairs; i += stride) {
    const longlong2 l = reinterpret_cast<const longlong2*>(label)[i], p = reinterpret_cast<const longlong2*>(pred)[i];
    float2 m = make_float2(1.f, 1.f);
    if (mask) m = reinterpret_cast<const float2*>(mask)[i];
    count(l.x, p.x, m.x != 0.f);
    count(l.y, p.y, m.y != 0.f);
  }
  for (int64_t i = 2 * n_pairs + first; i < n; i += stride) count(label[i], pred[i], mask ? mask[i] != 0.f : true);
  __syncthreads();

  for (int bin = threadIdx.x; bin < bins; bin += NT) {
    unsigned long long s = 0;
    for (int r = 0; r < copies; ++r) s += hist[bin * copies + r];
    if (s) atomicAdd(&conf[bin], s);
  }
}

}  // namespace

extern "C" int dgv2_seg_confusion(int64_t* conf, const int64_t* label, const int64_t* pred, const float* mask,
                                  int64_t n, int num_classes, void* stream) {
  if (!conf || !label || !pred || n < 1 || n >= (1LL << 40) || num_classes < 1 || num_classes > C_MAX)
    return DGV2_EINVAL;
  const int bins = (num_classes + 1) * (num_classes + 1);
  int copies = 1;
  while (copies < 64 && 2 * copies * bins <= LDS_WORDS) copies *= 2;
  const int pairs_ok = aligned16(label) && aligned16(pred) && (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
  // a block counts at most n / MAX_BLOCKS + NT < 2^32 pixels: the 32-bit LDS counters cannot wrap
  const int grid = grid_for((n + 1) / 2, NT, MAX_BLOCKS);
  seg_confusion_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(reinterpret_cast<unsigned long long*>(conf), label, pred,
                                                            mask, n, num_classes, copies, pairs_ok);
  DGV2_RETURN_LAST();
}
