// kNN label filter of the range-image segmentation models (reference: semseg/models/knn.py:38-76, the RangeNet++
// filter; the formulas are in include/dgv2.h).  fp32 distances, int64 labels, plain HIP, one launch.
//
//  * A block owns a TH x TW pixel tile of one sample, one pixel per thread.  It stages the raw depth of the tile with
//    a halo of (2 ph, 2 pw) (0 outside the image: unfold's padding) and the labels with a halo of (ph, pw) (0 outside
//    the image, -1 for a label outside [0, num_classes)) in LDS; everything else is computed from there: no [B,K,HW]
//    tensor exists.
//  * dist_k(p) = sum_j w_j |nb(p + o_j + o_k) - depth(p + o_j)| reads only the (2kh-1) x (2kw-1) depth window around
//    p.  A thread loads that window into registers once (negative -> +inf applied on the way) and keeps its K = kh kw
//    distances in registers; the kernel is templated over (kh, kw), every loop is unrolled and every register array is
//    indexed statically.  An anchor p + o_j outside the image contributes nothing (the conv's zero padding): a branch,
//    not a zero weight, because 0 * inf is NaN.
//  * Selection is a rank: rank_i = #{j : d_j < d_i, or d_j == d_i and j < i}; slot i is among the k nearest iff
//    rank_i < k.  That is the tie rule of the header (lower slot first), costs K (K-1) / 2 comparisons whatever k is,
//    and needs no sort.
//  * The vote needs no bins: the voters are counted label by label, lowest label first (a round takes the smallest
//    label still uncounted, counts and retires its voters), and the winner is the first label with the highest count.
//    At most k rounds, in practice one or two: neighbours mostly agree.  num_classes is unbounded.
//  * The kernel is bound by vector-instruction issue (K^2 taps, then K (K-1) / 2 comparisons with two carry-adds
//    each), not by memory: 20 bytes per pixel move.
#include "common.h"

#include <math.h>

namespace {

constexpr int KMAX = 5, TH = 8, TW = 32, NT = TH * TW;

struct Geo {
  int H, W, tiles_h, tiles_w, k, num_classes;
  float cutoff;
};

template <int KH, int KW>
__global__ __launch_bounds__(NT) void knn2d_kernel(int64_t* __restrict__ out, const float* __restrict__ depth,
                                                   const int64_t* __restrict__ label,
                                                   const float* __restrict__ dist_kernel, Geo g) {
  constexpr int PH = KH / 2, PW = KW / 2, K = KH * KW;
  constexpr int DH = TH + 4 * PH, DW = TW + 4 * PW;   // staged depth
  constexpr int LH = TH + 2 * PH, LW = TW + 2 * PW;   // staged labels
  constexpr int WH = 2 * KH - 1, WW = 2 * KW - 1;     // a pixel's depth window
  __shared__ float sd[DH * DW];
  __shared__ int sl[LH * LW];

  const int tiles = g.tiles_h * g.tiles_w, tile = blockIdx.x % tiles;
  const int64_t b = blockIdx.x / tiles, HW = (int64_t)g.H * g.W;
  const int h0 = (tile / g.tiles_w) * TH, w0 = (tile % g.tiles_w) * TW;
  const float* db = depth + b * HW;
  const int64_t* lb = label + b * HW;
  for (int idx = threadIdx.x; idx < DH * DW; idx += NT) {
    const int h = h0 - 2 * PH + idx / DW, w = w0 - 2 * PW + idx % DW;
    sd[idx] = (h >= 0 && h < g.H && w >= 0 && w < g.W) ? db[(int64_t)h * g.W + w] : 0.f;
  }
  for (int idx = threadIdx.x; idx < LH * LW; idx += NT) {
    const int h = h0 - PH + idx / LW, w = w0 - PW + idx % LW;
    int v = 0;
    if (h >= 0 && h < g.H && w >= 0 && w < g.W) {
      const int64_t l = lb[(int64_t)h * g.W + w];
      v = (l >= 0 && l < g.num_classes) ? (int)l : -1;
    }
    sl[idx] = v;
  }
  float wgt[K];
#pragma unroll
  for (int j = 0; j < K; ++j) wgt[j] = dist_kernel[j];   // uniform: scalar loads
  __syncthreads();

  const int r = threadIdx.x / TW, c = threadIdx.x % TW, h = h0 + r, w = w0 + c;
  if (h >= g.H || w >= g.W) return;

  // the window around the pixel, as the neighbour sees it: negative -> +inf
  float nb[WH][WW];
#pragma unroll
  for (int y = 0; y < WH; ++y)
#pragma unroll
    for (int x = 0; x < WW; ++x) {
      const float v = sd[(r + y) * DW + c + x];
      nb[y][x] = v < 0.f ? INFINITY : v;
    }

  float dist[K];
#pragma unroll
  for (int k = 0; k < K; ++k) dist[k] = 0.f;
#pragma unroll
  for (int jy = 0; jy < KH; ++jy)
#pragma unroll
    for (int jx = 0; jx < KW; ++jx) {
      const int qh = h + jy - PH, qw = w + jx - PW;
      if (qh >= 0 && qh < g.H && qw >= 0 && qw < g.W) {
        const float anchor = sd[(r + jy + PH) * DW + c + jx + PW];   // raw
        const float wj = wgt[jy * KW + jx];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky)
#pragma unroll
          for (int kx = 0; kx < KW; ++kx)
            dist[ky * KW + kx] = fmaf(wj, fabsf(nb[jy + ky][jx + kx] - anchor), dist[ky * KW + kx]);
      }
    }

  // rank_i = #{j > i : d_j < d_i} + #{j < i : d_j <= d_i} = ahead[i] + i - behind[i]: one comparison and two
  // carry-adds per pair
  int ahead[K], behind[K];
#pragma unroll
  for (int i = 0; i < K; ++i) ahead[i] = behind[i] = 0;
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = i + 1; j < K; ++j) {
      const int j_first = dist[j] < dist[i] ? 1 : 0;   // a tie: the lower slot i comes first
      ahead[i] += j_first;
      behind[j] += j_first;
    }

  // the label a slot votes for, or NONE: not selected, beyond the cutoff, or a label outside [0, num_classes)
  constexpr int NONE = 0x7fffffff;   // above every label: l < num_classes <= INT_MAX
  const float cut = g.cutoff > 0.f ? g.cutoff : INFINITY;
  int vote[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int l = sl[(r + i / KW) * LW + c + i % KW];
    const bool in = ahead[i] + i - behind[i] < g.k && !(dist[i] > cut) && l >= 0;
    vote[i] = in ? l : NONE;
  }
  // count the voters label by label, lowest label first: one round per distinct label among at most k voters
  int best_count = 0, best = 0;   // no votes: class 0, as argmax over all-zero bins
  while (true) {
    int lowest = vote[0];
#pragma unroll
    for (int i = 1; i < K; ++i) lowest = min(lowest, vote[i]);
    if (lowest == NONE) break;
    int n = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const bool hit = vote[i] == lowest;
      n += hit ? 1 : 0;
      vote[i] = hit ? NONE : vote[i];
    }
    if (n > best_count) {   // labels come in ascending order: a tie stays with the lower one
      best_count = n;
      best = lowest;
    }
  }
  out[b * HW + (int64_t)h * g.W + w] = best;
}

#define KNN_CASE(KH_, KW_)                                                                         \
  if (kh == KH_ && kw == KW_) {                                                                    \
    knn2d_kernel<KH_, KW_><<<(unsigned)blocks, NT, 0, st>>>(out, depth, label, dist_kernel, g);   \
    DGV2_RETURN_LAST();                                                                            \
  }

}  // namespace

extern "C" int dgv2_knn2d(int64_t* out, const float* depth, const int64_t* label, const float* dist_kernel, int B,
                          int H, int W, int kh, int kw, int k, int num_classes, float cutoff, void* stream) {
  if (!out || !depth || !label || !dist_kernel || B <= 0 || H <= 0 || W <= 0 || num_classes < 1) return DGV2_EINVAL;
  if (kh < 1 || kw < 1 || kh > KMAX || kw > KMAX || kh % 2 == 0 || kw % 2 == 0) return DGV2_EINVAL;
  if (kh * kw == 1 || k < 1 || k > kh * kw || cutoff != cutoff) return DGV2_EINVAL;   // 1 x 1: w = 0, 0 * inf
  if ((int64_t)H * W >= (1LL << 31)) return DGV2_EINVAL;
  Geo g{H, W, (H + TH - 1) / TH, (W + TW - 1) / TW, k, num_classes, cutoff};
  const int64_t blocks = (int64_t)B * g.tiles_h * g.tiles_w;
  if (blocks >= (1LL << 31)) return DGV2_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  KNN_CASE(1, 3) KNN_CASE(1, 5) KNN_CASE(3, 1) KNN_CASE(3, 3) KNN_CASE(3, 5) KNN_CASE(5, 1) KNN_CASE(5, 3) KNN_CASE(5, 5)
  return DGV2_EINVAL;
}
