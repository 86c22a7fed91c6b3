// One PointNet trunk of the FPD / KPD feature extractor -- the per-point 3 -> 64 -> 128 -> 1024 chain and the max over
// the points of a cloud -- without a per-point activation in memory (include/dgv2.h, "PointNet trunk", states the
// arithmetic; DESIGN.md section 40 the structure and the measurements).  gfx950 only.
//
// A block of four waves owns one tile of P = 128 points of one cloud and carries it through the three layers:
//   1  VALU.  Thread t takes point t & 127 and 32 of the 64 channels (waves 0-1 the first half, waves 2-3 the second, so
//      W1 / b1 are read at wave-uniform addresses): q = pts . trans, h1 = relu(W1 q + b1), written to the LDS image
//      h1[P][68] with 16-byte stores.  A lane beyond the cloud's last point reads that last point again: a duplicate
//      cannot change a maximum, so ragged tiles need no mask and no padding value exists that could enter the max.
//   2  v_mfma_f32_32x32x2_f32, points on the rows, channels on the columns.  Wave w owns channels [32w, 32w + 32) for
//      all four 32-point row blocks: its W2 fragment (32 floats a lane, 16-byte global loads) stays in registers, the A
//      operands are 16-byte LDS reads of h1.  All 64 accumulators of a lane are complete before the barrier after which
//      h2 = relu(acc + b2) overwrites the same LDS bytes as the image h2[P][132].
//   3  the same product shape with K = 128.  Wave w owns channels [256w, 256w + 256) as eight column blocks; per block
//      its W3 fragment (64 floats a lane, 16 x 16-byte loads from the L2-resident 512 KB matrix) is held in registers
//      for all four row blocks, the next block's fragment is loaded while this one multiplies, and the only operand
//      traffic per four MFMAs is one 16-byte LDS read.  The lane's 64 results (64 points of one channel) fold into one
//      maximum, lanes l and l ^ 32 combine, and 32 lanes own the block's 32 channel maxima.
// Both LDS images have a row pitch of 4 (mod 64) floats: the 16 lanes of a ds_read_b128 group read 16 different 16-byte
// slots of the 256-byte bank row, and the 4-byte h2 stores of a half-wave go to 32 consecutive banks.
//
// k order.  MFMA number t of k-group g multiplies k = 8g + t on lanes 0-31 and k = 8g + 4 + t on lanes 32-63 (a lane's
// 16-byte read is four consecutive k), so every output is the ONE fmaf chain
//   k = 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, ...          (v_mfma_f32_32x32x2_f32 is an exact k-ordered fmaf chain)
// from 0, whatever lane, row block, tile or cloud the point sits in; the bias is added after the chain.
//
// Several blocks share a cloud when N > P.  Bias and ReLU are monotone, so each block applies them to its own maxima
// and combines the results in feat itself with integer atomics on the float's bits (signed max for a clear sign bit,
// unsigned min for a set one: together the total order of the non-NaN floats, -0 < +0); a fill launch sets feat to -inf
// first.  A maximum does not depend on the order of its operands, so the bits do not depend on the arrival order.  No
// workspace.  N <= P: one block per cloud stores its maxima, one launch.
#include <math.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int PN_P = DGV2_POINTNET_TILE;   // points per block
constexpr int PN_THREADS = 256;
constexpr int PN_C1 = 64, PN_C2 = 128, PN_C3 = DGV2_POINTNET_FEATURES;
constexpr int PN_RB = PN_P / 32;           // 32-point row blocks of a tile
constexpr int PN_H1P = PN_C1 + 4;          // LDS row pitches in floats: 4 (mod 64)
constexpr int PN_H2P = PN_C2 + 4;
constexpr int PN_LDS = PN_P * PN_H2P * (int)sizeof(float);   // 67 584 bytes: two blocks on a compute unit
static_assert(PN_P == 128 && PN_THREADS == 2 * PN_P, "layer 1 maps one point and half the channels to a thread");
static_assert(PN_P * PN_H1P <= PN_P * PN_H2P, "the h1 image lives in the h2 image's bytes");

struct PnP {
  float* feat;
  const float *pts, *trans, *w1, *b1, *w2, *b2, *w3, *b3;
  int N, tiles, relu_last, direct;
};

// The 32 x 32 product of one 32-point row block (K = 8 * G floats a row at `a`) with the lane's fragment bw, as one
// accumulator chain from 0.  One chain at a time: the MFMA's issue interval equals its dependent-accumulator latency
// (64 cycles), so a single chain keeps the matrix core busy and only one row block's A reads are in flight.
template <int G>
__device__ __forceinline__ f32x16 pn_mfma_block(const float* a, const f32x4 (&bw)[G]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + 8 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bw[g][t], acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(PN_THREADS, 2) void pointnet_trunk_kernel(const PnP p) {
  extern __shared__ __attribute__((aligned(16))) float pn_tile[];   // h1[P][PN_H1P], then h2[P][PN_H2P]

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int b = blockIdx.x / p.tiles, tl = blockIdx.x - b * p.tiles;
  const int p0 = tl * PN_P;
  const int npts = p.N - p0 < PN_P ? p.N - p0 : PN_P;   // >= 1: tiles = ceil(N / P)

  // ---- layer 1 ---------------------------------------------------------------------------------------------------------
  {
    const int pi = t & (PN_P - 1), half = wave >> 1;
    const int src = p0 + (pi < npts ? pi : npts - 1);
    const float* const pp = p.pts + ((int64_t)b * p.N + src) * 3;
    const float x = pp[0], y = pp[1], z = pp[2];
    float q[3] = {x, y, z};
    if (p.trans) {
      const float* const T = p.trans + (int64_t)b * 9;
#pragma unroll
      for (int j = 0; j < 3; ++j) q[j] = fmaf(z, T[6 + j], fmaf(y, T[3 + j], x * T[j]));
    }
    const float* const w = p.w1 + half * 32 * 3;
    const float* const bs = p.b1 + half * 32;
    float* const dst = pn_tile + pi * PN_H1P + half * 32;
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
      f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* const wc = w + (c + u) * 3;
        const float s = fmaf(wc[2], q[2], fmaf(wc[1], q[1], wc[0] * q[0]));
        v[u] = fmaxf(s + bs[c + u], 0.f);
      }
      *reinterpret_cast<f32x4*>(dst + c) = v;
    }
  }
  __syncthreads();

  // ---- layer 2 ---------------------------------------------------------------------------------------------------------
  {
    const int col = wave * 32 + lr;
    f32x4 bw[PN_C1 / 8];
#pragma unroll
    for (int g = 0; g < PN_C1 / 8; ++g) bw[g] = *reinterpret_cast<const f32x4*>(p.w2 + col * PN_C1 + 8 * g + 4 * lh);
    const float bias = p.b2[col];
    f32x16 acc[PN_RB];
#pragma unroll
    for (int rb = 0; rb < PN_RB; ++rb) acc[rb] = pn_mfma_block<PN_C1 / 8>(pn_tile + (rb * 32 + lr) * PN_H1P + 4 * lh, bw);
    __syncthreads();   // every wave has read the h1 image: its bytes become the h2 image
#pragma unroll
    for (int rb = 0; rb < PN_RB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rb * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
        pn_tile[row * PN_H2P + col] = fmaxf(acc[rb][r] + bias, 0.f);
      }
  }
  __syncthreads();

  // ---- layer 3 ---------------------------------------------------------------------------------------------------------
  constexpr int G3 = PN_C2 / 8, CB = PN_C3 / 4 / 32;   // 16 k-groups; 8 column blocks a wave
  const float* const a3 = pn_tile + lr * PN_H2P + 4 * lh;
  const float* const w3 = p.w3 + (int64_t)(wave * (PN_C3 / 4) + lr) * PN_C2 + 4 * lh;
  float* const out = p.feat + (int64_t)b * PN_C3 + wave * (PN_C3 / 4) + lr;
  const float* const b3 = p.b3 + wave * (PN_C3 / 4) + lr;

  auto load_w3 = [&](f32x4 (&bw)[G3], int cb) {
#pragma unroll
    for (int g = 0; g < G3; ++g) bw[g] = *reinterpret_cast<const f32x4*>(w3 + cb * 32 * PN_C2 + 8 * g);
  };
  auto block = [&](const f32x4 (&bw)[G3], int cb) {
    // every column block reads the same h2 image: the reads stay in the loop (hoisted out of it as loop invariants they
    // are 256 registers a lane, which spill)
    int again = 0;
    asm volatile("" : "+v"(again));
    const float* const a = a3 + again;
    float m = -INFINITY;
#pragma unroll
    for (int rb = 0; rb < PN_RB; ++rb) {
      const f32x16 acc = pn_mfma_block<G3>(a + rb * 32 * PN_H2P, bw);
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (lh == 0) {
      float v = m + b3[cb * 32];
      if (p.relu_last) v = fmaxf(v, 0.f);
      float* const o = out + cb * 32;
      if (p.direct) {
        *o = v;
      } else {
        const int iv = __float_as_int(v);
        if (iv >= 0)
          atomicMax(reinterpret_cast<int*>(o), iv);
        else
          atomicMin(reinterpret_cast<unsigned*>(o), (unsigned)iv);
      }
    }
  };

  f32x4 bwa[G3], bwb[G3];
  load_w3(bwa, 0);
#pragma unroll 1
  for (int cb = 0; cb < CB; cb += 2) {
    load_w3(bwb, cb + 1);
    block(bwa, cb);
    if (cb + 2 < CB) load_w3(bwa, cb + 2);
    block(bwb, cb + 1);
  }
}

__global__ void pointnet_fill_kernel(float* __restrict__ feat, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) feat[i] = -INFINITY;
}

}  // namespace

extern "C" int dgv2_pointnet_trunk(float* feat, const float* pts, const float* trans, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const float* w3, const float* b3, int B, int N,
                                   int relu_last, void* stream) {
  if (!feat || !pts || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return DGV2_EINVAL;
  if (B < 1 || N < 1 || (relu_last != 0 && relu_last != 1)) return DGV2_EINVAL;
  if (!aligned16(w2) || !aligned16(w3)) return DGV2_EINVAL;   // read with 16-byte loads
  const int64_t tiles = ((int64_t)N + PN_P - 1) / PN_P;
  if ((int64_t)B * tiles > DGV2_POINTNET_MAX_TILES) return DGV2_ENOTSUP;
  PnP p;
  p.feat = feat; p.pts = pts; p.trans = trans;
  p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.w3 = w3; p.b3 = b3;
  p.N = N; p.tiles = (int)tiles; p.relu_last = relu_last; p.direct = tiles == 1;
  hipStream_t st = (hipStream_t)stream;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)pointnet_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PN_LDS);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  if (!p.direct) {
    const int64_t n = (int64_t)B * PN_C3;   // B <= DGV2_POINTNET_MAX_TILES / 2 here: at most 2^29 blocks
    pointnet_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(feat, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  pointnet_trunk_kernel<<<(unsigned)(B * tiles), PN_THREADS, PN_LDS, st>>>(p);
  DGV2_RETURN_LAST();
}
