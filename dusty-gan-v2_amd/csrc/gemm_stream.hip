// gemm_stream.hip -- the generator's level-0 / level-1 per-sample-weight contractions (bf16) with a deeper operand
// delivery than the generic engines of gemm_core.h.  The ARITHMETIC is the generic engines': same block tile, same
// fragment ownership, one v_mfma_f32_16x16x32_bf16 per K-step of 32 into one accumulator per fragment in ascending K,
// same epilogue in the same order -- every output, every sum-of-squares partial and its slot are the generic kernels'
// bit for bit.  What differs is how the operands reach the matrix cores:
//
//   NN  (weights A [O][K], pixels B [P][K], both K-contiguous; tile 128 channels x 128 pixels, wave w = pixels 32w..)
//     * a stage is FOUR K-steps (128 channels = whole 256-byte row pieces) per __syncthreads, not one;
//     * the pixel rows of a wave are read by that wave alone, so they never touch LDS: a lane's 16-byte global load of
//       row n0 + 32 w + 16 nf + (lane & 15), chunk 4 kt + (lane >> 4) IS its B fragment (conv1x1.hip's scheme);
//     * the weights are shared by the four waves and go through LDS in whole stages, double buffered, 16-byte slots
//       XOR-swizzled by (row & 15) so that both the row-wise stores and the ds_read_b128 fragment reads are conflict-free;
//     * the loads of stage s + 1 are in flight across the 64 MFMAs of stage s: eight 16-byte loads of A per lane from
//       the top of the stage, and the two B loads of step kt from the moment step kt of stage s has issued its MFMAs
//       (into the registers it has just released).
//   TN  (gy [P][O], x [P][J], K = pixels; tile 64 x 128, fp32 out, no split-K)
//     * a stage is four 32-pixel K-steps (twelve 16-byte loads per thread in flight), one LDS image (48 KB: three
//       blocks per CU), fragments through the same ds_read_b64_tr_b16 reads as gemm_tn_kernel;
//     * the fp32 tile is transposed through the (then idle) LDS and leaves in 16-byte stores, 512-byte runs per row.
#include <type_traits>

#include "gemm_core.h"

namespace {

constexpr int kStageSteps = 4;   // K-steps of 32 per stage

// Branch-free operand sources (a branch around a load would make the next load wait for it).  One type serves the dense
// and the concatenated operands: element k < Ka of a row comes from the per-sample `a`, the rest from the batch-shared `s`
// (dense: Ka = K).  Indices past the operand are CLAMPED to its last row / chunk instead of zero-filled: a valid address
// whose value feeds only accumulator rows / columns that the epilogue never stores, and K-steps that are never issued.
// Addresses are a wave-uniform base plus a 32-bit lane offset; the row parts are computed once per block.
struct RowSrc {   // NN: a [rows][K] K-contiguous operand; one sample's part stays below 2^31 elements (32-bit offsets)
  const bf16_t* a;
  int64_t a_batch_stride;
  int lda, Ka;      // Ka % 32 == 0: a K-step lies on one side of the split
  const bf16_t* s;
  int lds_, rows, K;
};
__device__ __forceinline__ uint4 ld16(const bf16_t* base /* wave-uniform */, unsigned off /* elements */) {
  return *reinterpret_cast<const uint4*>(base + off);
}
// the zero fill of the rows k >= K (they are summed), applied where the chunk is STORED to LDS: a mask, not a select (the
// compiler turns `k < K ? load : 0` into a branch around the load), and not at the load (it would be waited for there)
__device__ __forceinline__ uint4 zero_past(uint4 v, int64_t k, int64_t K) {
  const unsigned keep = k < K ? ~0u : 0u;
  return make_uint4(v.x & keep, v.y & keep, v.z & keep, v.w & keep);
}
struct ColSrc {   // TN: 8 consecutive columns of row min(k, K - 1) of a [K][cols] operand
  const bf16_t* a;
  int64_t a_batch_stride;
  int lda, Ca;
  const bf16_t* s;
  int lds_, cols;
  __device__ __forceinline__ uint4 load(int batch, int64_t k, int64_t K, int colchunk) const {
    const int64_t kk = k < K ? k : K - 1;
    const int col = min(colchunk * 8, cols - 8);
    const bf16_t* pa = a + batch * a_batch_stride + kk * lda + col;
    const bf16_t* ps = s + kk * lds_ + (col - Ca);
    return *reinterpret_cast<const uint4*>(col < Ca ? pa : ps);   // rows k >= K: see zero_past()
  }
};

// ----------------------------------------------------------------------------------------------
// NN.  Same template interface as gemm_nn_kernel<bf16_t, 128, ...>; K % 32 == 0.
// ----------------------------------------------------------------------------------------------
// __launch_bounds__' second argument is the minimum number of WAVES per SIMD; a 256-thread block is one wave per SIMD, so
// here (and only at this block size) it reads as blocks per CU: 2 caps the kernel at 256 VGPRs.
template <class Epi, bool BATCH_FAST>
__global__ __launch_bounds__(256, 2) void gemm_nn_stream_kernel(RowSrc al, RowSrc bl, Epi epi, int K) {
  constexpr int TO = 128, TP = 128, MF = TO / 16, NF = 2, KT = kStageSteps;
  constexpr int ROWCH = 4 * KT;                  // 16-byte chunks per row and stage
  constexpr int ACH = TO * ROWCH / 256;          // A chunks per thread and stage
  __shared__ __attribute__((aligned(16))) uint4 ldsA[2][TO * ROWCH];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lc = lane >> 4;
  const int batch = BATCH_FAST ? blockIdx.x : blockIdx.z;
  const int m0 = blockIdx.y * TO;
  const int n0 = (BATCH_FAST ? blockIdx.z : blockIdx.x) * TP;
  const int nk = K >> 5;
  const int ns = (nk + KT - 1) / KT;

  uint4 ra[ACH], rb[KT][NF];
  auto swz = [](int row, int ch) { return row * ROWCH + (ch ^ (row & (ROWCH - 1))); };
  const bf16_t* abase = al.a + batch * al.a_batch_stride;
  const bf16_t* bbase_a = bl.a + batch * bl.a_batch_stride;
  unsigned offA[ACH], offBa[NF], offBs[NF];
#pragma unroll
  for (int i = 0; i < ACH; ++i) offA[i] = (unsigned)min(m0 + (tid + i * 256) / ROWCH, al.rows - 1) * (unsigned)al.lda;
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const unsigned r = (unsigned)min(n0 + wave * 32 + nf * 16 + lr, bl.rows - 1);
    offBa[nf] = r * (unsigned)bl.lda + lc * 8;
    offBs[nf] = r * (unsigned)bl.lds_ + lc * 8;
  }
  auto gloadA = [&](int s) {
    const unsigned k = (unsigned)min(s * (32 * KT) + (tid % ROWCH) * 8, K - 8);   // past K only in a last, partial stage
#pragma unroll
    for (int i = 0; i < ACH; ++i) ra[i] = ld16(abase, offA[i] + k);
  };
  auto gloadB = [&](int s, int kt) {
    const int k0 = min((s * KT + kt) * 32, K - 32);   // wave-uniform, and so is the side of the split
    const bool side_a = k0 < bl.Ka;
    const bf16_t* base = side_a ? bbase_a : bl.s;
    const unsigned k = (unsigned)(side_a ? k0 : k0 - bl.Ka);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) rb[kt][nf] = ld16(base, (side_a ? offBa[nf] : offBs[nf]) + k);
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int id = tid + i * 256;
      ldsA[buf][swz(id / ROWCH, id % ROWCH)] = ra[i];
    }
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  gloadA(0);
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) gloadB(0, kt);
  lstore(0);
  __syncthreads();
  // KN K-steps of stage s, ascending (KN is a compile-time count: no MFMA sits under a per-step branch).  PRE: the B
  // fragments of step kt of the NEXT stage are requested into the registers step kt has just released.
  auto steps = [&](auto knc, auto prec, int s, int cur) {
    constexpr int KN = decltype(knc)::value;
    constexpr bool PRE = decltype(prec)::value;
#pragma unroll
    for (int kt = 0; kt < KN; ++kt) {
      uint4 a[MF];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) a[mf] = ldsA[cur][swz(mf * 16 + lr, kt * 4 + lc)];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) Mfma16<bf16_t>::run(acc[mf][nf], a[mf], rb[kt][nf]);
      if (PRE) {
        __builtin_amdgcn_sched_barrier(0);   // the loads stay here, behind the MFMAs that read their registers
        gloadB(s + 1, kt);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  int cur = 0;
  for (int s = 0; s + 1 < ns; ++s) {   // every stage but the last is whole and has a successor: straight-line body
    gloadA(s + 1);                     // in flight across this stage's MFMAs, stored to LDS behind them
    __builtin_amdgcn_sched_barrier(0);   // (left alone, the scheduler sinks these loads to the LDS stores that use them)
    steps(std::integral_constant<int, KT>(), std::true_type(), s, cur);
    lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  {
    const int kn = nk - (ns - 1) * KT;   // wave-uniform, 1 .. KT
    if (kn >= KT) steps(std::integral_constant<int, KT>(), std::false_type(), ns - 1, cur);
    else if (kn == 3) steps(std::integral_constant<int, 3>(), std::false_type(), ns - 1, cur);
    else if (kn == 2) steps(std::integral_constant<int, 2>(), std::false_type(), ns - 1, cur);
    else steps(std::integral_constant<int, 1>(), std::false_type(), ns - 1, cur);
  }
  __syncthreads();   // the LDS image is idle from here on (block_sum reuses it)
  // from here on: gemm_nn_kernel's epilogue, statement for statement (the order the per-thread `ss` is summed in)
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
      epi(batch, m0 + mf * 16 + lc * 4, n0 + wave * 32 + nf * 16 + lr, acc[mf][nf]);
  if (epi.sumsq) {
    float* red = reinterpret_cast<float*>(&ldsA[0][0]);
    const float s = block_sum(epi.ss, red);
    if (tid == 0) epi.sumsq[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
  }
}

// ----------------------------------------------------------------------------------------------
// TN.  gemm_tn_kernel<bf16_t, 64, 128, ...> with ksplit == 1; J % 4 == 0, out 16-byte aligned rows.
// ----------------------------------------------------------------------------------------------
// (256, 3): three waves per SIMD = three 256-thread blocks per CU, 168 VGPRs at the most
__global__ __launch_bounds__(256, 3) void gemm_tn_stream_kernel(ColSrc al, ColSrc bl, float* __restrict__ out, int M, int J,
                                                             int64_t K, int64_t out_batch_stride, int ldo) {
  constexpr int TO = 64, TJ = 128, KS = 32, CE = 8, KT = kStageSteps;
  constexpr int MF = TO / 16, NF = TJ / 64;
  constexpr int ACH_ROW = TO / CE, BCH_ROW = TJ / CE;
  constexpr int ACH = KT * KS * ACH_ROW / 256, BCH = KT * KS * BCH_ROW / 256;
  constexpr int OLD = TJ + 4;   // row pitch (floats) of the fp32 tile on its way out
  static_assert(TO * OLD * 4 <= KT * KS * (TO + TJ) * 2, "the output tile reuses the operand image");
  __shared__ __attribute__((aligned(16))) bf16_t lds[KT * KS * (TO + TJ)];
  bf16_t* ldsA = lds;
  bf16_t* ldsB = lds + KT * KS * TO;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int batch = blockIdx.z;
  const int m0 = blockIdx.y * TO;
  const int j0 = blockIdx.x * TJ;
  const int nk = (int)((K + KS - 1) / KS);
  const int ns = (nk + KT - 1) / KT;

  uint4 ra[ACH], rb[BCH];
  auto gload = [&](int s) {
    const int64_t kb = (int64_t)s * (KT * KS);
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int id = tid + i * 256;
      ra[i] = al.load(batch, kb + id / ACH_ROW, K, (m0 / CE) + id % ACH_ROW);
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int id = tid + i * 256;
      rb[i] = bl.load(batch, kb + id / BCH_ROW, K, (j0 / CE) + id % BCH_ROW);
    }
  };
  auto lstore = [&](int s) {
    const int64_t kb = (int64_t)s * (KT * KS);
#pragma unroll
    for (int i = 0; i < ACH; ++i)
      reinterpret_cast<uint4*>(ldsA)[tid + i * 256] = zero_past(ra[i], kb + (tid + i * 256) / ACH_ROW, K);
#pragma unroll
    for (int i = 0; i < BCH; ++i)
      reinterpret_cast<uint4*>(ldsB)[tid + i * 256] = zero_past(rb[i], kb + (tid + i * 256) / BCH_ROW, K);
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto step = [&](int kt) {
    uint4 a[MF], b[NF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) a[mf] = TnFrag<bf16_t>::template read<TO>(ldsA + kt * KS * TO, mf * 16, lane);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
      b[nf] = TnFrag<bf16_t>::template read<TJ>(ldsB + kt * KS * TJ, wave * (TJ / 4) + nf * 16, lane);
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) Mfma16<bf16_t>::run(acc[mf][nf], a[mf], b[nf]);
  };

  if (ns > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int s = 0; s < ns; ++s) {
    if (s + 1 < ns) gload(s + 1);
    const int kn = nk - s * KT;
    if (kn >= KT) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) step(kt);
    } else {
      for (int kt = 0; kt < kn; ++kt) step(kt);
    }
    __syncthreads();
    if (s + 1 < ns) {
      lstore(s + 1);
      __syncthreads();
    }
  }
  // the tile [m][j] through LDS (the loop's last barrier has retired every fragment read), then rows of 16-byte stores
  float* ot = reinterpret_cast<float*>(lds);
  const int lr = lane & 15, lc = lane >> 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) ot[(mf * 16 + lc * 4 + r) * OLD + wave * (TJ / 4) + nf * 16 + lr] = acc[mf][nf][r];
  __syncthreads();
  float* ob = out + batch * out_batch_stride;
#pragma unroll
  for (int i = 0; i < TO * (TJ / 4) / 256; ++i) {
    const int id = tid + i * 256;
    const int m = id / (TJ / 4), jv = (id % (TJ / 4)) * 4;
    if (m0 + m >= M || j0 + jv >= J) continue;   // J % 4 == 0: a 4-column group is inside or outside as a whole
    *reinterpret_cast<f32x4*>(ob + (int64_t)(m0 + m) * ldo + j0 + jv) = *reinterpret_cast<const f32x4*>(ot + m * OLD + jv);
  }
}

bool nn_geometry(int dtype, int ydtype, int K, int O) {
  return dtype == DGV2_BF16 && ydtype == DGV2_BF16 && O > 64 && K % 32 == 0;   // O > 64: the generic TO = 128 instance
}

int take_sumsq(StoreEpilogue<bf16_t>& epi, dim3 grid, float* sumsq, int sumsq_cap, int* sumsq_used) {
  const int64_t nblk = (int64_t)grid.x * grid.y * grid.z;
  if (sumsq && sumsq_used && nblk <= sumsq_cap) {
    epi.sumsq = sumsq;
    *sumsq_used = (int)nblk;
  }
  return 0;
}

}  // namespace

// dgv2_bmm_nn_sq on the staged delivery; same arguments, same results.  DGV2_ENOTSUP outside bf16 in / bf16 out, O > 64,
// I % 32 == 0, ldx % 8 == 0, wstride % 8 == 0, ldy % 4 == 0 and 16-byte aligned y / x / w / resid.
extern "C" int dgv2_gemm_stream_nn(void* y, const void* x, const void* w, int B, int P, int I, int O, int ldx, int ldy,
                                   int64_t wstride, const float* row_scale, const float* bias, int act, float alpha,
                                   float scale, const void* resid, int dtype, int ydtype, float* sumsq, int sumsq_cap,
                                   int* sumsq_used, void* stream) {
  if (sumsq_used) *sumsq_used = 0;
  if (!y || !x || !w || B <= 0 || P <= 0 || I <= 0 || O <= 0 || ldx < I || ldy < O) return DGV2_EINVAL;
  if (act != 0 && act != 3) return DGV2_EINVAL;
  if (!nn_geometry(dtype, ydtype, I, O) || (int64_t)P * ldx >= (1ll << 31) || (int64_t)O * I >= (1ll << 31) || ldx % 8 || wstride % 8 || ldy % 4 || !aligned16(y) || !aligned16(x) || !aligned16(w)
      || (resid && !aligned16(resid)))
    return DGV2_ENOTSUP;
  typedef bf16_t T;
  RowSrc al{(const T*)w, wstride, I, I, (const T*)w, I, O, I};
  RowSrc bl{(const T*)x, (int64_t)P * ldx, ldx, I, (const T*)x, ldx, P, I};
  StoreEpilogue<T> epi{(T*)y, (int64_t)P * ldy, ldy, O, P, true, bias, act, alpha, scale, nullptr, 0.f, row_scale, (const T*)resid};
  dim3 grid((P + 127) / 128, (O + 127) / 128, B);
  take_sumsq(epi, grid, sumsq, sumsq_cap, sumsq_used);
  gemm_nn_stream_kernel<StoreEpilogue<T>, false>
      <<<grid, 256, 0, (hipStream_t)stream>>>(al, bl, epi, I);
  DGV2_RETURN_LAST();
}

// dgv2_bmm_nn_cat_sq on the staged delivery.  DGV2_ENOTSUP outside bf16 in / bf16 out, O > 64, O % 4 == 0 and
// Ka % 32 == 0, Ks % 32 == 0 (whole K-steps on either side of the split, which may fall inside a stage).
extern "C" int dgv2_gemm_stream_nn_cat(void* y, const void* xa, const void* xs, const void* w, int B, int P, int Ka, int Ks,
                                       int O, const float* row_scale, const float* bias, int act, float alpha, float scale,
                                       int dtype, int ydtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream) {
  if (sumsq_used) *sumsq_used = 0;
  if (!y || !xs || !w || (Ka > 0 && !xa) || B <= 0 || P <= 0 || Ka < 0 || Ks <= 0 || O <= 0) return DGV2_EINVAL;
  if (act != 0 && act != 3) return DGV2_EINVAL;
  if (dtype != DGV2_BF16 && dtype != DGV2_F32) return DGV2_EINVAL;
  const int ce = dtype == DGV2_BF16 ? 8 : 4;
  if (Ka % ce || Ks % ce || !aligned16(xs) || (Ka > 0 && !aligned16(xa)) || !aligned16(w) || !aligned16(y))
    return DGV2_EINVAL;   // what dgv2_bmm_nn_cat_sq itself refuses
  if (!nn_geometry(dtype, ydtype, Ka + Ks, O) || O % 4 || Ka % 32 || (int64_t)P * (Ka > Ks ? Ka : Ks) >= (1ll << 31)
      || (int64_t)O * (Ka + Ks) >= (1ll << 31))
    return DGV2_ENOTSUP;
  typedef bf16_t T;
  const int K = Ka + Ks;
  RowSrc al{(const T*)w, (int64_t)O * K, K, K, (const T*)w, K, O, K};
  RowSrc bl{(const T*)xa, (int64_t)P * Ka, Ka, Ka, (const T*)xs, Ks, P, K};
  StoreEpilogue<T> epi{(T*)y, (int64_t)P * O, O, O, P, true, bias, act, alpha, scale, nullptr, 0.f, row_scale};
  dim3 grid(B, (O + 127) / 128, (P + 127) / 128);
  take_sumsq(epi, grid, sumsq, sumsq_cap, sumsq_used);
  gemm_nn_stream_kernel<StoreEpilogue<T>, true>
      <<<grid, 256, 0, (hipStream_t)stream>>>(al, bl, epi, K);
  DGV2_RETURN_LAST();
}

// dgv2_bmm_tn on the staged delivery.  DGV2_ENOTSUP outside bf16, O > 32 (the generic TO = 64 instance), no split-K
// (see dgv2_bmm_tn), I % 8 == 0, ldgy % 8 == 0, ldx % 8 == 0 and 16-byte aligned gw / gy / x.
extern "C" int dgv2_gemm_stream_tn(float* gw, const void* gy, const void* x, int B, int P, int I, int O, int ldgy, int ldx,
                                   int dtype, void* stream) {
  if (!gw || !gy || !x || B <= 0 || P <= 0 || I <= 0 || O <= 0 || ldgy < O || ldx < I) return DGV2_EINVAL;
  if (dtype != DGV2_BF16 && dtype != DGV2_F32) return DGV2_EINVAL;
  if (dtype != DGV2_BF16 || O <= 32 || bmm_tn_ksplit(B, P, I, O) != 1 || I % 8 || O % 8 || ldgy % 8 || ldx % 8 || !aligned16(gw)
      || !aligned16(gy) || !aligned16(x))
    return DGV2_ENOTSUP;
  typedef bf16_t T;
  ColSrc al{(const T*)gy, (int64_t)P * ldgy, ldgy, O, (const T*)gy, ldgy, O};
  ColSrc bl{(const T*)x, (int64_t)P * ldx, ldx, I, (const T*)x, ldx, I};
  dim3 grid((I + 127) / 128, (O + 63) / 64, B);
  gemm_tn_stream_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(al, bl, gw, O, I, P, (int64_t)O * I, I);
  DGV2_RETURN_LAST();
}

// dgv2_bmm_tn_cat on the staged delivery; DGV2_ENOTSUP as dgv2_gemm_stream_tn (J = Ka + Ks), O % 8 == 0.
extern "C" int dgv2_gemm_stream_tn_cat(float* gw, const void* gy, const void* xa, const void* xs, int B, int P, int Ka,
                                       int Ks, int O, int dtype, void* stream) {
  if (!gw || !gy || !xs || (Ka > 0 && !xa) || B <= 0 || P <= 0 || Ka < 0 || Ks <= 0 || O <= 0) return DGV2_EINVAL;
  if (dtype != DGV2_BF16 && dtype != DGV2_F32) return DGV2_EINVAL;
  const int ce = dtype == DGV2_BF16 ? 8 : 4;
  if (Ka % ce || Ks % ce || !aligned16(xs) || (Ka > 0 && !aligned16(xa))) return DGV2_EINVAL;
  const int J = Ka + Ks;
  if (dtype != DGV2_BF16 || O <= 32 || O % 8 || bmm_tn_ksplit(B, P, J, O) != 1 || !aligned16(gw) || !aligned16(gy))
    return DGV2_ENOTSUP;
  typedef bf16_t T;
  ColSrc al{(const T*)gy, (int64_t)P * O, O, O, (const T*)gy, O, O};
  ColSrc bl{(const T*)xa, (int64_t)P * Ka, Ka, Ka, (const T*)xs, Ks, J};
  dim3 grid((J + 127) / 128, (O + 63) / 64, B);
  gemm_tn_stream_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(al, bl, gw, O, J, P, (int64_t)O * J, J);
  DGV2_RETURN_LAST();
}
