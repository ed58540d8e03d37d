// bf16_train.hip — the dense layers of the "bf16_dense" training precision on the bf16 matrix cores: bf16 operands,
// fp32 accumulation, one MFMA product per k step (the fp32 modes emulate fp32 with six bf16 products: gemm_x6.hip,
// fusion_x6.hip).
//
// Rounding: every operand is rounded to nearest-even by a plain cast (yl_pack_bf16: v_cvt_pk_bf16_f32, a NaN stays a NaN)
// on its way into LDS / registers; nothing of the truncating fx_split8 split is used (its h term alone is biased toward
// zero by ~2^-9 per operand, and that bias would go straight into the batch statistics).  Weights are read as fp32 and
// rounded in the same kernels, or (fusion forward) rounded into a bf16 image at the start of every call: no image
// outlives the call, so an Adam step can never leave a stale one behind.  Bias, BatchNorm statistics, the column sums of
// the bias gradient and the split-K reduction stay fp32, in a fixed order (deterministic: no float atomics).
//
// Kernels
//   k_bt_gemm<TA, TB>     C [M, N] = pro(A) . pro(B)^T over K, 64 x 64 workgroup tile (2 x 2 waves of 32 x 32, one
//                         v_mfma_f32_32x32x16_bf16 accumulator each), 32 k per LDS stage, the next stage's fp32 loads in
//                         registers while the current one's MFMAs run.  TA / TB: the operand is stored k-major ([K][M]),
//                         else row-major with k contiguous.  Epilogues: + bias, store or accumulate, BatchNorm partial
//                         statistics of the stored values (the layout yolat_bn_finalize reads), or a split-K partial.
//                         Serves the classifier layers 0 / 1 and fusion_block_super: forward (+ statistics), dX = dY . W,
//                         dW = dY^T . pro(A).
//   k_bt_fusion_rows      training fusion GEMM [N, 128] x [128, F] with the per-(proposal, column) extreme-of-z key
//                         epilogue of the fp32 training kernel (segmax.hpp fx_key64: same key, same tie rule), on the
//                         structure of fusion_h8.hip's k_hfusion_rows8: a wave's 32 rows of A as bf16 MFMA fragments in
//                         registers, the weight image streamed through a double-buffered LDS tile, one barrier per
//                         column tile.  The pooled value and the arg row k_pool_finish decodes come from the same key,
//                         i.e. from the same bf16 products.
#include "segmax.hpp"
#include "internal.hpp"

typedef unsigned bt_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bt_bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int BT_BM = 64, BT_BK = 32, BT_RS = BT_BK + 8;    // tile rows (M and N), k per stage, LDS row stride (bf16)
constexpr int BT_CS_ROWS = 32;                              // rows per column-sum partial (db)

struct BtOp {
  const float* p; long ld;
  const float *sc, *sh;      // nullable: v = sc[col] * v + sh[col] (col = stored column), then ReLU if relu
  int relu;
};

struct BtEpi {
  const float* bias;         // nullable, [N]
  float* out; long ldo;
  int accumulate;
  float* stats;              // nullable: float2 [ceil(M / 32)][N] (sum, M2) of the stored values per 32-row group
  long part;                 // split-K: element stride between the partial products of gridDim.z > 1
};

// 8 consecutive fp32 values of a stored row, prologue applied, rounded to bf16 (RNE) and packed
__device__ __forceinline__ bt_u32x4 bt_pack8(const BtOp& o, const float* src, int col0, bool ok) {
  float x[8];
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    if (o.sc != nullptr) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        x[i] = fmaf(x[i], o.sc[col0 + i], o.sh[col0 + i]);
        if (o.relu) x[i] = fmaxf(x[i], 0.f);
      }
    } else if (o.relu) {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = fmaxf(x[i], 0.f);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0.f;
  }
  const bt_u32x4 v = {yl_pack_bf16(x[0], x[1]), yl_pack_bf16(x[2], x[3]), yl_pack_bf16(x[4], x[5]),
                      yl_pack_bf16(x[6], x[7])};
  return v;
}

// one 64 (m or n) x 32 (k) operand tile: thread tid holds 8 packed bf16 values
//   !T (stored [MN][K], k contiguous): row tid / 4, k (tid % 4) * 8 .. +8          (K % 32 == 0)
//   T  (stored [K][MN], mn contiguous): k row tid / 8, mn (tid % 8) * 8 .. +8       (MN % 8 == 0)
template <bool T>
__device__ __forceinline__ bt_u32x4 bt_load(const BtOp& o, int mn0, int k0, int MN, int K, int tid) {
  if (!T) {
    const int r = tid >> 2, kq = (tid & 3) * 8, mn = mn0 + r;
    const bool ok = mn < MN;
    return bt_pack8(o, o.p + (long)(ok ? mn : 0) * o.ld + k0 + kq, k0 + kq, ok);
  } else {
    const int kr = tid >> 3, q = (tid & 7) * 8, k = k0 + kr, mn = mn0 + q;
    const bool ok = k < K && mn < MN;
    return bt_pack8(o, o.p + (long)(ok ? k : 0) * o.ld + (ok ? mn : 0), ok ? mn : 0, ok);
  }
}

template <bool T>
__device__ __forceinline__ void bt_store(unsigned short* S, const bt_u32x4& v, int tid) {
  if (!T) {
    *reinterpret_cast<bt_u32x4*>(&S[(tid >> 2) * BT_RS + (tid & 3) * 8]) = v;
  } else {
    const int kr = tid >> 3, q = (tid & 7) * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      S[(q + 2 * i) * BT_RS + kr] = (unsigned short)(v[i] & 0xFFFFu);
      S[(q + 2 * i + 1) * BT_RS + kr] = (unsigned short)(v[i] >> 16);
    }
  }
}

// C [M, N] = sum over k of A(m, k) B(n, k); gridDim = (N tiles, M tiles, k splits of kper)
template <bool TA, bool TB>
__global__ void __launch_bounds__(256) k_bt_gemm(BtOp A, BtOp B, BtEpi ep, int M, int N, int K, int kper) {
  __shared__ __attribute__((aligned(16))) unsigned short As[BT_BM * BT_RS];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[BT_BM * BT_RS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int n0 = blockIdx.x * BT_BM, m0 = blockIdx.y * BT_BM;
  const int kb = blockIdx.z * kper, ke = yl_min(K, kb + kper);
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  bt_u32x4 ra = {0u, 0u, 0u, 0u}, rb = {0u, 0u, 0u, 0u};
  if (kb < ke) {
    ra = bt_load<TA>(A, m0, kb, M, K, tid);
    rb = bt_load<TB>(B, n0, kb, N, K, tid);
  }
  for (int k0 = kb; k0 < ke; k0 += BT_BK) {
    __syncthreads();                                  // the previous stage's fragment reads are done
    bt_store<TA>(As, ra, tid);
    bt_store<TB>(Bs, rb, tid);
    __syncthreads();
    if (k0 + BT_BK < ke) {                            // next stage's loads in flight under this stage's MFMAs
      ra = bt_load<TA>(A, m0, k0 + BT_BK, M, K, tid);
      rb = bt_load<TB>(B, n0, k0 + BT_BK, N, K, tid);
    }
#pragma unroll
    for (int ks = 0; ks < BT_BK / 16; ++ks) {
      const bt_bf16x8 a = *reinterpret_cast<const bt_bf16x8*>(&As[(32 * wm + l31) * BT_RS + 16 * ks + 8 * lhi]);
      const bt_bf16x8 b = *reinterpret_cast<const bt_bf16x8*>(&Bs[(32 * wn + l31) * BT_RS + 16 * ks + 8 * lhi]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
  }
  // C layout: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 lhi of the wave's 32-row group
  const int col = n0 + 32 * wn + l31, rg = m0 + 32 * wm, rb0 = rg + 4 * lhi;
  const bool cok = col < N;
  if (gridDim.z > 1) {
    float* o = ep.out + (long)blockIdx.z * ep.part;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rb0 + (r & 3) + 8 * (r >> 2);
      if (cok && row < M) o[(long)row * N + col] = acc[r];
    }
    return;
  }
  const float bv = (ep.bias != nullptr && cok) ? ep.bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += bv;
  if (ep.stats != nullptr && rg < M) {
    const int cnt = yl_min(32, M - rg);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += (rb0 + (r & 3) + 8 * (r >> 2) < M) ? acc[r] : 0.f;
    s += __shfl_xor(s, 32);
    const float mean = s / (float)cnt;
    float q = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[r] - mean;
      q += (rb0 + (r & 3) + 8 * (r >> 2) < M) ? d * d : 0.f;
    }
    q += __shfl_xor(q, 32);
    if (lhi == 0 && cok) reinterpret_cast<float2*>(ep.stats)[(long)(rg >> 5) * N + col] = make_float2(s, q);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rb0 + (r & 3) + 8 * (r >> 2);
    if (cok && row < M) {
      float* o = ep.out + (long)row * ep.ldo + col;
      *o = ep.accumulate ? *o + acc[r] : acc[r];
    }
  }
}

// out[i] (row-major [rows, cols], ld) = sum over s of part[s * stride + i], s in order (deterministic split-K sum)
__global__ void __launch_bounds__(256) k_bt_reduce(const float* __restrict__ part, int S, long stride, long rows, int cols,
                                                   float* out, long ld) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[(long)z * stride + i];
  out[(i / cols) * ld + i % cols] = s;
}

// column sums of X [M, N] over row chunks of BT_CS_ROWS: part[chunk][n] (fp32, fixed order; short chunks, many
// workgroups: the loads of a thread are a short dependent chain, 256-row chunks were latency bound at ~100 us per call)
__global__ void __launch_bounds__(256) k_bt_colsum(const float* __restrict__ X, long ld, int M, int N, float* part) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int r0 = blockIdx.y * BT_CS_ROWS, r1 = yl_min(M, r0 + BT_CS_ROWS);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += X[(long)r * ld + n];
  part[(long)blockIdx.y * N + n] = s;
}

// bf16 image of W [F, K] (round to nearest even), the layout the rows kernel streams
__global__ void __launch_bounds__(256) k_bt_round(const float* __restrict__ W, long elems, unsigned short* __restrict__ out) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
  if (i >= elems) return;
  const unsigned u = yl_pack_bf16(W[i], i + 1 < elems ? W[i + 1] : 0.f);
  out[i] = (unsigned short)(u & 0xFFFFu);
  if (i + 1 < elems) out[i + 1] = (unsigned short)(u >> 16);
}

// ---- training fusion GEMM with the extreme-of-z key epilogue (K = 128) ----
struct BtFus {
  const float* A; long lda; int N;
  const unsigned short* W;   // [F, 128] bf16 image (no folding: z = A . W^T + bias is the pre-activation)
  const float* bias;         // [F]
  const float* sgn;          // [F]: the BatchNorm scale; its sign decides max or min
  const int* seg;            // [N] non-decreasing proposal ids
  unsigned long long* keys;  // [P, F]
  int F, groups, ng;
};

__global__ void __launch_bounds__(512, 2) k_bt_fusion_rows(BtFus p) {
  constexpr int KD = 128, KS = KD / 16, RS = KD + 8, CPR = KD / 8;
  constexpr int NW = 64 * CPR / 512;                        // 16-byte pieces of one W tile per thread
  __shared__ __attribute__((aligned(16))) unsigned short Ws[2][64 * RS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  // (row tile, column group) pairs, column group fastest, dealt to the XCDs in contiguous ranges
  int logical;
  {
    const int total = gridDim.x, chunk = total >> 3, rem = total & 7;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    logical = xcd * chunk + (xcd < rem ? xcd : rem) + slot;
  }
  const int N = p.N, F = p.F;
  const int rt = logical / p.groups, cg = logical % p.groups;
  const int tn = F >> 6, ct0 = cg * p.ng;
  const int ngl = yl_min(p.ng, tn - ct0);
  if (ngl <= 0) return;
  const int row0 = rt * 256 + wave * 32;
  // this wave's 32 rows of A as bf16 MFMA A fragments (lane = row, 8 consecutive k per lane half), rounded once
  bt_bf16x8 Afr[KS];
  {
    const long r = yl_min(row0 + l31, N - 1);
    const float* ap = p.A + r * p.lda + 8 * lhi;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4 a0 = *reinterpret_cast<const float4*>(ap + 16 * ks), a1 = *reinterpret_cast<const float4*>(ap + 16 * ks + 4);
      const bt_u32x4 v = {yl_pack_bf16(a0.x, a0.y), yl_pack_bf16(a0.z, a0.w), yl_pack_bf16(a1.x, a1.y),
                          yl_pack_bf16(a1.z, a1.w)};
      Afr[ks] = __builtin_bit_cast(bt_bf16x8, v);
    }
  }
  FxRuns runs;
  unsigned roff[16];                                        // proposal id x F of each of the lane's rows
  fx_seg_runs_off(row0 + l31 < N ? p.seg[row0 + l31] : -1, lhi, (unsigned)F, runs, roff);
  const unsigned wr0 = (unsigned)tid / CPR, wk = ((unsigned)tid % CPR) * 8;
  auto load_w = [&](int ct, bt_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const unsigned r = wr0 + (unsigned)t * (512 / CPR);
      rw[t] = *reinterpret_cast<const bt_u32x4*>(p.W + (unsigned)(ct * 64 + (int)r) * KD + wk);
    }
  };
  auto store_w = [&](int buf, const bt_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const unsigned r = wr0 + (unsigned)t * (512 / CPR);
      *reinterpret_cast<bt_u32x4*>(&Ws[buf][r * RS + wk]) = rw[t];
    }
  };
  bt_u32x4 rw[NW];
  load_w(ct0, rw);
  store_w(0, rw);
  __syncthreads();
  for (int j = 0; j < ngl; ++j) {
    const int ct = ct0 + j, buf = j & 1;
    const int c0 = ct * 64 + l31, c1 = c0 + 32;
    const float t0 = p.bias[c0], t1 = p.bias[c1];
    const unsigned m0 = p.sgn[c0] < 0.f ? 0x80000000u : 0u, m1 = p.sgn[c1] < 0.f ? 0x80000000u : 0u;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = t0; acc1[r] = t1; }
    if (j + 1 < ngl) load_w(ct + 1, rw);                  // in flight while the MFMAs below run
    const unsigned short* wb = &Ws[buf][l31 * RS + 8 * lhi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bt_bf16x8 b0 = *reinterpret_cast<const bt_bf16x8*>(wb + 16 * ks);
      const bt_bf16x8 b1 = *reinterpret_cast<const bt_bf16x8*>(wb + 32 * RS + 16 * ks);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Afr[ks], b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Afr[ks], b1, acc1, 0, 0, 0);
    }
    if (j + 1 < ngl) store_w(buf ^ 1, rw);               // (its readers finished before the last barrier)
    fx_key64(acc0, acc1, p.keys, roff, (unsigned)c0, true, true, m0, m1, (unsigned)(row0 + 4 * lhi), runs);
    __syncthreads();
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

static int bt_launch(bool ta, bool tb, const BtOp& a, const BtOp& b, const BtEpi& ep, long M, long N, long K, int S,
                     long kper, hipStream_t st) {
  dim3 grid(yl_cdiv(N, BT_BM), yl_cdiv(M, BT_BM), S);
  if (grid.y > 65535) return YOLAT_E_UNSUPPORTED;
  if (!ta && !tb) hipLaunchKernelGGL((k_bt_gemm<false, false>), grid, dim3(256), 0, st, a, b, ep, (int)M, (int)N, (int)K, (int)kper);
  else if (!ta && tb) hipLaunchKernelGGL((k_bt_gemm<false, true>), grid, dim3(256), 0, st, a, b, ep, (int)M, (int)N, (int)K, (int)kper);
  else if (ta && tb) hipLaunchKernelGGL((k_bt_gemm<true, true>), grid, dim3(256), 0, st, a, b, ep, (int)M, (int)N, (int)K, (int)kper);
  else return YOLAT_E_UNSUPPORTED;
  YL_LAUNCH_CHECK();
  return 0;
}

static bool bt_vec_ok(const float* p, long ld) { return p != nullptr && yl_aligned16(p) && ld % 4 == 0; }

extern "C" int yolat_bt_linear_fwd(const float* A, int64_t lda, int64_t M, int64_t K, const float* a_scale,
                                   const float* a_shift, int a_relu, const float* W, int64_t ldw, const float* bias,
                                   int64_t N, float* Y, int64_t ldy, float* stats, yolat_stream_t stream) {
  if (M <= 0 || K <= 0 || N <= 0 || !A || !W || !Y || lda < K || ldw < K || ldy < N || (a_scale == nullptr) != (a_shift == nullptr))
    return YOLAT_E_INVALID;
  if (K % BT_BK != 0 || !bt_vec_ok(A, lda) || !bt_vec_ok(W, ldw) || M >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  BtOp a{A, (long)lda, a_scale, a_shift, a_relu};
  BtOp b{W, (long)ldw, nullptr, nullptr, 0};
  BtEpi ep{bias, Y, (long)ldy, 0, stats, 0};
  return bt_launch(false, false, a, b, ep, M, N, K, 1, K, (hipStream_t)stream);
}

extern "C" int yolat_bt_linear_fwd_wt(const float* A, int64_t lda, int64_t M, int64_t K, const float* Wt, int64_t ldw,
                                      int64_t N, float* Y, int64_t ldy, int accumulate, yolat_stream_t stream) {
  if (M <= 0 || K <= 0 || N <= 0 || !A || !Wt || !Y || lda < K || ldw < N || ldy < N) return YOLAT_E_INVALID;
  if (K % BT_BK != 0 || N % 8 != 0 || !bt_vec_ok(A, lda) || !bt_vec_ok(Wt, ldw) || M >= (1LL << 31))
    return YOLAT_E_UNSUPPORTED;
  BtOp a{A, (long)lda, nullptr, nullptr, 0};
  BtOp b{Wt, (long)ldw, nullptr, nullptr, 0};
  BtEpi ep{nullptr, Y, (long)ldy, accumulate, nullptr, 0};
  return bt_launch(false, true, a, b, ep, M, N, K, 1, K, (hipStream_t)stream);
}

// split-K plan of the weight gradient: enough workgroups for the chip, every split a multiple of 32 rows
static void bt_dw_plan(long M, long N, long K, int* S, long* kper) {
  const long tiles = (long)yl_cdiv(N, BT_BM) * yl_cdiv(K, BT_BM);
  long s = (512 + tiles - 1) / tiles;
  const long smax = (M + 255) / 256;
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  long kp = (M + s - 1) / s;
  kp = (kp + BT_BK - 1) / BT_BK * BT_BK;
  *kper = kp;
  *S = (int)((M + kp - 1) / kp);
}

extern "C" size_t yolat_bt_linear_bwd_w_work_elems(int64_t M, int64_t N, int64_t K) {
  int S;
  long kper;
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  bt_dw_plan(M, N, K, &S, &kper);
  const size_t dw = S > 1 ? (size_t)S * N * K : 0;
  return dw + (size_t)yl_cdiv(M, BT_CS_ROWS) * N + 64;
}

extern "C" int yolat_bt_linear_bwd_w(const float* dY, int64_t ldd, int64_t M, int64_t N, const float* A, int64_t lda,
                                     int64_t K, const float* a_scale, const float* a_shift, int a_relu, float* dW,
                                     int64_t lddw, float* db, float* work, yolat_stream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !dY || !A || !dW || !work || ldd < N || lda < K || lddw < K ||
      (a_scale == nullptr) != (a_shift == nullptr))
    return YOLAT_E_INVALID;
  if (N % 8 != 0 || K % 8 != 0 || !bt_vec_ok(dY, ldd) || !bt_vec_ok(A, lda) || M >= (1LL << 31) ||
      (db != nullptr && yl_cdiv(M, BT_CS_ROWS) > 65535))
    return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  int S;
  long kper;
  bt_dw_plan(M, N, K, &S, &kper);
  // dW [N, K] = sum over rows m of dY[m, n] pro(A)[m, k]: GEMM rows n, columns k, reduction over m (both stored k-major)
  BtOp a{dY, (long)ldd, nullptr, nullptr, 0};
  BtOp b{A, (long)lda, a_scale, a_shift, a_relu};
  float* colpart = work + (S > 1 ? (size_t)S * N * K : 0);
  if (S > 1) {
    BtEpi ep{nullptr, work, 0, 0, nullptr, (long)(N * K)};
    YL_TRY(bt_launch(true, true, a, b, ep, N, K, M, S, kper, st));
    hipLaunchKernelGGL(k_bt_reduce, dim3(yl_cdiv(N * K, 256)), dim3(256), 0, st, work, S, (long)(N * K), (long)N, (int)K,
                       dW, (long)lddw);
    YL_LAUNCH_CHECK();
  } else {
    BtEpi ep{nullptr, dW, (long)lddw, 0, nullptr, 0};
    YL_TRY(bt_launch(true, true, a, b, ep, N, K, M, 1, kper, st));
  }
  if (db != nullptr) {
    const int nc = yl_cdiv(M, BT_CS_ROWS);
    hipLaunchKernelGGL(k_bt_colsum, dim3(yl_cdiv(N, 256), nc), dim3(256), 0, st, dY, (long)ldd, (int)M, (int)N, colpart);
    YL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bt_reduce, dim3(yl_cdiv(N, 256)), dim3(256), 0, st, colpart, nc, (long)N, 1L, (int)N, db, (long)N);
    YL_LAUNCH_CHECK();
  }
  return 0;
}

// The training fusion GEMM of fusion_train.hip step 4 in bf16: keys [P, F] (zeroed by the caller) <- per (proposal,
// column) extreme of sign(sgn) * (A . W^T + bias) with its lowest row.  W is rounded into `wimg` (F * 128 bf16, 16-byte
// aligned) first.  K == 128, F % 64 == 0.
int yl_fusion_rows_bf16_key64(const float* A, long lda, long N, long K, const float* W, const float* bias, long F,
                              const float* sgn, const int* node_seg, unsigned long long* keys, uint16_t* wimg,
                              yolat_stream_t stream) {
  if (K != 128 || F % 64 != 0 || lda % 4 != 0 || !yl_aligned16(A) || !yl_aligned16(wimg) || !bias)
    return YOLAT_E_UNSUPPORTED;
  if (N >= (1LL << 31) - 256 || (long long)N * F >= (1LL << 32)) return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bt_round, dim3(yl_cdiv(F * K, 512)), dim3(256), 0, st, W, (long)(F * K), wimg);
  YL_LAUNCH_CHECK();
  BtFus p;
  p.A = A; p.lda = lda; p.N = (int)N; p.W = wimg; p.bias = bias; p.sgn = sgn; p.seg = node_seg; p.keys = keys; p.F = (int)F;
  // column groups by the cost model of fusion_h8.hip: rounds x (1 prologue + tiles per workgroup), 2 workgroups per CU
  const int tn = (int)(F / 64), tm = yl_cdiv(N, 256);
  long best = -1;
  int groups = 1;
  for (int g = 1; g <= tn; g *= 2) {
    const long wgs = (long)tm * g, rounds = (wgs + 511) / 512;
    const long cost = rounds * (2 + yl_cdiv(tn, g));
    if (best < 0 || cost < best) { best = cost; groups = g; }
  }
  p.ng = yl_cdiv(tn, groups);
  p.groups = yl_cdiv(tn, p.ng);
  const long total = (long)tm * p.groups;
  if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_bt_fusion_rows, dim3((unsigned)total), dim3(512), 0, st, p);
  YL_LAUNCH_CHECK();
  return 0;
}
