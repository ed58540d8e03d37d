// fusion_x6.hip — eval-mode fusion block + per-proposal max pooling (architecture3cc_rpn_gp_iter2.py:61-63,122) with
// the [N,128] x [128,1024] GEMM as an fp32 GEMM EMULATED on the bf16 matrix cores (round 2).
//
// Why: the fp32-input MFMA of gfx950 executes on the SIMD's vector ALUs at the fp32 vector rate ("fp32 MFMA
// and the vector ALU"): the round-1 kernel (k_gemm_nt_two, 64x64 tiles) sits at 0.48 of that peak at cfg 2 and its
// epilogue VALU work adds to, not under, its MFMA time.  Both operands split exactly into three bfloat16 terms
// (truncation: 8 + 8 + 8 significand bits) and six products per 16 k — a_h b_l, a_l b_h, a_m b_m, a_m b_h, a_h b_m,
// a_h b_h, the three O(2^-24) ones dropped — give the fp32 result up to the summation order at 16/6 = 2.7x the
// fp32-MFMA rate, on a pipe that runs beside the VALU.
//
// Structure: a 512-thread workgroup (8 waves) owns 256 rows.  Every wave splits ITS 32 rows x K of A once into
// registers (3 x K/16 fragments = 96 VGPRs at K = 128) and keeps them for all the column tiles it walks; the weights —
// split once per weight version by yolat_split_bf16x3, BatchNorm scale folded into their rows — stream through a
// double-buffered LDS tile (3 x 64 columns x K bf16 = 48 KB, row stride K+8: conflict-free ds_read_b128), the next
// tile's 16-byte pieces loaded into registers while the current tile's 96 MFMAs per wave and its pooling epilogue
// run; one barrier per column tile.  W is re-streamed once per 256 rows (4x less L2 -> LDS traffic than 64-row
// tiles: at N = 200 k, 0.65 GB instead of 2.6 GB).  Pooling epilogue: the run-length integer atomicMax of
// bf16_eval.hip's rows kernel (values >= 0: int order == float order, exact, order-independent).
// fusion_block_super (P rows, its own weights, plain relu store) is a second problem of the same launch.
// The EVAL pair launch also exists with three half-precision products per 16 k instead of six bfloat16 ones
// (fusion_f16x3.hip k_fusion_rows_f16x3) — the eval forward's default; the training, node-side and Linear uses of the rows
// kernel stay on k_fusion_rows_x6.  Both kernels' workgroup shape and the launcher that picks an instantiation are
// fx_rows.hpp; the grid planner (fx_plan) and the pair launch's set-up (yl_fx_pair_setup) are here.
#include "x6.hpp"
#include "fx_rows.hpp"
#ifdef YOLAT_FX_STAMPS
extern __device__ long long fx_stamps_d[4096 * 32];
#define FX_EPI_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) fx_stamps_d[blockIdx.x * 32 + 25 + (k)] = wall_clock64(); } while (0)
#endif
#include "segmax.hpp"
#include "operands.hpp"
#include <map>

#ifdef YOLAT_FX_STAMPS
// debug build only (tools/exp/r06_fx_stamps.sh): wall-clock stamps (100 MHz) of thread 0 of every workgroup of the K = 128
// rows kernel, read back through yolat_debug_fx_stamps — where a workgroup's time goes
__device__ long long fx_stamps_d[4096 * 32];
#define FX_STAMP(k) do { if (KD == 128 && threadIdx.x == 0 && blockIdx.x < 4096) fx_stamps_d[blockIdx.x * 32 + (k)] = wall_clock64(); } while (0)
#define FX_STAMP_META()                                                                          \
  do {                                                                                           \
    if (KD == 128 && threadIdx.x == 0 && blockIdx.x < 4096) {                                    \
      fx_stamps_d[blockIdx.x * 32 + 21] = (long long)ngl;                                        \
      fx_stamps_d[blockIdx.x * 32 + 22] = (long long)(small ? 1 : 0);                            \
      unsigned xcc_;                                                                             \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                        \
      fx_stamps_d[blockIdx.x * 32 + 23] = (long long)xcc_;                                       \
    }                                                                                            \
  } while (0)
extern "C" int yolat_debug_fx_stamps(long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fx_stamps_d), sizeof(long long) * (size_t)n);
}
#else
#define FX_STAMP(k) do { } while (0)
#define FX_STAMP_META() do { } while (0)
#endif
// (the training-mode key epilogue fx_key / fx_key64 lives in segmax.hpp: the bf16 training kernel shares it)

// One GEMM problem of the launch: rows of A against the pre-split weights [F, KD]; seg != NULL -> pooling epilogue into
// `out` (pool); else plain store of act(.) — column tiles [0, ct2) into out [rows, ldo], column tiles [ct2, ...) into
// out2 [rows, ldo2] (its column 0 = column 64 * ct2 of the product), act = ReLU when relu != 0.  The defaults are a plain
// problem's: a launch site sets what differs.  (Field order and types are the kernel argument layout.)
struct FxProb {
  const float* A; long lda; int N;
  const yl_bf16_t *Wh, *Wm, *Wl;
  const float* tfold;
  const int* seg;
  float* out; long ldo;
  float* out2 = nullptr; long ldo2 = 0; int ct2 = 1 << 30;
  int F, relu;
  int tm, groups, ng;
  int full = 0;          // the first `full` row tiles (a multiple of 8) are walked WHOLE by one workgroup each (fx_plan)
  // training-mode pooling (fusion_train.hip): key64 != NULL (with seg) -> for every (proposal, column) the row with the
  // largest s*z (s = sign of sgn[column], z = the accumulator) is recorded by a 64-bit atomicMax on
  // orderable(s*z) << 32 | ~row (ties -> lowest row); nothing else is written
  unsigned long long* key64 = nullptr; const float* sgn = nullptr;
  // training-mode Linear (yolat_linear_fwd_rows_x6): optional prologue on A, v = max(a * a_scale[k] + a_shift[k],
  // a_floor) (BatchNorm + ReLU of the producer), and optional BatchNorm partial statistics of the stored values:
  // stats[(row / 32) * F + col] = (sum, M2) of the 32-row group (the layout yolat_bn_finalize reads)
  const float *a_scale = nullptr, *a_shift = nullptr; float a_floor = 0.f;
  float* stats = nullptr;
};

// RIDER = false: the rider argument is never read (an instantiation that reads it keeps more kernel arguments live:
// 75 -> 121 spilled SGPRs, and the cfg-5 fusion launch went 332 -> 365 us until the two were separated)
template <int KD, bool RIDER = false, int ACT = 0>
__global__ void __launch_bounds__(FxShape<KD>::T, 2) k_fusion_rows_x6(FxProb p0, FxProb p1, PoolRider rider,
                                                                      FxSlopes<ACT> slopes) {
  constexpr int T = FxShape<KD>::T, NWAVE = T / 64;
  constexpr int KS = KD / 16, RS = KD + 8, CPR = KD / 8;    // k steps, LDS row stride (bf16), 16-byte chunks per row
  constexpr int CHUNKS = 3 * 64 * CPR, NW = CHUNKS / T;     // 16-byte chunks of one W tile, per thread
  static_assert(CHUNKS % T == 0, "W tile / thread mismatch");
  constexpr int TK = 64, TS = TK + 4;                       // the prologue's transposition tile: [32 rows][TK + 4] floats per wave
  constexpr int SMEM_W = 2 * 3 * 64 * RS * 2, SMEM_T = NWAVE * 32 * TS * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM_W > SMEM_T ? SMEM_W : SMEM_T];
  yl_bf16_t (*Ws)[3 * 64 * RS] = reinterpret_cast<yl_bf16_t (*)[3 * 64 * RS]>(smem);
  constexpr int FX_STG_LD = 36;
  // per-wave staging tile of the plain-store epilogue — KD = 64 only (node side, training Linear): the KD = 128 kernel
  // sits at 248 registers and spilled with it
  __shared__ __attribute__((aligned(16))) float st_s[KD == 64 ? NWAVE * 32 * FX_STG_LD : 4];
  const int tid = threadIdx.x;
#include "fx_wg_map.inc"
  // the problem's fields as wave-uniform scalars (a reference to "p0 or p1" would make the compiler index the
  // kernel arguments through memory)
  struct { const float* A; long lda; int N; const float* tfold; const int* seg; float* out; long ldo; float* out2;
           long ldo2; int ct2, relu, groups, ng; unsigned long long* key64; const float* sgn; const float *a_scale,
           *a_shift; float a_floor; float* stats; } P;
  P.A = small ? p1.A : p0.A;
  P.lda = small ? p1.lda : p0.lda;
  P.N = small ? p1.N : p0.N;
  P.tfold = small ? p1.tfold : p0.tfold;
  P.seg = small ? p1.seg : p0.seg;
  P.out = small ? p1.out : p0.out;
  P.ldo = small ? p1.ldo : p0.ldo;
  P.out2 = small ? p1.out2 : p0.out2;
  P.ldo2 = small ? p1.ldo2 : p0.ldo2;
  P.ct2 = small ? p1.ct2 : p0.ct2;
  P.relu = small ? p1.relu : p0.relu;
  P.key64 = small ? p1.key64 : p0.key64;
  P.sgn = small ? p1.sgn : p0.sgn;
  P.a_scale = small ? p1.a_scale : p0.a_scale;
  P.a_shift = small ? p1.a_shift : p0.a_shift;
  P.a_floor = small ? p1.a_floor : p0.a_floor;
  P.stats = small ? p1.stats : p0.stats;
  const int F = small ? p1.F : p0.F;
  P.groups = small ? p1.groups : p0.groups;
  P.ng = small ? p1.ng : p0.ng;
  const float* __restrict__ A = P.A;
  const int N = P.N;
  const int tn = (F + 63) >> 6;
  float slope = 0.f;
  if constexpr (ACT != 0) slope = *(small ? slopes.s1 : slopes.s0);
  const int rt = whole ? logical : (small ? 0 : p0.full) + logical / P.groups;
  const int cg = whole ? 0 : logical % P.groups;
  const int ct0 = cg * P.ng;
  const int ngl = whole ? tn : yl_min(P.ng, tn - ct0);
  if (ngl <= 0) return;

  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt * (T / 2) + wave * 32;
  FX_STAMP(0);
  // (round 6) everything the tile loop needs besides A goes out FIRST — the rows' proposal ids, the first W tile, its
  // shifts and sign masks: their latency runs under the A prologue instead of after it (stamps: 1.5 us of a cfg-2
  // workgroup's 23.5 lay between the end of the split and the first MFMA)
  const int sv_pre = (P.seg != nullptr && row0 + l31 < N) ? P.seg[row0 + l31] : -1;
  const yl_bf16_t* const wparts[3] = {small ? p1.Wh : p0.Wh, small ? p1.Wm : p0.Wm, small ? p1.Wl : p0.Wl};
#define FX_W_CLAMP 1
#include "fx_w_movers.inc"
#undef FX_W_CLAMP
  fx_u32x4 rw[NW];
  load_w(ct0, rw);
  // shifts (and, training mode, the sign-bit masks of the key) of the first tile; later tiles: fetched one tile ahead,
  // BEFORE that tile's W loads, so that no wait on them ever sits behind younger loads or the epilogue's atomics (vmcnt
  // retires in order).  (Rounds 2-5 loaded the signs inside the epilogue: an exposed L2 round trip per column tile.)
  float t0 = P.tfold[yl_min(ct0 * 64 + l31, F - 1)], t1 = P.tfold[yl_min(ct0 * 64 + 32 + l31, F - 1)];
  unsigned sm0 = 0u, sm1 = 0u;
  if (P.key64 != nullptr) {
    sm0 = P.sgn[yl_min(ct0 * 64 + l31, F - 1)] < 0.f ? 0x80000000u : 0u;
    sm1 = P.sgn[yl_min(ct0 * 64 + 32 + l31, F - 1)] < 0.f ? 0x80000000u : 0u;
  }
  // ---- this wave's 32 rows of A, split once.  Loaded row by row (a row's 64 floats of the pass = 16 lanes x 16 bytes:
  // whole cache lines per instruction, eight loads in flight) and turned into the MFMA operand order (lane = row, 8
  // consecutive k) through a [32][TK + 4] fp32 tile in LDS — the weights' buffers, not yet in use.  (Reading the operand
  // order straight from memory, every lane its own row, as a chain of dependent 16-byte loads was 126 of the kernel's
  // 350 us at N = 200 k: profiles/r03_fusion_x6_ablation.txt.)
  fx_bf16x8 Ah[KS], Am[KS], Al[KS];
  {
    float* Tt = reinterpret_cast<float*>(smem) + wave * (32 * TS);
    const int lr = lane >> 4, lc = (lane & 15) * 4;
#pragma unroll
    for (int q = 0; q < KD / TK; ++q) {
      float4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        v[i] = *reinterpret_cast<const float4*>(A + (long)yl_min(row0 + 4 * i + lr, N - 1) * P.lda + TK * q + lc);
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<float4*>(Tt + (4 * i + lr) * TS + lc) = v[i];
#pragma unroll
      for (int u = 0; u < TK / 16; ++u) {
        const int ks = (TK / 16) * q + u;
        const float4 a0 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi);
        const float4 a1 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi + 4);
        float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        if (P.a_scale != nullptr) {
          const float* sp = P.a_scale + 16 * ks + 8 * lhi;
          const float* hp = P.a_shift + 16 * ks + 8 * lhi;
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = fmaxf(fmaf(x[e], sp[e], hp[e]), P.a_floor);
        }
        fx_split8(x, Ah[ks], Am[ks], Al[ks]);
      }
    }
  }
  FX_STAMP(1);
  const bool pooling = P.seg != nullptr;
  FxRuns runs;
  unsigned roff[16];                                    // element offset of each of the lane's rows' proposal in the output
  fx_seg_runs_off(sv_pre, lhi, P.key64 != nullptr ? (unsigned)F : (unsigned)P.ldo, runs, roff);
  FX_STAMP(2);
  __syncthreads();                                          // every wave is done with its transposition tile
  store_w(0, rw);
  __syncthreads();
  FX_STAMP(3);
  for (int j = 0; j < ngl; ++j) {
    const int ct = ct0 + j, buf = j & 1;
    const int c0 = ct * 64 + l31, c1 = c0 + 32;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = t0; acc1[r] = t1; }
    const unsigned m0 = sm0, m1 = sm1;
    if (j + 1 < ngl) {
      t0 = P.tfold[yl_min(c0 + 64, F - 1)];
      t1 = P.tfold[yl_min(c1 + 64, F - 1)];
      if (P.key64 != nullptr) {
        sm0 = P.sgn[yl_min(c0 + 64, F - 1)] < 0.f ? 0x80000000u : 0u;
        sm1 = P.sgn[yl_min(c1 + 64, F - 1)] < 0.f ? 0x80000000u : 0u;
      }
      load_w(ct + 1, rw);                              // in flight while the MFMAs below run
    }
    const yl_bf16_t* wb = &Ws[buf][l31 * RS + 8 * lhi];
    // B fragments: column block 0 / 1 x hi / mid / lo; the compiler issues the next k step's reads as registers free up
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fx_bf16x8 bf[6];                                 // [0] b0h [1] b1h [2] b0m [3] b1m [4] b0l [5] b1l
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        bf[q] = *reinterpret_cast<const fx_bf16x8*>(wb + q * 32 * RS + 16 * ks);
      }
      // small terms first.  The empty asm ties both accumulators after every MFMA: it pins the MFMAs' program order
      // (instruction selection otherwise pairs up MFMAs on the same accumulator) and emits nothing
#define FX_MFMA(acc, a, b)                                         \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); \
  asm volatile("" : "+v"(acc0), "+v"(acc1))
      FX_MFMA(acc0, Al[ks], bf[0]);
      FX_MFMA(acc1, Al[ks], bf[1]);
      FX_MFMA(acc0, Ah[ks], bf[4]);
      FX_MFMA(acc1, Ah[ks], bf[5]);
      FX_MFMA(acc0, Am[ks], bf[2]);
      FX_MFMA(acc1, Am[ks], bf[3]);
      FX_MFMA(acc0, Am[ks], bf[0]);
      FX_MFMA(acc1, Am[ks], bf[1]);
      FX_MFMA(acc0, Ah[ks], bf[2]);
      FX_MFMA(acc1, Ah[ks], bf[3]);
      FX_MFMA(acc0, Ah[ks], bf[0]);
      FX_MFMA(acc1, Ah[ks], bf[1]);
#undef FX_MFMA
    }
    // next W tile into the other buffer (its readers finished before the last barrier) BEFORE the epilogue: the
    // wait for its loads then never includes the epilogue's atomics / stores
    FX_STAMP(4 + 4 * (j & 3));
    if (j + 1 < ngl) store_w(buf ^ 1, rw);
    // everything still in flight here (next tile's shifts and W pieces, the previous tile's atomics) was issued a
    // whole MFMA phase ago: waiting now costs nothing and keeps the compiler from waiting on the shifts at the top
    // of the next tile, where the wait would also cover this tile's atomics (vmcnt retires in order)
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
    FX_STAMP(5 + 4 * (j & 3));
    if (pooling && P.key64 != nullptr) {
      fx_key64(acc0, acc1, P.key64, roff, (unsigned)c0, c0 < F, c1 < F, m0, m1, (unsigned)(row0 + 4 * lhi), runs);
    } else if (pooling) {
      if constexpr (ACT != 0) fx_segmax2_off_act(acc0, acc1, P.out, roff, (unsigned)c0, c0 < F, c1 < F, runs, slope);
      else fx_segmax2_off(acc0, acc1, P.out, roff, (unsigned)c0, c0 < F, c1 < F, runs);
    } else if constexpr (ACT != 0) {
      // plain store of act(.) (fusion_block_super: P rows): the accumulator layout as it is — a few row tiles per launch
      unsigned rb = (unsigned)(row0 + 4 * lhi);
      asm volatile("" : "+v"(rb));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned row = rb + (r & 3) + 8 * (r >> 2);
        if ((int)row < N) {
          float* o = P.out + (unsigned long)row * (unsigned long)P.ldo;
          if (c0 < F) o[c0] = acc0[r] > 0.f ? acc0[r] : slope * acc0[r];
          if (c1 < F) o[c1] = acc1[r] > 0.f ? acc1[r] : slope * acc1[r];
        }
      }
    } else {
      // the row base goes through an opaque asm so that the 16 row addresses are recomputed here instead of being
      // kept in 32 registers across the MFMA loop
      unsigned rb = (unsigned)(row0 + 4 * lhi);
      asm volatile("" : "+v"(rb));
      if (P.stats != nullptr) {
        // BatchNorm partial statistics of this wave's 32-row group, as wave_epilogue (epilogue.hpp) takes them
        int cnt = N - row0;
        cnt = cnt > 32 ? 32 : cnt;
        if (cnt > 0) {
          float s0 = 0.f, s1 = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool ok = row0 + (r & 3) + 8 * (r >> 2) + 4 * lhi < N;
            s0 += ok ? acc0[r] : 0.f;
            s1 += ok ? acc1[r] : 0.f;
          }
          s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32);
          const float m0 = s0 / (float)cnt, m1 = s1 / (float)cnt;
          float q0 = 0.f, q1 = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool ok = row0 + (r & 3) + 8 * (r >> 2) + 4 * lhi < N;
            const float d0 = acc0[r] - m0, d1 = acc1[r] - m1;
            q0 += ok ? d0 * d0 : 0.f;
            q1 += ok ? d1 * d1 : 0.f;
          }
          q0 += __shfl_xor(q0, 32); q1 += __shfl_xor(q1, 32);
          if (lhi == 0) {
            float2* sp = reinterpret_cast<float2*>(P.stats) + (long)(row0 >> 5) * F;
            if (c0 < F) sp[c0] = make_float2(s0, q0);
            if (c1 < F) sp[c1] = make_float2(s1, q1);
          }
        }
      }
      const bool second = ct >= P.ct2;
      float* const ob = second ? P.out2 : P.out;
      const unsigned long old = (unsigned long)(second ? P.ldo2 : P.ldo);
      const int cb = second ? 64 * P.ct2 : 0;
      const float lo = P.relu ? 0.f : -INFINITY;
      // full tile, 16-byte aligned rows: the two 32 x 32 blocks go row-major through this wave's staging tile, so that
      // every lane stores 16 bytes and one instruction covers 8 rows x 128 bytes (in the accumulator layout a store
      // instruction is 4 bytes per lane, 2 rows x 128 bytes: 4x the instructions for the node side's 205 MB)
      if (KD == 64 && row0 + 32 <= N && ct * 64 + 64 <= F && (old & 3) == 0 && ((uintptr_t)ob & 15) == 0) {
        float* stg = st_s + wave * (32 * FX_STG_LD);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            stg[((r & 3) + 8 * (r >> 2) + 4 * lhi) * FX_STG_LD + l31] = fmaxf(blk == 0 ? acc0[r] : acc1[r], lo);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int chunk = lane + 64 * t, R = chunk >> 3, c = (chunk & 7) * 4;
            *reinterpret_cast<float4*>(ob + (unsigned long)(row0 + R) * old - cb + ct * 64 + 32 * blk + c) =
                *reinterpret_cast<const float4*>(stg + R * FX_STG_LD + c);
          }
        }
      } else
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned row = rb + (r & 3) + 8 * (r >> 2);
        if ((int)row < N) {
          float* o = ob + (unsigned long)row * old - cb;
          if (c0 < F) o[c0] = fmaxf(acc0[r], lo);
          if (c1 < F) o[c1] = fmaxf(acc1[r], lo);
        }
      }
    }
    FX_STAMP(6 + 4 * (j & 3));
    __syncthreads();
    FX_STAMP(7 + 4 * (j & 3));
  }
  FX_STAMP(20);
  FX_STAMP_META();
}

// W [rows, cols] fp32 (optionally scaled per row) -> three bfloat16 matrices hi / mid / lo [rows, cols] with
// hi + mid + lo == fl(row_scale * W) exactly.
static __global__ void k_split_bf16x3(const float* __restrict__ W, long ldw, long rows, int cols,
                                      const float* __restrict__ row_scale, yl_bf16_t* __restrict__ hi,
                                      yl_bf16_t* __restrict__ mid, yl_bf16_t* __restrict__ lo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const long r = i / cols;
  float x = W[r * ldw + (i % cols)];
  if (row_scale != nullptr) x *= row_scale[r];
  const unsigned u = __float_as_uint(x);
  const float h = __uint_as_float(u & 0xffff0000u), hm = __uint_as_float(u & 0xffffff00u);
  const float m = hm - h, l = x - hm;
  hi[i] = (yl_bf16_t)(u >> 16);
  mid[i] = (yl_bf16_t)(__float_as_uint(m) >> 16);
  lo[i] = (yl_bf16_t)(__float_as_uint(l) >> 16);
}

extern "C" int yolat_split_bf16x3(const float* W, int64_t ldw, int64_t rows, int64_t cols, const float* row_scale,
                                  uint16_t* hi, uint16_t* mid, uint16_t* lo, yolat_stream_t stream) {
  if (rows <= 0 || cols <= 0 || !W || !hi || !mid || !lo || ldw < cols) return YOLAT_E_INVALID;
  hipLaunchKernelGGL(k_split_bf16x3, dim3(yl_cdiv(rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, W, (long)ldw,
                     (long)rows, (int)cols, row_scale, hi, mid, lo);
  YL_LAUNCH_CHECK();
  return 0;
}

// Work split of the big problem (round 4).  One launch runs in rounds of `slots` resident workgroups; a workgroup costs one
// prologue (load + three-way split of its rows of A, measured ~ one column tile's time) plus its column tiles.  Rounds 2-3
// picked ONE power-of-two column split for all row tiles, i.e. paid either the round quantisation of whole-row workgroups
// (782 row tiles on 256 slots: 4 rounds of 17 units for 3.05 rounds of work) or a prologue per few column tiles (4 column
// tiles per workgroup at cfg 5: 5 units for 4 of work).  Now the first `full` row tiles — whole rounds — go to one workgroup
// each, and only the remainder is split into column groups: the plan with the smallest makespan of a list schedule in
// dispatch order (small problem's workgroups, cost 2; whole-row workgroups, cost 1 + tn; tail workgroups, cost 1 + ng).
namespace {
struct FxPlan { int full, groups, ng; };
double fx_makespan(int slots, long n_small, long n_full, int c_full, long n_tail, int c_tail) {
  // list schedule in dispatch order on identical slots (the next job goes to the slot that frees first), simulated on GROUPS
  // of slots with equal finish time instead of job by job: the jobs of a class are identical, so the k = min(jobs left,
  // group size) jobs that go to the earliest group move k of its slots to (time + cost) in one step.  A step per
  // (class, round) instead of a heap operation per job: the plan of a 200 k-row launch costs microseconds, not 0.6 ms
  // (every new (N, P) of a data loader is a cache miss in fx_plan).
  std::map<double, long> t;
  t[0.0] = slots;
  double last = 0.0;
  auto run = [&](long n, double c) {
    while (n > 0) {
      auto it = t.begin();
      const double at = it->first;
      const long k = n < it->second ? n : it->second;
      it->second -= k;
      if (it->second == 0) t.erase(it);
      t[at + c] += k;
      if (at + c > last) last = at + c;
      n -= k;
    }
  };
  run(n_small, 2.0);
  run(n_full, (double)c_full);
  run(n_tail, (double)c_tail);
  return last;
}
FxPlan fx_plan(int tm, int tn, long n_small, int slots) {
  struct Key { int tm, tn, slots; long n_small; FxPlan plan; };
  static thread_local Key cache[8];
  static thread_local int used = 0, next = 0;
  for (int i = 0; i < used; ++i)
    if (cache[i].tm == tm && cache[i].tn == tn && cache[i].slots == slots && cache[i].n_small == n_small) return cache[i].plan;
  FxPlan best{0, 1, tn};
  double best_t = 1e300;
  // whole rounds only (slots is a multiple of 8); candidates: none, all whole rounds, one round fewer — the schedule is
  // simulated job by job, and very large inputs would otherwise try hundreds of values
  const int f1 = (tm / slots) * slots;
  const int cand[3] = {0, f1, f1 >= slots ? f1 - slots : 0};
  for (int ci = 0; ci < 3; ++ci) {
    const int full = cand[ci];
    if (ci > 0 && full == cand[ci - 1]) continue;
    for (int g = 1; g <= tn; g *= 2) {
      const int ng = yl_cdiv(tn, g), groups = yl_cdiv(tn, ng);
      if (full == tm && g > 1) break;
      const double t = fx_makespan(slots, n_small, full, 1 + tn, (long)(tm - full) * groups, 1 + ng);
      if (t < best_t - 1e-9) { best_t = t; best = FxPlan{full, groups, ng}; }
    }
  }
  cache[next] = Key{tm, tn, slots, n_small, best};
  next = (next + 1) & 7;
  if (used < 8) ++used;
  return best;
}

struct FxX6 {
  using Prob = FxProb;
  template <int KD, bool RIDER, int ACT>
  static void launch(unsigned grid, hipStream_t st, const FxProb& p0, const FxProb& p1, const PoolRider& pr, FxSlopes<ACT> sl) {
    hipLaunchKernelGGL((k_fusion_rows_x6<KD, RIDER, ACT>), dim3(grid), dim3(FxShape<KD>::T), 0, st, p0, p1, pr, sl);
  }
};
}  // namespace

// What the x6 and the f16x3 pair launch share before the launch: the argument check, the grid and the rider copy.  The
// weights differ in number and kind, so their NULL and alignment terms arrive evaluated (w_null, w_unaligned).  The two
// checks differ in ONE term, kept as it was: f16x3 also declines P * ldys >= 2^32 (ys_span32), x6 does not.
// Grid.  A workgroup costs one prologue (load + split of its rows of A, measured ~ one column tile's time) plus its column
// tiles; fx_plan splits the node problem, the small problem always gets the finest split (its few row tiles must not become
// the longest workgroups).
int yl_fx_pair_setup(const float* A, int64_t lda, int64_t N, int64_t D, const float* tfold, int64_t F, const int32_t* node_seg,
                     float* pool, int64_t ldpool, const float* S, int64_t lds, int64_t P, const float* tsfold, float* Ys,
                     int64_t ldys, bool w_null, bool w_unaligned, bool ys_span32, const PoolRider* rider, const float* slope_f,
                     const float* slope_s, FxPairGrid* g) {
  if ((slope_f == nullptr) != (slope_s == nullptr)) return YOLAT_E_INVALID;
  if (N <= 0 || P <= 0 || F <= 0 || !A || w_null || !tfold || !node_seg || !pool || !S || !tsfold || !Ys) return YOLAT_E_INVALID;
  if (N >= (1LL << 31) - 256 || lda < D || lds < D || ldpool < F || ldys < F) return YOLAT_E_INVALID;
  if ((D != 64 && D != 128) || F % 64 != 0 || lda % 4 != 0 || lds % 4 != 0 || !yl_aligned16(A) || !yl_aligned16(S) ||
      w_unaligned || (int64_t)P * ldpool >= (1LL << 32) || (ys_span32 && (int64_t)P * ldys >= (1LL << 32)))
    return YOLAT_E_UNSUPPORTED;
  const int rows_wg = D == 64 ? FxShape<64>::ROWS : FxShape<128>::ROWS, wg_round = D == 64 ? 512 : 256;
  g->tn = (int)(F / 64);
  g->tm0 = yl_cdiv(N, rows_wg);
  g->tm1 = yl_cdiv(P, rows_wg);
  const long n1 = (((long)g->tm1 * g->tn + 7) & ~7L);
  const FxPlan plan = fx_plan(g->tm0, g->tn, n1, wg_round);
  g->full = plan.full; g->groups = plan.groups; g->ng = plan.ng;
  g->rider = PoolRider{};
  if (rider && rider->blocks > 0) g->rider = *rider;
  const long total = (long)g->full + (long)(g->tm0 - g->full) * g->groups + n1 + g->rider.blocks;
  if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  g->total = (unsigned)total;
  return 0;
}

// pool[p, 0:F] = max over the rows of proposal p of relu(A . (sf (.) Wf)^T + tfold),  Ys = relu(S . (sfs (.) Wfs)^T
// + tsfold): both fusion blocks with pre-split weights (yolat_split_bf16x3 of the scaled rows) and folded shifts
// (s*b + t).  `pool` must be zero-filled first (yolat_pool_prepare).  D in {64, 128}, F % 64 == 0.
int yl_fusion_pair_eval_x6_impl(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh, const uint16_t* Wm,
                                const uint16_t* Wl, const float* tfold, int64_t F, const int32_t* node_seg, float* pool,
                                int64_t ldpool, const float* S, int64_t lds, int64_t P, const uint16_t* Wsh,
                                const uint16_t* Wsm, const uint16_t* Wsl, const float* tsfold, float* Ys, int64_t ldys,
                                const PoolRider* rider, yolat_stream_t stream, const float* slope_f,
                                const float* slope_s) {
  FxPairGrid g;
  YL_TRY(yl_fx_pair_setup(A, lda, N, D, tfold, F, node_seg, pool, ldpool, S, lds, P, tsfold, Ys, ldys,
                          !Wh || !Wm || !Wl || !Wsh || !Wsm || !Wsl,
                          !yl_aligned16(Wh) || !yl_aligned16(Wm) || !yl_aligned16(Wl) || !yl_aligned16(Wsh) ||
                              !yl_aligned16(Wsm) || !yl_aligned16(Wsl),
                          /*ys_span32=*/false, rider, slope_f, slope_s, &g));
  // (leaky activation: `pool` holds -inf / 0 per proposal, yolat_pool_init_signed, not zeros)
  const int relu = slope_f == nullptr;
  FxProb p0, p1;
  p0.A = A; p0.lda = lda; p0.N = (int)N; p0.Wh = Wh; p0.Wm = Wm; p0.Wl = Wl; p0.tfold = tfold; p0.seg = node_seg;
  p0.out = pool; p0.ldo = ldpool; p0.F = (int)F; p0.relu = relu;
  p0.tm = g.tm0; p0.full = g.full; p0.groups = g.groups; p0.ng = g.ng;
  p1.A = S; p1.lda = lds; p1.N = (int)P; p1.Wh = Wsh; p1.Wm = Wsm; p1.Wl = Wsl; p1.tfold = tsfold; p1.seg = nullptr;
  p1.out = Ys; p1.ldo = ldys; p1.F = (int)F; p1.relu = relu;
  p1.tm = g.tm1; p1.groups = g.tn; p1.ng = 1;
  fx_launch_rows<FxX6>(D, g.total, p0, p1, g.rider, slope_f, slope_s, (hipStream_t)stream);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_fusion_pair_eval_x6(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh,
                                         const uint16_t* Wm, const uint16_t* Wl, const float* tfold, int64_t F,
                                         const int32_t* node_seg, float* pool, int64_t ldpool, const float* S,
                                         int64_t lds, int64_t P, const uint16_t* Wsh, const uint16_t* Wsm,
                                         const uint16_t* Wsl, const float* tsfold, float* Ys, int64_t ldys,
                                         yolat_stream_t stream) {
  return yl_fusion_pair_eval_x6_impl(A, lda, N, D, Wh, Wm, Wl, tfold, F, node_seg, pool, ldpool, S, lds, P, Wsh, Wsm, Wsl,
                                     tsfold, Ys, ldys, nullptr, stream);
}

// The activation-aware pair launch (leaky activations, act.hip): pool[p, 0:F] = max over the rows of proposal p of
// act_f(A . (sf (.) Wf)^T + tfold), 0 for an empty proposal; Ys = act_s(S . (sfs (.) Wfs)^T + tsfold).  Two launches: the
// signed start values of `pool` from seg_ptr (-inf / 0), then the ACT instantiation of the rows kernel.
extern "C" int yolat_fusion_pair_eval_x6_act(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh,
                                             const uint16_t* Wm, const uint16_t* Wl, const float* tfold, int64_t F,
                                             const float* slope_f, const int32_t* node_seg, const int32_t* seg_ptr,
                                             float* pool, int64_t ldpool, const float* S, int64_t lds, int64_t P,
                                             const uint16_t* Wsh, const uint16_t* Wsm, const uint16_t* Wsl,
                                             const float* tsfold, const float* slope_s, float* Ys, int64_t ldys,
                                             yolat_stream_t stream) {
  if (!slope_f || !slope_s || !seg_ptr) return YOLAT_E_INVALID;
  YL_TRY(yolat_pool_init_signed(seg_ptr, P, F, pool, ldpool, stream));
  return yl_fusion_pair_eval_x6_impl(A, lda, N, D, Wh, Wm, Wl, tfold, F, node_seg, pool, ldpool, S, lds, P, Wsh, Wsm, Wsl,
                                     tsfold, Ys, ldys, nullptr, stream, slope_f, slope_s);
}

// Training-mode fusion GEMM (fusion_train.hip step 4) on the rows kernel: z = A . W^T + bias never stored, per
// (proposal, column) extreme-of-z keys.  W [F, K] fp32 is split here (it changes every step) into `wsplit`
// (3 * F * K bfloat16, 16-byte aligned).  K in {64, 128}, F % 64 == 0; returns YOLAT_E_UNSUPPORTED otherwise.
int yl_fusion_rows_x6_key64(const float* A, long lda, long N, long K, const float* W, const float* bias, long F,
                            const float* sgn, const int* node_seg, unsigned long long* keys, uint16_t* wsplit,
                            yolat_stream_t stream) {
  if ((K != 64 && K != 128) || F % 64 != 0 || lda % 4 != 0 || !yl_aligned16(A) || !yl_aligned16(wsplit) || !bias)
    return YOLAT_E_UNSUPPORTED;
  // (the kernel addresses the keys with 32-bit element offsets proposal id x F; ids are < N)
  if (N >= (1LL << 31) - 256 || (long long)N * F >= (1LL << 32)) return YOLAT_E_UNSUPPORTED;
  uint16_t *wh = wsplit, *wm = wsplit + F * K, *wl = wsplit + 2 * F * K;
  const int rc = yolat_split_bf16x3(W, K, F, K, nullptr, wh, wm, wl, stream);
  if (rc != 0) return rc;
  const int tn = (int)(F / 64);
  FxProb p0, p1;
  p0.A = A; p0.lda = lda; p0.N = (int)N; p0.Wh = wh; p0.Wm = wm; p0.Wl = wl; p0.tfold = bias; p0.seg = node_seg;
  p0.out = nullptr; p0.ldo = F; p0.F = (int)F; p0.relu = 0;
  p0.key64 = keys; p0.sgn = sgn;
  const int rows_wg = K == 64 ? FxShape<64>::ROWS : FxShape<128>::ROWS, wg_round = K == 64 ? 512 : 256;
  p0.tm = yl_cdiv(N, rows_wg);
  const FxPlan plan = fx_plan(p0.tm, tn, 0, wg_round);
  p0.full = plan.full; p0.groups = plan.groups; p0.ng = plan.ng;
  p1 = p0;
  p1.tm = 0; p1.groups = 1; p1.ng = 1; p1.full = 0;
  const long total = (long)p0.full + (long)(p0.tm - p0.full) * p0.groups;
  if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  fx_launch_rows<FxX6>(K, (unsigned)total, p0, p1, PoolRider{}, nullptr, nullptr, (hipStream_t)stream);
  YL_LAUNCH_CHECK();
  return 0;
}

// Training-mode Linear on the rows kernel:  Y [M, Nout] = pro(A) [M, K] . W^T + bias  (pre-activation), with the optional
// BatchNorm+ReLU prologue on A and the optional BatchNorm partial statistics of Y (yolat_linear_fwd's `stats`).  W [Nout,
// K] fp32 (contiguous rows, ldw) is split here — it changes every step — into `wsplit` (3 * Nout * K bfloat16, 16-byte
// aligned).  K in {64, 128}, Nout % 64 == 0, lda % 4 == 0.  For many rows (one workgroup per 256 rows): the second edge
// Linear of a training conv layer, [E, 64] -> [E, 64] (torch_vertex.py:311,335 nn.3).
extern "C" int yolat_linear_fwd_rows_x6(const float* A, int64_t lda, int64_t M, int64_t K, const float* a_scale,
                                        const float* a_shift, int a_relu, const float* W, int64_t ldw, const float* bias,
                                        int64_t Nout, float* Y, int64_t ldy, float* stats, uint16_t* wsplit,
                                        yolat_stream_t stream) {
  if (M <= 0 || !A || !W || !bias || !Y || !wsplit || lda < K || ldw < K || ldy < Nout) return YOLAT_E_INVALID;
  if ((a_scale == nullptr) != (a_shift == nullptr) || (a_relu && !a_scale)) return YOLAT_E_INVALID;
  if ((K != 64 && K != 128) || Nout <= 0 || Nout % 64 != 0 || lda % 4 != 0 || !yl_aligned16(A) || !yl_aligned16(wsplit) ||
      M >= (1LL << 31) - 256)
    return YOLAT_E_UNSUPPORTED;
  uint16_t *wh = wsplit, *wm = wsplit + Nout * K, *wl = wsplit + 2 * Nout * K;
  const int rc = yolat_split_bf16x3(W, ldw, Nout, K, nullptr, wh, wm, wl, stream);
  if (rc != 0) return rc;
  const int tn = (int)(Nout / 64);                     // the bias is the accumulators' initial value
  FxProb p0, p1;
  p0.A = A; p0.lda = lda; p0.N = (int)M; p0.Wh = wh; p0.Wm = wm; p0.Wl = wl; p0.tfold = bias; p0.seg = nullptr;
  p0.out = Y; p0.ldo = ldy; p0.F = (int)Nout; p0.relu = 0;
  p0.a_scale = a_scale; p0.a_shift = a_shift; p0.a_floor = a_relu ? 0.f : -INFINITY; p0.stats = stats;
  p0.tm = yl_cdiv(M, K == 64 ? FxShape<64>::ROWS : FxShape<128>::ROWS); p0.groups = 1; p0.ng = tn;
  p1 = p0;
  p1.tm = 0; p1.groups = 1; p1.ng = 1;
  const long total = (long)p0.tm;
  if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  fx_launch_rows<FxX6>(K, (unsigned)total, p0, p1, PoolRider{}, nullptr, nullptr, (hipStream_t)stream);
  YL_LAUNCH_CHECK();
  return 0;
}

// Node side of a factorised conv layer (eval, C = Cin = 64) on the same rows kernel: UV = f_in . Wuv'^T + uv_bias
// (two column tiles -> UV [N, 128]) and root = f_in . Wr^T + br (third column tile -> f_out) as one problem with the
// stacked, pre-split weights Wfr [192, 64] and shifts tfr [192]; the node branch relu(s_in . (sn (.) Wn)^T + tn') as the
// second problem.  Replaces yolat_node_uv_eval (three fp32-MFMA GEMMs in one launch) — the same launch count, the
// products on the bf16 matrix cores, A read once per 256 rows.
extern "C" int yolat_node_uv_eval_x6(const float* f_in, int64_t ld_f, const float* s_in, int64_t ld_s, int64_t N,
                                     const uint16_t* Wfr_h, const uint16_t* Wfr_m, const uint16_t* Wfr_l, const float* tfr,
                                     const uint16_t* Wn_h, const uint16_t* Wn_m, const uint16_t* Wn_l, const float* tn_fold,
                                     float* UV, int64_t ld_uv, float* f_out, int64_t ld_fo, float* s_out, int64_t ld_so,
                                     yolat_stream_t stream) {
  if (N <= 0 || N >= (1LL << 31) - 256 || !f_in || !s_in || !Wfr_h || !Wfr_m || !Wfr_l || !tfr || !Wn_h || !Wn_m || !Wn_l ||
      !tn_fold || !UV || !f_out || !s_out)
    return YOLAT_E_INVALID;
  if (ld_f < 64 || ld_s < 64 || ld_uv < 128 || ld_fo < 64 || ld_so < 64) return YOLAT_E_INVALID;
  if (ld_f % 4 != 0 || ld_s % 4 != 0 || !yl_aligned16(f_in) || !yl_aligned16(s_in) || !yl_aligned16(Wfr_h) ||
      !yl_aligned16(Wfr_m) || !yl_aligned16(Wfr_l) || !yl_aligned16(Wn_h) || !yl_aligned16(Wn_m) || !yl_aligned16(Wn_l))
    return YOLAT_E_UNSUPPORTED;
  FxProb p0, p1;
  p0.A = f_in; p0.lda = ld_f; p0.N = (int)N; p0.Wh = Wfr_h; p0.Wm = Wfr_m; p0.Wl = Wfr_l; p0.tfold = tfr; p0.seg = nullptr;
  p0.out = UV; p0.ldo = ld_uv; p0.out2 = f_out; p0.ldo2 = ld_fo; p0.ct2 = 2; p0.F = 192; p0.relu = 0;
  p0.tm = yl_cdiv(N, FxShape<64>::ROWS); p0.groups = 1; p0.ng = 3;
  p1.A = s_in; p1.lda = ld_s; p1.N = (int)N; p1.Wh = Wn_h; p1.Wm = Wn_m; p1.Wl = Wn_l; p1.tfold = tn_fold; p1.seg = nullptr;
  p1.out = s_out; p1.ldo = ld_so; p1.F = 64; p1.relu = 1;
  p1.tm = yl_cdiv(N, FxShape<64>::ROWS); p1.groups = 1; p1.ng = 1;
  const long total = (long)p0.tm * p0.groups + (((long)p1.tm * p1.groups + 7) & ~7L);
  if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  fx_launch_rows<FxX6>(64, (unsigned)total, p0, p1, PoolRider{}, nullptr, nullptr, (hipStream_t)stream);
  YL_LAUNCH_CHECK();
  return 0;
}
