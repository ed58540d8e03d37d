// rownorm.hip — the row norms of gcn_lib/sparse/torch_nn.py:23-34: nn.LayerNorm(nc, elementwise_affine=True) and
// nn.InstanceNorm1d(nc, affine=False) on a 2-D [M, nc] input.  Both are ONE per-row arithmetic, the same in train() and eval():
//   z = (y - mean) / sqrt(var + eps) * gamma + beta,   mean / biased var over the nc columns of the row,
// gamma / beta NULL for the instance norm.  Unlike BatchNorm it cannot be folded into the Linear in front of it.
//   yolat_rownorm_act, yolat_rownorm_act_bwd      the op and its backward (training, classifier layers of the eval forward)
//   yolat_fusion_pair_eval_x6_rn                  eval fusion block: GEMM + row norm + ReLU + per-proposal max in one launch,
//                                                 the [N, F] matrix never written (k_fusion_rows_rn below)
//   yolat_fusion_pair_eval_rn                     the same for any D / F, materialising row ranges in a capped workspace
// Numerics: the variance is always the mean of CENTRED squares (never E[y^2] - mean^2).  The row kernels centre on the
// row's first element before they sum (a constant row has an exactly zero deviation: z = beta exactly); the fused kernel
// never sees the mean at all — its weights arrive centred (see k_fusion_rows_rn).
#include "x6.hpp"
#include "segmax.hpp"
#include "operands.hpp"
#include "internal.hpp"

namespace {
__device__ __forceinline__ float rn_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;                                                   // (a butterfly: every lane holds the same bits)
}

// ---- Z = relu?(rownorm(Y) * gamma + beta): one wave per row, 4 rows per workgroup.  REG: the row lives in registers
// (C <= 1024: 16 values per lane, column = lane + 64 i — whole cache lines per load); else it is re-read per pass.
// Z may be Y: a lane writes only elements it has read itself.
template <bool REG>
__global__ void __launch_bounds__(256) k_rownorm_act(const float* Y, long ldy, long M, int C, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, int relu, float* Z, long ldz,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63;
  const float inv_c = 1.f / (float)C;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < M; r += (long)gridDim.x * 4) {
    const float* y = Y + r * ldy;
    float* z = Z + r * ldz;
    const float y0 = y[0];
    float v[REG ? 16 : 1];
    float s = 0.f;
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? y[c] - y0 : 0.f;
        s += v[i];
      }
    } else {
      for (int c = lane; c < C; c += 64) s += y[c] - y0;
    }
    const float ms = rn_wave_sum(s) * inv_c;                  // mean - y0
    float q = 0.f;
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = lane + 64 * i < C ? v[i] - ms : 0.f;
        v[i] = d;
        q = fmaf(d, d, q);
      }
    } else {
      for (int c = lane; c < C; c += 64) { const float d = (y[c] - y0) - ms; q = fmaf(d, d, q); }
    }
    const float rstd = 1.f / sqrtf(rn_wave_sum(q) * inv_c + eps);
    if (lane == 0) {
      if (mean_out) mean_out[r] = y0 + ms;
      if (rstd_out) rstd_out[r] = rstd;
    }
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
          float o = v[i] * rstd;
          if (gamma) o = fmaf(o, gamma[c], beta[c]);
          z[c] = relu ? fmaxf(o, 0.f) : o;
        }
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float o = ((y[c] - y0) - ms) * rstd;
        if (gamma) o = fmaf(o, gamma[c], beta[c]);
        z[c] = relu ? fmaxf(o, 0.f) : o;
      }
    }
  }
}

// ---- backward.  With xh = (Y - mean) rstd and z' = gamma xh + beta RECOMPUTED from the saved pre-norm Y:
//   g = relu ? (z' > 0 ? dZ : 0) : dZ
//   per 256-row block and column: (sum g, sum g xh)                          k_rn_bwd_partial   (gamma != NULL only)
//   fp64 sums over the blocks in block order -> dgamma, dbeta                k_rn_bwd_finalize
//   dY = rstd (g gamma - mean_c(g gamma) - xh mean_c(g gamma xh))            k_rn_bwd_rows: one wave per row
// Every sum has a fixed order: two calls give identical bits.  dY may be dZ (the partial sums are taken first).
constexpr int RNB_ROWS = 256;
__device__ __forceinline__ float rn_gate(float dz, float xh, float ga, float be, int relu) {
  return (!relu || fmaf(xh, ga, be) > 0.f) ? dz : 0.f;
}
__global__ void __launch_bounds__(256) k_rn_bwd_partial(const float* dZ, long lddz, const float* Y, long ldy, long M, int C,
                                                        const float* mean, const float* rstd, const float* gamma,
                                                        const float* beta, int relu, float* part) {
  __shared__ float red[2][4][64];
  const int cl = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const long r0 = (long)blockIdx.y * RNB_ROWS;
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float ga = gamma[c], be = beta[c];
    long r1 = r0 + RNB_ROWS;
    if (r1 > M) r1 = M;
    for (long r = r0 + ty; r < r1; r += 4) {
      const float xh = (Y[r * ldy + c] - mean[r]) * rstd[r];
      const float g = rn_gate(dZ[r * lddz + c], xh, ga, be, relu);
      s1 += g;
      s2 = fmaf(g, xh, s2);
    }
  }
  red[0][ty][cl] = s1; red[1][ty][cl] = s2;
  __syncthreads();
  if (ty == 0 && c < C) {
    for (int t = 1; t < 4; ++t) { s1 += red[0][t][cl]; s2 += red[1][t][cl]; }
    float* o = part + ((long)blockIdx.y * C + c) * 2;
    o[0] = s1; o[1] = s2;
  }
}
__global__ void __launch_bounds__(64) k_rn_bwd_finalize(const float* part, long nb, int C, float* dgamma, float* dbeta,
                                                        int accumulate) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (long i = 0; i < nb; ++i) {
    const float* t = part + (i * C + c) * 2;
    a += (double)t[0]; b += (double)t[1];
  }
  float dg = (float)b, dbt = (float)a;
  if (accumulate) { dg += dgamma[c]; dbt += dbeta[c]; }
  dgamma[c] = dg; dbeta[c] = dbt;
}
template <bool REG>
__global__ void __launch_bounds__(256) k_rn_bwd_rows(const float* dZ, long lddz, const float* Y, long ldy, long M, int C,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                     float* dY, long lddy) {
  const int lane = threadIdx.x & 63;
  const float inv_c = 1.f / (float)C;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < M; r += (long)gridDim.x * 4) {
    const float* y = Y + r * ldy;
    const float* dz = dZ + r * lddz;
    float* dy = dY + r * lddy;
    const float mu = mean[r], is = rstd[r];
    float gg[REG ? 16 : 1], xv[REG ? 16 : 1];
    float s1 = 0.f, s2 = 0.f;
    auto elem = [&](int c, float& g, float& xh) {
      xh = (y[c] - mu) * is;
      const float ga = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
      g = rn_gate(dz[c], xh, ga, be, relu) * ga;
    };
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        gg[i] = 0.f; xv[i] = 0.f;
        if (c < C) elem(c, gg[i], xv[i]);
        s1 += gg[i];
        s2 = fmaf(gg[i], xv[i], s2);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float g, xh;
        elem(c, g, xh);
        s1 += g;
        s2 = fmaf(g, xh, s2);
      }
    }
    const float m1 = rn_wave_sum(s1) * inv_c, m2 = rn_wave_sum(s2) * inv_c;
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < C) dy[c] = is * (gg[i] - m1 - xv[i] * m2);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float g, xh;
        elem(c, g, xh);
        dy[c] = is * (g - m1 - xh * m2);
      }
    }
  }
}

// ---- generic route: per-proposal maximum of a row range of the materialised, ReLU'd [rows, F] matrix, merged into the
// zero-filled pool by the integer atomicMax of the ReLU kernels (values >= 0: int order == float order).  One thread per
// column walks 16 rows and flushes once per run of equal proposal ids, so a row range may start and end anywhere.
__global__ void __launch_bounds__(256) k_rn_range_max(const float* __restrict__ Zr, long ldz, int rows, int F,
                                                      const int* __restrict__ node_seg, int P, float* pool, long ldpool) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= F) return;
  const int r0 = blockIdx.y * 16;
  int r1 = r0 + 16;
  if (r1 > rows) r1 = rows;
  int cur = 0, seg = node_seg[r0];
  for (int r = r0; r < r1; ++r) {
    const int s = node_seg[r];
    if (s != seg) {
      if (cur > 0 && seg >= 0 && seg < P) atomicMax(reinterpret_cast<int*>(pool + (long)seg * ldpool + c), cur);
      cur = 0; seg = s;
    }
    cur = yl_max(cur, __float_as_int(Zr[(long)r * ldz + c]));
  }
  if (cur > 0 && seg >= 0 && seg < P) atomicMax(reinterpret_cast<int*>(pool + (long)seg * ldpool + c), cur);
}

// ---- the fused eval kernel --------------------------------------------------------------------------------------------
// pool[p, :] = max over the rows of proposal p of relu(rownorm(A . W^T + b) gamma + beta); second problem of the launch
// (fusion_block_super, P rows): plain store of the same.  Built from the blocks of k_fusion_rows_x6 (fusion_x6.hip; the
// W-tile movers are the same text, fx_w_movers.inc): exact 3-way bf16 split and six products, A split once into registers
// and kept, W tiles double-buffered through LDS, run-length integer atomicMax epilogue.  The work split differs: a
// workgroup owns RN_ROWS WHOLE rows and walks all F / 64 column tiles, twice.
// The mean never appears.  The caller hands in the CENTRED weights Wc = W - (mean over the F outputs of W), bc = b - mean(b):
//   (A . Wc^T + bc)[r, c] = y[r, c] - mean_c(y[r, :])   algebraically, for every row,
// so an accumulator IS the deviation d, however far the row mean is from zero, and var = mean_c(d^2) is a centred sum.
//   sweep 1: sum of d^2 per row as per-lane partials in the accumulator layout (a lane holds 16 rows of one column),
//            added across the column tiles, reduced across the 32 lanes of a row once at the end -> rstd in the same 16 registers
//   sweep 2: the products again (W comes from L2 through LDS), d * rstd * gamma + beta, ReLU, pooling / store.
struct RnProb {
  const float* A; long lda; int N;
  const yl_bf16_t *Wh, *Wm, *Wl;
  const float* tcen;
  const float *gamma, *beta;
  const int* seg;
  float* out; long ldo;
  int tm;
};
constexpr int RN_T = 256, RN_ROWS = YOLAT_RN_ROWS;
static_assert(RN_ROWS == RN_T / 2, "32 rows per wave");

template <int KD>
__global__ void __launch_bounds__(RN_T) k_fusion_rows_rn(RnProb p0, RnProb p1, int F, float eps) {
  constexpr int T = RN_T, NWAVE = T / 64;
  constexpr int KS = KD / 16, RS = KD + 8, CPR = KD / 8;    // k steps, LDS row stride (bf16), 16-byte chunks per row
  constexpr int CHUNKS = 3 * 64 * CPR, NW = CHUNKS / T;     // 16-byte chunks of one W tile, per thread
  static_assert(CHUNKS % T == 0, "W tile / thread mismatch");
  constexpr int TK = 64, TS = TK + 4;                       // the prologue's transposition tile: [32 rows][TK + 4] floats per wave
  constexpr int SMEM_W = 2 * 3 * 64 * RS * 2, SMEM_T = NWAVE * 32 * TS * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM_W > SMEM_T ? SMEM_W : SMEM_T];
  yl_bf16_t (*Ws)[3 * 64 * RS] = reinterpret_cast<yl_bf16_t (*)[3 * 64 * RS]>(smem);
  const int tid = threadIdx.x;
  // the small problem's workgroups come first: they start with the first round instead of forming a tail
  const bool small = (int)blockIdx.x < p1.tm;
  const int rt = small ? (int)blockIdx.x : (int)blockIdx.x - p1.tm;
  const float* __restrict__ A = small ? p1.A : p0.A;
  const long lda = small ? p1.lda : p0.lda;
  const int N = small ? p1.N : p0.N;
  const float* tcen = small ? p1.tcen : p0.tcen;
  const float* gamma = small ? p1.gamma : p0.gamma;
  const float* beta = small ? p1.beta : p0.beta;
  const int* seg = small ? p1.seg : p0.seg;
  float* out = small ? p1.out : p0.out;
  const long ldo = small ? p1.ldo : p0.ldo;
  const int tn = F >> 6;                                    // F % 64 == 0

  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt * RN_ROWS + wave * 32;
  const int sv_pre = (seg != nullptr && row0 + l31 < N) ? seg[row0 + l31] : -1;
  const yl_bf16_t* const wparts[3] = {small ? p1.Wh : p0.Wh, small ? p1.Wm : p0.Wm, small ? p1.Wl : p0.Wl};
#define FX_W_CLAMP 0                                        // (F % 64 == 0)
#include "fx_w_movers.inc"
#undef FX_W_CLAMP
  fx_u32x4 rw[NW];
  load_w(0, rw);
  float t0 = tcen[l31], t1 = tcen[32 + l31];
  // ---- this wave's 32 rows of A, split once (k_fusion_rows_x6's prologue: row-wise loads, transposed through LDS)
  fx_bf16x8 Ah[KS], Am[KS], Al[KS];
  {
    float* Tt = reinterpret_cast<float*>(smem) + wave * (32 * TS);
    const int lr = lane >> 4, lc = (lane & 15) * 4;
#pragma unroll
    for (int q = 0; q < KD / TK; ++q) {
      float4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        v[i] = *reinterpret_cast<const float4*>(A + (long)yl_min(row0 + 4 * i + lr, N - 1) * lda + TK * q + lc);
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<float4*>(Tt + (4 * i + lr) * TS + lc) = v[i];
#pragma unroll
      for (int u = 0; u < TK / 16; ++u) {
        const int ks = (TK / 16) * q + u;
        const float4 a0 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi);
        const float4 a1 = *reinterpret_cast<const float4*>(Tt + l31 * TS + 16 * u + 8 * lhi + 4);
        const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        fx_split8(x, Ah[ks], Am[ks], Al[ks]);
      }
    }
  }
  const bool pooling = seg != nullptr;
  FxRuns runs;
  unsigned roff[16];                                    // element offset of each of the lane's rows' proposal in the pool
  fx_seg_runs_off(sv_pre, lhi, (unsigned)ldo, runs, roff);
  float q2[16];                                         // sweep 1: partial sums of d^2 of the lane's 16 rows; sweep 2: rstd
#pragma unroll
  for (int r = 0; r < 16; ++r) q2[r] = 0.f;
  __syncthreads();                                          // every wave is done with its transposition tile
  store_w(0, rw);
  __syncthreads();
  const float inv_f = 1.f / (float)F;
  for (int j = 0; j < 2 * tn; ++j) {
    const bool second = j >= tn;
    const int ct = second ? j - tn : j, buf = j & 1;
    const int c0 = ct * 64 + l31, c1 = c0 + 32;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = t0; acc1[r] = t1; }
    float g0 = 1.f, g1 = 1.f, b0 = 0.f, b1 = 0.f;
    if (second && gamma != nullptr) { g0 = gamma[c0]; g1 = gamma[c1]; b0 = beta[c0]; b1 = beta[c1]; }
    if (j + 1 < 2 * tn) {
      const int cn = ct + 1 == tn ? 0 : ct + 1;
      t0 = tcen[cn * 64 + l31];
      t1 = tcen[cn * 64 + 32 + l31];
      load_w(cn, rw);                                  // in flight while the MFMAs below run
    }
    const yl_bf16_t* wb = &Ws[buf][l31 * RS + 8 * lhi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fx_bf16x8 bf[6];                                 // [0] b0h [1] b1h [2] b0m [3] b1m [4] b0l [5] b1l
#pragma unroll
      for (int q = 0; q < 6; ++q) bf[q] = *reinterpret_cast<const fx_bf16x8*>(wb + q * 32 * RS + 16 * ks);
      // small terms first; the empty asm pins the MFMAs' program order (fusion_x6.hip).  Its operands are constrained to
      // ACCUMULATION registers: at one wave per SIMD the compiler keeps the accumulators there anyway, and a "+v" made it
      // copy all 32 to vector registers and back around every MFMA (3090 v_accvgpr moves per column tile, 313 us at cfg 2)
#define RN_MFMA(acc, a, b)                                          \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); \
  asm volatile("" : "+a"(acc0), "+a"(acc1))
      RN_MFMA(acc0, Al[ks], bf[0]);
      RN_MFMA(acc1, Al[ks], bf[1]);
      RN_MFMA(acc0, Ah[ks], bf[4]);
      RN_MFMA(acc1, Ah[ks], bf[5]);
      RN_MFMA(acc0, Am[ks], bf[2]);
      RN_MFMA(acc1, Am[ks], bf[3]);
      RN_MFMA(acc0, Am[ks], bf[0]);
      RN_MFMA(acc1, Am[ks], bf[1]);
      RN_MFMA(acc0, Ah[ks], bf[2]);
      RN_MFMA(acc1, Ah[ks], bf[3]);
      RN_MFMA(acc0, Ah[ks], bf[0]);
      RN_MFMA(acc1, Ah[ks], bf[1]);
#undef RN_MFMA
    }
    // next W tile into the other buffer (its readers finished before the last barrier) BEFORE the epilogue
    if (j + 1 < 2 * tn) store_w(buf ^ 1, rw);
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): everything in flight was issued a whole MFMA phase ago
    if (!second) {
#pragma unroll
      for (int r = 0; r < 16; ++r) q2[r] = fmaf(acc0[r], acc0[r], fmaf(acc1[r], acc1[r], q2[r]));
      if (j == tn - 1) {
        // the 32 lanes of a half-wave hold the 32 columns of the same 16 rows: butterfly within the half
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s = q2[r];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
          q2[r] = 1.f / sqrtf(s * inv_f + eps);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc0[r] = fmaf(acc0[r] * q2[r], g0, b0);
        acc1[r] = fmaf(acc1[r] * q2[r], g1, b1);
      }
      if (pooling) {
        fx_segmax2_off(acc0, acc1, out, roff, (unsigned)c0, true, true, runs);
      } else {
        unsigned rb = (unsigned)(row0 + 4 * lhi);
        asm volatile("" : "+v"(rb));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned row = rb + (r & 3) + 8 * (r >> 2);
          if ((int)row < N) {
            float* o = out + (unsigned long)row * (unsigned long)ldo;
            o[c0] = fmaxf(acc0[r], 0.f);
            o[c1] = fmaxf(acc1[r], 0.f);
          }
        }
      }
    }
    __syncthreads();
  }
}
}  // namespace

// ---- host side --------------------------------------------------------------------------------------------------------
extern "C" int yolat_rownorm_act(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* gamma, const float* beta,
                                 float eps, int relu, float* Z, int64_t ldz, float* save_mean, float* save_rstd,
                                 yolat_stream_t stream) {
  if (M < 0 || C <= 0 || C >= (1LL << 31) || (gamma == nullptr) != (beta == nullptr) || !(eps >= 0.f) ||
      (M > 0 && (!Y || !Z)) || ldy < C || ldz < C)
    return YOLAT_E_INVALID;
  if (M == 0) return 0;
  int gx = yl_cdiv(M, 4);
  if (gx > 65536) gx = 65536;
  if (C <= 1024)
    hipLaunchKernelGGL(k_rownorm_act<true>, dim3(gx), dim3(256), 0, (hipStream_t)stream, Y, (long)ldy, (long)M, (int)C, gamma,
                       beta, eps, relu, Z, (long)ldz, save_mean, save_rstd);
  else
    hipLaunchKernelGGL(k_rownorm_act<false>, dim3(gx), dim3(256), 0, (hipStream_t)stream, Y, (long)ldy, (long)M, (int)C, gamma,
                       beta, eps, relu, Z, (long)ldz, save_mean, save_rstd);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t yolat_rownorm_act_bwd_work_elems(int64_t M, int64_t C) {
  if (M <= 0 || C <= 0) return 0;
  return (size_t)(2 * (long)yl_cdiv(M, RNB_ROWS) * C);
}

extern "C" int yolat_rownorm_act_bwd(const float* dZ, int64_t lddz, const float* Y, int64_t ldy, int64_t M, int64_t C,
                                     const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                     int relu, float* dgamma, float* dbeta, int accumulate, float* dY, int64_t lddy,
                                     float* work, yolat_stream_t stream) {
  if (M <= 0 || C <= 0 || C >= (1LL << 31) || !dZ || !Y || !save_mean || !save_rstd || !dY || lddz < C || ldy < C || lddy < C ||
      (gamma == nullptr) != (beta == nullptr))
    return YOLAT_E_INVALID;
  if (gamma != nullptr && (!dgamma || !dbeta || !work)) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (gamma != nullptr) {
    const long nb = yl_cdiv(M, RNB_ROWS);
    hipLaunchKernelGGL(k_rn_bwd_partial, dim3(yl_cdiv(C, 64), (unsigned)nb), dim3(256), 0, st, dZ, (long)lddz, Y, (long)ldy,
                       (long)M, (int)C, save_mean, save_rstd, gamma, beta, relu, work);
    YL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rn_bwd_finalize, dim3(yl_cdiv(C, 64)), dim3(64), 0, st, work, nb, (int)C, dgamma, dbeta, accumulate);
    YL_LAUNCH_CHECK();
  }
  int gx = yl_cdiv(M, 4);
  if (gx > 65536) gx = 65536;
  if (C <= 1024)
    hipLaunchKernelGGL(k_rn_bwd_rows<true>, dim3(gx), dim3(256), 0, st, dZ, (long)lddz, Y, (long)ldy, (long)M, (int)C, save_mean,
                       save_rstd, gamma, beta, relu, dY, (long)lddy);
  else
    hipLaunchKernelGGL(k_rn_bwd_rows<false>, dim3(gx), dim3(256), 0, st, dZ, (long)lddz, Y, (long)ldy, (long)M, (int)C, save_mean,
                       save_rstd, gamma, beta, relu, dY, (long)lddy);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_fusion_pair_eval_x6_rn(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh,
                                            const uint16_t* Wm, const uint16_t* Wl, const float* tcen, int64_t F,
                                            const float* gamma_f, const float* beta_f, const int32_t* node_seg, float* pool,
                                            int64_t ldpool, const float* S, int64_t lds, int64_t P, const uint16_t* Wsh,
                                            const uint16_t* Wsm, const uint16_t* Wsl, const float* tscen,
                                            const float* gamma_s, const float* beta_s, float* Ys, int64_t ldys, float eps,
                                            yolat_stream_t stream) {
  if (N <= 0 || P <= 0 || F <= 0 || !A || !Wh || !Wm || !Wl || !tcen || !node_seg || !pool || !S || !Wsh || !Wsm || !Wsl ||
      !tscen || !Ys || !(eps >= 0.f))
    return YOLAT_E_INVALID;
  if ((gamma_f == nullptr) != (beta_f == nullptr) || (gamma_s == nullptr) != (beta_s == nullptr)) return YOLAT_E_INVALID;
  if (lda < D || lds < D || ldpool < F || ldys < F) return YOLAT_E_INVALID;
  if ((D != 64 && D != 128) || F % 64 != 0) return YOLAT_E_UNSUPPORTED;
  if (lda % 4 != 0 || lds % 4 != 0 || !yl_aligned16(A) || !yl_aligned16(S) || !yl_aligned16(Wh) || !yl_aligned16(Wm) ||
      !yl_aligned16(Wl) || !yl_aligned16(Wsh) || !yl_aligned16(Wsm) || !yl_aligned16(Wsl))
    return YOLAT_E_UNSUPPORTED;
  // 32-bit element offsets into the pool (segmax.hpp) and 31-bit row / weight indices
  if ((long)P * ldpool >= (1LL << 32) || N >= (1LL << 31) - 2 * RN_ROWS || F * D >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
  RnProb p0{}, p1{};
  p0.A = A; p0.lda = lda; p0.N = (int)N; p0.Wh = Wh; p0.Wm = Wm; p0.Wl = Wl; p0.tcen = tcen; p0.gamma = gamma_f;
  p0.beta = beta_f; p0.seg = node_seg; p0.out = pool; p0.ldo = ldpool; p0.tm = yl_cdiv(N, RN_ROWS);
  p1.A = S; p1.lda = lds; p1.N = (int)P; p1.Wh = Wsh; p1.Wm = Wsm; p1.Wl = Wsl; p1.tcen = tscen; p1.gamma = gamma_s;
  p1.beta = beta_s; p1.seg = nullptr; p1.out = Ys; p1.ldo = ldys; p1.tm = yl_cdiv(P, RN_ROWS);
  const long total = (long)p0.tm + p1.tm;
  hipStream_t st = (hipStream_t)stream;
  if (D == 128) hipLaunchKernelGGL(k_fusion_rows_rn<128>, dim3((unsigned)total), dim3(RN_T), 0, st, p0, p1, (int)F, eps);
  else hipLaunchKernelGGL(k_fusion_rows_rn<64>, dim3((unsigned)total), dim3(RN_T), 0, st, p0, p1, (int)F, eps);
  YL_LAUNCH_CHECK();
  return 0;
}

bool yl_rn_fused(const yolat_model_eval* m, int64_t N) {
  if (m->rn_route == YOLAT_RN_ROUTE_FUSED) return true;
  if (m->rn_route == YOLAT_RN_ROUTE_MATERIALISE) return false;
  return N >= YOLAT_RN_FUSED_MIN_ROWS;
}

// rows of the fusion block materialised per pass: the [rows, F] matrix is the only scratch, kept <= 64 MiB
static long rn_chunk_rows(long N, long F) {
  long rc = (16L << 20) / (F > 0 ? F : 1);
  if (rc < 16) rc = 16;
  if (rc > (1L << 19)) rc = 1L << 19;                         // (k_rn_range_max: 16 rows per grid row)
  return rc < N ? rc : N;
}

extern "C" size_t yolat_fusion_pair_eval_rn_work_elems(int64_t N, int64_t F) {
  if (N <= 0 || F <= 0) return 0;
  return (size_t)rn_chunk_rows(N, F) * (size_t)F;
}

extern "C" int yolat_fusion_pair_eval_rn(const float* A, int64_t lda, int64_t N, int64_t D, const float* Wf, const float* bf,
                                         int64_t F, const float* gamma_f, const float* beta_f, const int32_t* node_seg,
                                         float* pool, int64_t ldpool, const float* S, int64_t lds, int64_t P,
                                         const float* Wfs, const float* bfs, const float* gamma_s, const float* beta_s,
                                         float* Ys, int64_t ldys, float eps, float* work, yolat_stream_t stream) {
  if (N <= 0 || D <= 0 || F <= 0 || P <= 0 || N >= (1LL << 31) || F >= (1LL << 31) || P >= (1LL << 31) || !A || !Wf || !node_seg || !pool ||
      !work || ldpool < F || lda < D || !(eps >= 0.f))
    return YOLAT_E_INVALID;
  if ((gamma_f == nullptr) != (beta_f == nullptr) || (gamma_s == nullptr) != (beta_s == nullptr)) return YOLAT_E_INVALID;
  if (S != nullptr && (!Wfs || !Ys || ldys < F || lds < D)) return YOLAT_E_INVALID;      // (everything before the first launch)
  const long rc = rn_chunk_rows(N, F);
  for (long r0 = 0; r0 < N; r0 += rc) {
    const long n = N - r0 < rc ? N - r0 : rc;
    YL_TRY(yolat_linear_fwd(A + r0 * lda, lda, n, D, nullptr, nullptr, 0, Wf, D, bf, F, nullptr, nullptr, 0, work, F, 0,
                            nullptr, stream));
    YL_TRY(yolat_rownorm_act(work, F, n, F, gamma_f, beta_f, eps, 1, work, F, nullptr, nullptr, stream));
    hipLaunchKernelGGL(k_rn_range_max, dim3(yl_cdiv(F, 256), yl_cdiv(n, 16)), dim3(256), 0, (hipStream_t)stream, work, (long)F,
                       (int)n, (int)F, node_seg + r0, (int)P, pool, (long)ldpool);
    YL_LAUNCH_CHECK();
  }
  if (S != nullptr) {
    YL_TRY(yolat_linear_fwd(S, lds, P, D, nullptr, nullptr, 0, Wfs, D, bfs, F, nullptr, nullptr, 0, Ys, ldys, 0, nullptr,
                            stream));
    YL_TRY(yolat_rownorm_act(Ys, ldys, P, F, gamma_s, beta_s, eps, 1, Ys, ldys, nullptr, nullptr, stream));
  }
  return 0;
}

// the range maximum of the generic route for a caller in another file (bf16_eval.hip: the bf16 forward's materialising route):
// rows <= 2^20 rows of the ReLU'd Zr [rows, ldz] with their proposal ids, merged into the zero-started pool
int yl_rn_range_max(const float* Zr, int64_t ldz, int64_t rows, int64_t F, const int32_t* node_seg, int64_t P, float* pool,
                    int64_t ldpool, hipStream_t st) {
  if (!Zr || !node_seg || !pool || rows <= 0 || rows > (1LL << 20) || F <= 0 || F >= (1LL << 31) || P <= 0 || P >= (1LL << 31) ||
      ldz < F || ldpool < F)
    return YOLAT_E_INVALID;
  hipLaunchKernelGGL(k_rn_range_max, dim3(yl_cdiv(F, 256), yl_cdiv(rows, 16)), dim3(256), 0, st, Zr, (long)ldz, (int)rows, (int)F,
                     node_seg, (int)P, pool, (long)ldpool);
  YL_LAUNCH_CHECK();
  return 0;
}
