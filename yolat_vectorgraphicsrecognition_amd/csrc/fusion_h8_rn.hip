// fusion_h8_rn.hip — the bf16-storage eval forward behind a ROW norm (--norm layer / instance; rownorm.hip has the fp32 side):
//   k_hfusion_rows8_rn   fusion block + row norm + ReLU + per-proposal max, and fusion_block_super + row norm + ReLU, as ONE
//                        launch; the [N, F] matrix is never written
//   k_rownorm_act_h      the classifier's row norm: fp32 rows in, the normalised ReLU'd row out as bf16 with one rounding
// The fused kernel is the data flow of k_hfusion_rows8 (fusion_h8.hip) with the two sweeps of k_fusion_rows_rn (rownorm.hip):
// a 512-thread workgroup owns 256 WHOLE rows and all F / 64 column tiles (a row's statistics need every column, so there
// are no column groups); every wave keeps its 32 rows x K of A as bf16 MFMA fragments in registers; the weights stream
// through a double-buffered LDS tile, the next tile's pieces in registers while the current tile's MFMAs run.
// The caller hands in the CENTRED weights Wc = W - mean over the F outputs (taken in float64, then rounded to bf16) and the
// centred bias bc (fp32), so an accumulator is the deviation d = y - mean_c(y), however far the row mean is from zero, up
// to the rounding of Wc.  That rounding leaves a residual row mean m — bounded by 2^-9 |a| . mean_c |Wc|, ~1e-2 of the row's standard
// deviation in the worst case, ~1e-4 of it typically — which is no longer the pure fp32 rounding it is in the fp32 kernel.
// Sweep 1 therefore carries sum(d) next to sum(d^2) (16 more registers; it keeps the kernel within the fp32 envelope of
// tests/bf16_rownorm_ref.py, which subtracts the true mean): var = mean(d^2) - m^2, a subtraction that cancels nothing
// because m^2 <= 1e-4 var by construction — NOT the E[y^2] - mean^2 of an un-centred row.
//   sweep 1: per-lane partial sums of d and d^2 in the accumulator layout (a lane holds 16 rows of one column), added across
//            the column tiles, one butterfly each over the half-wave at the end -> rstd and -m rstd in the same 32 registers
//   sweep 2: W again (L2 resident), d again, (d rstd - m rstd) * gamma + beta, ReLU, then the unsigned LDS pooling table
//            of segmax.hpp (values >= 0: the pooled matrix starts from zeros) / the plain store of the super block.
#include "segmax.hpp"
#include "internal.hpp"

typedef unsigned short u16;
typedef unsigned h8r_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 h8r_bf16x8 __attribute__((ext_vector_type(8)));

namespace {
struct H8RnProb {
  const u16* Ah;        // bf16 rows (NULL -> Af)
  const float* Af;      // fp32 rows, converted while loading
  long lda; int N;
  const u16* W;         // [F, KD] bf16, centred over the F outputs before the rounding
  const float* tcen;    // [F] centred bias
  const float *gamma, *beta;   // [F], both NULL for the instance norm
  const int* seg;       // != NULL: pooling epilogue into out (pooled matrix); else out[row, col] = relu(.)
  float* out; long ldo;
  int tm;               // row tiles of 256
};

template <int KD>
__global__ void __launch_bounds__(512, 2) k_hfusion_rows8_rn(H8RnProb p0, H8RnProb p1, int F, float eps) {
  constexpr int KS = KD / 16, RS = KD + 8, CPR = KD / 8;    // k steps, LDS row stride (bf16), 16-byte chunks per row
  constexpr int NW = 64 * CPR / 512;                        // 16-byte pieces of one W tile per thread
  static_assert((64 * CPR) % 512 == 0, "W tile / thread mismatch");
  __shared__ __attribute__((aligned(16))) u16 Ws[2][64 * RS];
  __shared__ int seg_s[256];
  __shared__ int tab_s[2][FX_NP * 64];                     // per-column-tile pooled maxima of the workgroup (segmax.hpp)
  const int tid = threadIdx.x;
  // the small problem's workgroups come first: they start with the first round instead of forming a tail
  const bool small = (int)blockIdx.x < p1.tm;
  const int rt = small ? (int)blockIdx.x : (int)blockIdx.x - p1.tm;
  const u16* const Ah = small ? p1.Ah : p0.Ah;
  const float* const Af = small ? p1.Af : p0.Af;
  const long lda = small ? p1.lda : p0.lda;
  const int N = small ? p1.N : p0.N;
  const u16* const W = small ? p1.W : p0.W;
  const float* const tcen = small ? p1.tcen : p0.tcen;
  const float* const gamma = small ? p1.gamma : p0.gamma;
  const float* const beta = small ? p1.beta : p0.beta;
  const int* const seg = small ? p1.seg : p0.seg;
  float* const out = small ? p1.out : p0.out;
  const long ldo = small ? p1.ldo : p0.ldo;
  const int tn = F >> 6;                                    // F % 64 == 0

  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt * 256 + wave * 32;
  // ---- this wave's 32 rows of A as MFMA A fragments (lane = row, 8 consecutive k per lane half); rows >= N are clamped
  h8r_bf16x8 Afr[KS];
  {
    const long r = yl_min(row0 + l31, N - 1);
    if (Ah != nullptr) {
      const u16* ap = Ah + r * lda + 8 * lhi;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) Afr[ks] = __builtin_bit_cast(h8r_bf16x8, *reinterpret_cast<const h8r_u32x4*>(ap + 16 * ks));
    } else {
      const float* ap = Af + r * lda + 8 * lhi;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const float4 a0 = *reinterpret_cast<const float4*>(ap + 16 * ks), a1 = *reinterpret_cast<const float4*>(ap + 16 * ks + 4);
        const h8r_u32x4 v = {yl_pack_bf16(a0.x, a0.y), yl_pack_bf16(a0.z, a0.w), yl_pack_bf16(a1.x, a1.y),
                             yl_pack_bf16(a1.z, a1.w)};
        Afr[ks] = __builtin_bit_cast(h8r_bf16x8, v);
      }
    }
  }
  const bool pooling = seg != nullptr;
  FxTile tile{};
  if (pooling) {
    const int row_lo = rt * 256, row_hi = yl_min(row_lo + 256, N);
    tile = fx_tile(seg, row_lo, row_hi, N);
    for (int e = tid; e < 2 * FX_NP * 64; e += 512) (&tab_s[0][0])[e] = 0;
  }
  FxRuns runs;
  {
    const int sv = (pooling && row0 + l31 < N) ? seg[row0 + l31] : -1;
    if (lhi == 0) seg_s[wave * 32 + l31] = sv;          // read back by the same wave only, after the barrier below
    fx_seg_runs(sv, lhi, runs);
  }
  const int* segs = seg_s + wave * 32;
  const unsigned wr0 = (unsigned)tid / CPR, wk = ((unsigned)tid % CPR) * 8;   // row (of the first piece), k offset
  auto load_w = [&](int ct, h8r_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const unsigned r = wr0 + (unsigned)t * (512 / CPR);
      rw[t] = *reinterpret_cast<const h8r_u32x4*>(W + ((unsigned)ct * 64 + r) * KD + wk);
    }
  };
  auto store_w = [&](int buf, const h8r_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const unsigned r = wr0 + (unsigned)t * (512 / CPR);
      *reinterpret_cast<h8r_u32x4*>(&Ws[buf][r * RS + wk]) = rw[t];
    }
  };
  h8r_u32x4 rw[NW];
  load_w(0, rw);
  float t0 = tcen[l31], t1 = tcen[32 + l31];
  float q2[16], sm[16];                                 // sweep 1: partial sums of d^2 / d of the lane's 16 rows;
#pragma unroll                                          // sweep 2: rstd / -mean * rstd
  for (int r = 0; r < 16; ++r) { q2[r] = 0.f; sm[r] = 0.f; }
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
    // the previous column tile's pooled maxima (complete since its closing barrier) go out while this tile's MFMAs run
    if (pooling && j > tn) fx_tab_drain(tab_s[buf ^ 1], tile, out, (unsigned)ldo, ct - 1, F, tid, 512);
    const u16* wb = &Ws[buf][l31 * RS + 8 * lhi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const h8r_bf16x8 w0 = *reinterpret_cast<const h8r_bf16x8*>(wb + 16 * ks);
      const h8r_bf16x8 w1 = *reinterpret_cast<const h8r_bf16x8*>(wb + 32 * RS + 16 * ks);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Afr[ks], w0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Afr[ks], w1, acc1, 0, 0, 0);
    }
    // next W tile into the other buffer (its readers finished before the last barrier) BEFORE the epilogue
    if (j + 1 < 2 * tn) store_w(buf ^ 1, rw);
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
    if (!second) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        q2[r] = fmaf(acc0[r], acc0[r], fmaf(acc1[r], acc1[r], q2[r]));
        sm[r] += acc0[r] + acc1[r];
      }
      if (j == tn - 1) {
        // the 32 lanes of a half-wave hold the 32 columns of the same 16 rows: butterfly within the half
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s = q2[r], m = sm[r];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) { s += __shfl_xor(s, o); m += __shfl_xor(m, o); }
          m *= inv_f;
          const float rstd = 1.f / sqrtf(fmaxf(fmaf(-m, m, s * inv_f), 0.f) + eps);
          q2[r] = rstd;
          sm[r] = -m * rstd;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc0[r] = fmaf(fmaf(acc0[r], q2[r], sm[r]), g0, b0);
        acc1[r] = fmaf(fmaf(acc1[r], q2[r], sm[r]), g1, b1);
      }
      if (pooling) {
        fx_segmax2_lds(acc0, acc1, tab_s[buf], out, (unsigned)ldo, segs, tile.seg_base, lhi, (unsigned)c0, (unsigned)l31, true,
                       true, runs);
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
  if (pooling) fx_tab_drain(tab_s[(2 * tn - 1) & 1], tile, out, (unsigned)ldo, tn - 1, F, tid, 512);
}

__device__ __forceinline__ float rnh_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;                                                   // (a butterfly: every lane holds the same bits)
}

// ---- Z (bf16) = relu(rownorm(Y) * gamma + beta): the arithmetic of k_rownorm_act (rownorm.hip) — one wave per row, 4 rows
// per workgroup, centred on the row's first element, variance as a mean of centred squares — with the result rounded to
// bf16 once (round to nearest even).  REG: the row lives in registers (C <= 1024); else it is re-read per pass.  Z is a
// buffer of its own: a bf16 row r written in place would overlap fp32 row r / 2, which belongs to another wave.
template <bool REG>
__global__ void __launch_bounds__(256) k_rownorm_act_h(const float* __restrict__ Y, long ldy, long M, int C,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float eps, u16* __restrict__ Z, long ldz) {
  const int lane = threadIdx.x & 63;
  const float inv_c = 1.f / (float)C;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < M; r += (long)gridDim.x * 4) {
    const float* y = Y + r * ldy;
    u16* z = Z + r * ldz;
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
    const float ms = rnh_wave_sum(s) * inv_c;                 // mean - y0
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
    const float rstd = 1.f / sqrtf(rnh_wave_sum(q) * inv_c + eps);
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
          float o = v[i] * rstd;
          if (gamma) o = fmaf(o, gamma[c], beta[c]);
          z[c] = (u16)(yl_pack_bf16(fmaxf(o, 0.f), 0.f) & 0xFFFFu);
        }
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float o = ((y[c] - y0) - ms) * rstd;
        if (gamma) o = fmaf(o, gamma[c], beta[c]);
        z[c] = (u16)(yl_pack_bf16(fmaxf(o, 0.f), 0.f) & 0xFFFFu);
      }
    }
  }
}
}  // namespace

int yl_rownorm_act_h(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* gamma, const float* beta, float eps,
                     uint16_t* Z, int64_t ldz, hipStream_t st) {
  if (M <= 0 || C <= 0 || C >= (1LL << 31) || (gamma == nullptr) != (beta == nullptr) || !(eps >= 0.f) || !Y || !Z || ldy < C ||
      ldz < C)
    return YOLAT_E_INVALID;
  // the two buffers must not overlap: a wave writes its row while other waves still read theirs
  const uintptr_t y0 = (uintptr_t)Y, y1 = y0 + (size_t)((M - 1) * ldy + C) * 4, z0 = (uintptr_t)Z,
                  z1 = z0 + (size_t)((M - 1) * ldz + C) * 2;
  if (y0 < z1 && z0 < y1) return YOLAT_E_INVALID;
  int gx = yl_cdiv(M, 4);
  if (gx > 65536) gx = 65536;
  if (C <= 1024)
    hipLaunchKernelGGL(k_rownorm_act_h<true>, dim3(gx), dim3(256), 0, st, Y, (long)ldy, (long)M, (int)C, gamma, beta, eps, Z,
                       (long)ldz);
  else
    hipLaunchKernelGGL(k_rownorm_act_h<false>, dim3(gx), dim3(256), 0, st, Y, (long)ldy, (long)M, (int)C, gamma, beta, eps, Z,
                       (long)ldz);
  YL_LAUNCH_CHECK();
  return 0;
}

// what yl_hfusion_rows8_rn declines, before anything is written (the forward's descriptor check asks the same question)
bool yl_hfusion_rows8_rn_ok(const void* A, int64_t lda, int64_t N, int64_t D, const void* Wf, int64_t F, const void* As,
                            int64_t lda_s, int64_t P, const void* Wfs) {
  if ((D != 64 && D != 128) || F <= 0 || F % 64 != 0 || N <= 0 || P <= 0) return false;
  if (!yl_aligned16(A) || !yl_aligned16(As) || !yl_aligned16(Wf) || !yl_aligned16(Wfs) || lda % 8 != 0 || lda_s % 4 != 0)
    return false;
  // 31-bit row indices (a row tile may reach 255 rows past N) and 32-bit weight offsets
  return N < (1LL << 31) - 512 && P < (1LL << 31) - 512 && F * D < (1LL << 31);
}

// A [N, lda] bf16 x Wf [F, D] (centred, bf16) -> row norm -> relu -> per-proposal max into pool [*, ld_pool] (columns 0..F,
// zero before the launch), and As [P, lda_s] fp32 x Wfs [F, D] -> row norm -> relu -> sup_out [P, ld_sup].  D in {64, 128};
// F % 64 == 0; P * ld_pool < 2^32 is the caller's (32-bit element offsets into the pooled matrix).
int yl_hfusion_rows8_rn(const uint16_t* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wf, const float* tf,
                        const float* gamma_f, const float* beta_f, const int32_t* seg, float* pool, int64_t ld_pool, int64_t F,
                        const float* As, int64_t lda_s, int64_t P, const uint16_t* Wfs, const float* tfs, const float* gamma_s,
                        const float* beta_s, float* sup_out, int64_t ld_sup, float eps, hipStream_t st) {
  if (!A || !Wf || !tf || !seg || !pool || !As || !Wfs || !tfs || !sup_out || !(eps >= 0.f)) return YOLAT_E_INVALID;
  if ((gamma_f == nullptr) != (beta_f == nullptr) || (gamma_s == nullptr) != (beta_s == nullptr)) return YOLAT_E_INVALID;
  if (!yl_hfusion_rows8_rn_ok(A, lda, N, D, Wf, F, As, lda_s, P, Wfs)) return YOLAT_E_UNSUPPORTED;
  if (lda < D || lda_s < D || ld_pool < F || ld_sup < F) return YOLAT_E_INVALID;
  H8RnProb p0{}, p1{};
  p0.Ah = A; p0.Af = nullptr; p0.lda = lda; p0.N = (int)N; p0.W = Wf; p0.tcen = tf; p0.gamma = gamma_f; p0.beta = beta_f;
  p0.seg = seg; p0.out = pool; p0.ldo = ld_pool; p0.tm = yl_cdiv(N, 256);
  p1.Ah = nullptr; p1.Af = As; p1.lda = lda_s; p1.N = (int)P; p1.W = Wfs; p1.tcen = tfs; p1.gamma = gamma_s; p1.beta = beta_s;
  p1.seg = nullptr; p1.out = sup_out; p1.ldo = ld_sup; p1.tm = yl_cdiv(P, 256);
  const long total = (long)p0.tm + p1.tm;
  if (D == 128) hipLaunchKernelGGL(k_hfusion_rows8_rn<128>, dim3((unsigned)total), dim3(512), 0, st, p0, p1, (int)F, eps);
  else hipLaunchKernelGGL(k_hfusion_rows8_rn<64>, dim3((unsigned)total), dim3(512), 0, st, p0, p1, (int)F, eps);
  YL_LAUNCH_CHECK();
  return 0;
}
