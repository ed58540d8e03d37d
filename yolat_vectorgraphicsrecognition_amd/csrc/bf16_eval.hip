// bf16_eval.hip — SparseCADGCN.forward (eval) with bfloat16 STORAGE and fp32 accumulation: the precision mode
// BASELINE.json's large-graph configuration names (N = 200k / E = 1.2M / n_blocks = 4, "bf16").
//
// Same kernel sequence as forward_eval.hip (cad_recognition/architecture3cc_rpn_gp_iter2.py:44-71,106-137;
// gcn_lib/sparse/torch_vertex.py:319-337), with
//   * every [N,*] activation that crosses HBM stored as bf16: the per-node U|V products the edge kernel
//     gathers (256 -> 128 B per row), the layer outputs / concat slots, the node branch;
//   * every Linear with K >= 64 on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate), weights converted to
//     bf16 once per weight version, accumulators / bias / folded BatchNorm / ReLU / mean / max in fp32;
//   * the first layer's K = Cin0 = 5 products, the e_attr term (W1c.attr), the per-proposal pooled matrix Z
//     and the classifier activations stay fp32 (small or precision-critical).
// Rounding to bf16 is round-to-nearest-even (v_cvt_pk_bf16_f32).  Parity target: <= 1e-2 of the logits'
// scale against the fp32 oracle (SURVEY.md §8c "bf16 variant"); the fp32 path keeps the 1e-4 bar.
//
// Here: the fusion kernels, the node side of a conv layer > 0, the pooling prologue, the forward with its four entry points
// and the dense stages as ops.  The tile GEMM is hgemm.hpp (every k_hgemm instance of the library is instantiated HERE:
// yl_launch_hgemm serves bf16_linear.hip); edge stage: edge_chain.hip, rows8 fusion: fusion_h8.hip, conv stack: conv_local.hip.
// A row-norm base (--norm layer / instance, opted in by YOLAT_RN_ROUTE_BF16): the fusion pair and the classifier's two hidden
// layers take the branches of fusion_stage_rn / the forward's classifier block; kernels: fusion_h8_rn.hip, rownorm.hip.
#include "hgemm.hpp"
#include "gemm_nt.hpp"
#include "internal.hpp"
#include <stdlib.h>
#include <atomic>

// ------------------------------------------------------------------------------------------------
// fp32 -> bf16 (weights, once per weight version)
// ------------------------------------------------------------------------------------------------
static __global__ void k_f32_to_bf16(const float* __restrict__ src, long n, u16* __restrict__ dst) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (i + 1 < n) *reinterpret_cast<unsigned*>(dst + i) = yl_pack_bf16(src[i], src[i + 1]);
  else if (i < n) dst[i] = (u16)(yl_pack_bf16(src[i], 0.f) & 0xFFFFu);
}

extern "C" int yolat_f32_to_bf16(const float* src, int64_t n, uint16_t* dst, yolat_stream_t stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) return YOLAT_E_INVALID;
  if (n == 0) return 0;
  if ((((uintptr_t)dst) & 3) != 0) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_f32_to_bf16, dim3(yl_cdiv((n + 1) / 2, 256)), dim3(256), 0, (hipStream_t)stream, src, (long)n, dst);
  YL_LAUNCH_CHECK();
  return 0;
}

// fusion block over the nodes (+ per-proposal max epilogue) and fusion_block_super over the per-proposal
// means in one flattened launch, like k_gemm_nt_two: the small problem's 64x64 tiles come first (padded to a
// multiple of 8 so that the big problem keeps its id % 8 = XCD alignment), then the big problem's tiles.
template <int T0>
static __global__ void __launch_bounds__(256) k_hgemm_two(HOp A0, HOp B0, Epilogue e0, int M0, int N0, int K0, int tm0,
                                                          int tn0, FOp A1, HOp B1, Epilogue e1, int M1, int N1, int K1,
                                                          int tm1, int tn1) {
  __shared__ __attribute__((aligned(16))) u16 smem[HTileSmem<T0, T0>::elems];
  const int n1 = tm1 * tn1, n1p = (n1 + 7) & ~7;
  const int id = blockIdx.x;
  if (id < n1p) {
    if (id < n1) hgemm_tile<1, 1, FOp>(A1, B1, e1, M1, N1, K1, id / tn1, id % tn1, smem);
    return;
  }
  const int n0 = tm0 * tn0, j = id - n1p;
  const int chunk = n0 >> 3, rem = n0 & 7;
  const int xcd = j & 7, slot = j >> 3;
  const int logical = xcd * chunk + (xcd < rem ? xcd : rem) + slot;
  hgemm_tile<T0, T0, HOp>(A0, B0, e0, M0, N0, K0, logical / tn0, logical % tn0, smem);
}

// ------------------------------------------------------------------------------------------------
// A-resident GEMM for a SHORT K (the fusion block: K = 128, N = 1024): with one (row, column) tile per workgroup
// every tile is two dependent global->LDS round trips in front of 16 MFMAs — at N = 200k rows the launch was
// bound by that latency (211 us; 21 us of MFMA work).  Here a workgroup keeps its (64 TM) x K row tile of A in
// LDS and walks `ng` consecutive 64-column tiles of W: the NEXT tile's weights and epilogue constants are loaded
// into registers while the current tile's MFMAs and pooling epilogue run, so only the first round trip of a
// workgroup is exposed.  K <= KD (compile-time LDS extent); columns k >= K are zero-filled.
// ------------------------------------------------------------------------------------------------
// Run structure of a lane's 16 rows, derived ONCE per row tile from their segment ids (it is the same for every
// column and every column tile): keep[r] = 1 if row r continues the run of row r-1 else 0; off[r] = 32-bit element
// offset of the row's proposal in the pooled matrix; flush_bits bit r = a run of a valid segment ends at row r;
// uflush bit r = some lane of the wave flushes at r (wave-uniform: rows where nobody flushes cost no exec traffic).
struct SegRuns { float keep[16]; unsigned off[16]; unsigned flush_bits, uflush; };
__device__ __forceinline__ void yl_seg_runs(const int sgs[16], unsigned ldpool, SegRuns& sr) {
  unsigned fb = 0, uf = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    sr.keep[r] = (r > 0 && sgs[r] == sgs[r - 1]) ? 1.f : 0.f;
    sr.off[r] = (unsigned)(sgs[r] < 0 ? 0 : sgs[r]) * ldpool;
    const bool fl = sgs[r] >= 0 && (r == 15 || sgs[r] != sgs[r + 1]);
    fb |= fl ? (1u << r) : 0u;
    uf |= (__builtin_amdgcn_ballot_w64(fl) != 0ull) ? (1u << r) : 0u;
  }
  sr.flush_bits = fb; sr.uflush = uf;
}
// Pooling epilogue on that structure: per row one multiply (run reset: values are >= 0, so cur*0 restarts the max)
// and one 3-operand max (run max, activation, ReLU floor); the integer atomicMax (exact, order-independent) uses a
// 32-bit offset from a per-lane column pointer.  Same values as wave_epilogue_segmax's compare/select walk.
__device__ __forceinline__ void segmax_runs(const f32x16& acc, float* pool, unsigned col, bool col_ok, float sc,
                                            float sh, const SegRuns& sr) {
  float cur = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    cur = fmaxf(fmaxf(cur * sr.keep[r], fmaf(acc[r], sc, sh)), 0.f);
    if ((sr.uflush >> r) & 1u) {
      if (((sr.flush_bits >> r) & 1u) && col_ok && cur > 0.f)
        atomicMax(reinterpret_cast<int*>(pool) + (sr.off[r] + col), __float_as_int(cur));   // uniform base + 32-bit offset
    }
  }
}

template <int TM, int KD> struct HRowsSmem { static constexpr int elems = 64 * (TM + 1) * (KD + 8); };

template <int TM, int KD>
__device__ __forceinline__ void hgemm_rows(const HOp& A, const HOp& B, const Epilogue& ep, int M, int N, int K, int rt_,
                                           int ct0, int ng, u16* smem) {
  constexpr int BM = 64 * TM, RS = KD + 8, CPR = KD / 8;     // row stride (elements), 16-byte chunks per row
  constexpr int NA = TM * KD / 32, NW = KD / 32;            // chunks per thread: A tile, one 64-column W tile
  u16* As = smem;
  u16* Bs = smem + BM * RS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt_ * BM;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  auto load_w = [&](int ct, u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const int c = tid + 256 * t, r = c / CPR, kc = (c % CPR) * 8;
      const u32x4 v = *reinterpret_cast<const u32x4*>(B.p + (long)yl_min(ct * 64 + r, B.rows - 1) * B.ld + yl_min(kc, K - 8));
      rw[t] = kc < K ? v : zero4;
    }
  };
  u32x4 rw[NW];
  load_w(ct0, rw);
#pragma unroll
  for (int t = 0; t < NA; ++t) {
    const int c = tid + 256 * t, r = c / CPR, kc = (c % CPR) * 8;
    const u32x4 v = *reinterpret_cast<const u32x4*>(A.p + (long)yl_min(row0 + r, A.rows - 1) * A.ld + yl_min(kc, K - 8));
    *reinterpret_cast<u32x4*>(As + r * RS + kc) = kc < K ? v : zero4;
  }
  EpiPre pre[TM], nxt;
#pragma unroll
  for (int i = 0; i < TM; ++i) pre[i] = epi_prefetch(ep, row0 + (wm * TM + i) * 32, ct0 * 64 + wn * 32 + l31, M, N);
  nxt = pre[0];
  SegRuns runs[TM];                       // the rows' run structure is the same for every column tile
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int sgs[16];
    yl_tile_segs(pre[i].segv, lhi, sgs);
    yl_seg_runs(sgs, (unsigned)ep.ldpool, runs[i]);
  }
  for (int j = 0; j < ng; ++j) {
    const int ct = ct0 + j;
    __syncthreads();                      // the previous tile's fragment reads of Bs are done
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const int c = tid + 256 * t;
      *reinterpret_cast<u32x4*>(Bs + (c / CPR) * RS + (c % CPR) * 8) = rw[t];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TM; ++i) { pre[i].bias = nxt.bias; pre[i].sc = nxt.sc; pre[i].sh = nxt.sh; }
    if (j + 1 < ng) {                     // in flight while the MFMAs and the epilogue below run
      load_w(ct + 1, rw);
      nxt = epi_prefetch(ep, row0, (ct + 1) * 64 + wn * 32 + l31, M, N);
    }
    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KD / 16; ++ks) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (wn * 32 + l31) * RS + ks * 16 + lhi * 8);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + ((wm * TM + i) * 32 + l31) * RS + ks * 16 + lhi * 8);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i], 0, 0, 0);
      }
    }
    // pooling epilogue (this kernel exists for the fused per-proposal max): bias, folded BN + ReLU, run-length max
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      // (acc + bias)*sc + sh = acc*sc + (bias*sc + sh)
      const int colj = ct * 64 + wn * 32 + l31;
      segmax_runs(acc[i], ep.pool, (unsigned)colj, colj < N, pre[i].sc, fmaf(pre[i].bias, pre[i].sc, pre[i].sh), runs[i]);
    }
  }
}

// fusion block over the nodes (A-resident rows kernel, + per-proposal max epilogue) and fusion_block_super over the
// per-proposal means (plain 64x64 tiles, first and padded to a multiple of 8) in one flattened launch.  The big
// problem's workgroups are (row tile, column group) pairs, column group fastest, dealt to the XCDs in contiguous
// ranges so that the sharers of an A row tile hit one L2.
template <int TM, int KD>
static __global__ void __launch_bounds__(256) k_hfusion_rows(HOp A0, HOp B0, Epilogue e0, int M0, int N0, int K0, int tm0,
                                                             int groups, int ng, FOp A1, HOp B1, Epilogue e1, int M1,
                                                             int N1, int K1, int tm1, int tn1) {
  constexpr int SM = HRowsSmem<TM, KD>::elems > HTileSmem<1, 1>::elems ? HRowsSmem<TM, KD>::elems : HTileSmem<1, 1>::elems;
  __shared__ __attribute__((aligned(16))) u16 smem[SM];
  const int n1 = tm1 * tn1, n1p = (n1 + 7) & ~7;
  const int id = blockIdx.x;
  if (id < n1p) {
    if (id < n1) hgemm_tile<1, 1, FOp>(A1, B1, e1, M1, N1, K1, id / tn1, id % tn1, smem);
    return;
  }
  const int n0 = tm0 * groups, j = id - n1p;
  const int chunk = n0 >> 3, rem = n0 & 7;
  const int xcd = j & 7, slot = j >> 3;
  const int logical = xcd * chunk + (xcd < rem ? xcd : rem) + slot;
  const int rt = logical / groups, g = logical - rt * groups;
  const int tn = (N0 + 63) / 64;
  const int c0 = g * ng, cn = yl_min(ng, tn - c0);
  if (cn > 0) hgemm_rows<TM, KD>(A0, B0, e0, M0, N0, K0, rt, c0, cn, smem);
}

// node side of a factorised conv layer with Cin = 64 (bf16 in / bf16 weights):
//   y = 0,1 -> the two 64-column halves of UV = f_in.[W1a-W1b | W1b]^T   (stored bf16)
//   y = 2   -> root Linear lin_r(f_in) + br                               (stored fp32: the edge kernel adds the mean)
//   y = 3   -> node branch relu(bn(mlp_node(s_in)))                       (stored bf16)
struct NodeUvH {
  HOp af, as, wuv, wr, wn;
  Epilogue euv, er, en;
  int N, C, Cin;
};
__device__ __forceinline__ void hgemm_node3_body(const NodeUvH& a, u16* smem) {
  const int x = blockIdx.x, y = blockIdx.y;
  if (y < 2) hgemm_tile<1, 1, HOp>(a.af, a.wuv, a.euv, a.N, 2 * a.C, a.Cin, x, y, smem);
  else if (y == 2) hgemm_tile<1, 1, HOp>(a.af, a.wr, a.er, a.N, a.C, a.Cin, x, 0, smem);
  else hgemm_tile<1, 1, HOp>(a.as, a.wn, a.en, a.N, a.C, a.Cin, x, 0, smem);
}
static __global__ void __launch_bounds__(256) k_hgemm_node3(NodeUvH a) {
  __shared__ __attribute__((aligned(16))) u16 smem[HTileSmem<1, 1>::elems];
  hgemm_node3_body(a, smem);
}
// the same as the fall-back of the one-launch conv stack (conv_local.hip): dead unless the gate word holds its value.  (A
// persistent-grid form — a few hundred workgroups looping over the row tiles, so that the dead launch dispatches fewer
// workgroups — made the compiler keep 233 registers around the loop, or spill 140 under a bound: the live fall-back then
// ran at half speed; laundering the loop variable did not change that, and the tile as a real (noinline) call spilled
// 560 bytes per lane.  The full grid costs ~4 us per dead launch instead of ~2.)
static __global__ void __launch_bounds__(256) k_hgemm_node3_gated(NodeUvH a, YlGate gate) {
  __shared__ __attribute__((aligned(16))) u16 smem[HTileSmem<1, 1>::elems];
  if (yl_gate_dead(gate)) return;
  hgemm_node3_body(a, smem);
}
// the launch's record: f_in / s_in are [N, ld] bf16 rows (C = Cin = 64); UV' = (f_in . Wuv^T) * uv_scale + uv_shift and the
// node branch s_out are stored as bf16, the root term as fp32; cv gives br and the node branch's bn / sn / tn
static NodeUvH node3_h(const HOp& f_in, const HOp& s_in, const u16* Wuv, const u16* Wr, const u16* Wn, const float* uv_scale,
                       const float* uv_shift, const yolat_conv_eval& cv, u16* UV, float* root, u16* s_out, long ld_so) {
  const long C = 64;
  NodeUvH a;
  a.af = f_in; a.as = s_in;
  a.wuv = HOp{Wuv, 64, (int)(2 * C)}; a.wr = HOp{Wr, 64, (int)C}; a.wn = HOp{Wn, 64, (int)C};
  a.euv = plain_epilogue(); a.euv.Yh = UV; a.euv.ldy = 2 * C;
  a.euv.scale = uv_scale; a.euv.shift = uv_shift;
  a.er = plain_epilogue(); a.er.bias = cv.br; a.er.Y = root; a.er.ldy = C;
  a.en = plain_epilogue(); a.en.bias = cv.bn; a.en.scale = cv.sn; a.en.shift = cv.tn; a.en.relu = 1;
  a.en.Yh = s_out; a.en.ldy = ld_so;
  a.N = f_in.rows; a.C = (int)C; a.Cin = 64;
  return a;
}
static int launch_node3_h(const NodeUvH& a, YlGate gate, hipStream_t st) {
  const dim3 grid(yl_cdiv(a.N, 64), 4);
  if (gate.p) hipLaunchKernelGGL(k_hgemm_node3_gated, grid, dim3(256), 0, st, a, gate);
  else hipLaunchKernelGGL(k_hgemm_node3, grid, dim3(256), 0, st, a);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Pooling prologue on bf16 node features (k_pool_prepare of segment.hip): for proposal p
//   Z[p, 0:F] = 0;  Z[p, F:F+D] = max over rows of feats;  Z[p, 2F+D:2F+2D] = mean over rows of fsup   (fp32)
// ------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_pool_prepare_h(const u16* feats, const u16* fsup, long ld, int D, int F,
                                                               const int* seg_ptr, float* Z, long ldz,
                                                               YlGate gate, int np) {
  if (yl_gate_dead(gate)) return;      // fall-back of the one-launch conv stack (conv_local.hip): dead launch
  const int c = blockIdx.x * 256 + threadIdx.x;
  // (the gated launch covers its np proposals with a few hundred rows of workgroups: gridDim.y < np)
  for (int p = blockIdx.y; p < np; p += gridDim.y) {
    float* z = Z + (long)p * ldz;
    if (c < F) { z[c] = 0.f; continue; }
    if (c >= F + 2 * D) continue;
    const int r0 = seg_ptr[p], r1 = seg_ptr[p + 1];
    const bool is_max = c < F + D;
    const int k = is_max ? c - F : c - F - D;
    const u16* srcp = (is_max ? feats : fsup) + k;
    float best = 0.f, s = 0.f;
    bool any = false;
    int r = r0;
    for (; r + 8 <= r1; r += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __uint_as_float((unsigned)srcp[(long)(r + j) * ld] << 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!any || v[j] > best) { best = v[j]; any = true; }
        s += v[j];
      }
    }
    for (; r < r1; ++r) {
      const float v = __uint_as_float((unsigned)srcp[(long)r * ld] << 16);
      if (!any || v > best) { best = v; any = true; }
      s += v;
    }
    if (is_max) {
      z[F + k] = best;
    } else {
      const int cnt = r1 - r0;
      z[2 * F + D + k] = s / (float)(cnt > 1 ? cnt : 1);
    }
  }
}

// P proposals in chunks of 65535 (gridDim.y); a gated launch covers a chunk with <= 1024 rows of workgroups (few to kill)
static int launch_pool_prepare_h(const u16* feats, const u16* fsup, long ld, long D, long F, const int* seg_ptr, long P,
                                 float* Z, long ldz, YlGate gate, hipStream_t st) {
  for (long p0 = 0; p0 < P; p0 += 65535) {
    const long np = (P - p0) < 65535 ? (P - p0) : 65535;
    hipLaunchKernelGGL(k_pool_prepare_h, dim3(yl_cdiv(F + 2 * D, 256), (unsigned)(gate.p && np > 1024 ? 1024 : np)), dim3(256), 0,
                       st, feats, fsup, ld, (int)D, (int)F, seg_ptr + p0, Z + p0 * ldz, ldz, gate, (int)np);
    YL_LAUNCH_CHECK();
  }
  return 0;
}

// YOLAT_CONV_LOCAL: 0 = never, 1 = batches with >= 1024 proposals (default), 2 = every batch
// (read per call: tests flip it in-process)
static __global__ void k_zero_word(int* p) { if (threadIdx.x == 0) *p = 0; }
static int yl_conv_local_mode() {
  const char* e = getenv("YOLAT_CONV_LOCAL");
  return (e && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : 1;      // (3: measurement only — forced, WITHOUT the gated fall-back)
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {
struct PlanH {
  int* row_ptr; int* perm; int* src; int* dst; float* attr; int* work; int* seg_ptr; int* node_seg;
  u16* UV; float* root; u16* f_tmp[YOLAT_MAX_LAYERS]; u16* s_tmp[YOLAT_MAX_LAYERS];
  u16* feats; u16* fsup; float* Z; float* c1; float* c2;
  int* local_flag; int* eptr;
  float* act_work;      // leaky model off the rows8 route: a column range of the fusion block's BatchNorm output, fp32
  u16* rn_h1; u16* rn_h2;   // row-norm model: the classifier's normalised hidden activations, bf16 (c1 / c2 hold the fp32 GEMMs)
  float* rn_work;       // row-norm model on the materialising route: a row range of the fusion block's output, fp32
  size_t bytes;
};
// weights of the fusion pair: Wf / Wfs bf16 with their fp32 bias and BatchNorm scale / shift, the BatchNorm-folded forms
// (optional), and the slopes of a leaky model by address (both, or none for ReLU)
struct FusionStageH {
  const u16 *Wf, *Wfs; const float *bf, *sf, *tf, *bfs, *sfs, *tfs;
  const u16 *Wf_fold; const float* tf_fold; const u16* Wfs_fold; const float* tfs_fold; const float *slope_f, *slope_s;
  // a row-norm base (norm != YOLAT_NORM_BATCH): the *_fold weights are CENTRED, sf / tf are not read; gamma / beta of the two
  // sites by address (NULL: instance norm), eps and the descriptor's route
  int norm; int rn_route; const float *gamma_f, *beta_f, *gamma_s, *beta_s; float rn_eps;
};
FusionStageH fusion_weights(const yolat_model_eval_bf16* mh) {
  const yolat_model_eval* m = mh->base;
  const bool leaky = m->act != YOLAT_ACT_RELU;
  FusionStageH w{mh->Wf, mh->Wfs, m->bf, m->sf, m->tf, m->bfs, m->sfs, m->tfs, mh->Wf_fold, mh->tf_fold, mh->Wfs_fold,
                 mh->tfs_fold, leaky ? m->act_slope[0] : nullptr, leaky ? m->act_slope[1] : nullptr};
  if (m->norm != YOLAT_NORM_BATCH) {
    w.norm = m->norm; w.rn_route = m->rn_route; w.rn_eps = m->rn_eps;
    w.gamma_f = m->rn_gamma[0]; w.beta_f = m->rn_beta[0]; w.gamma_s = m->rn_gamma[1]; w.beta_s = m->rn_beta[1];
  }
  return w;
}
// does the fusion pair run on the A-in-registers rows kernel (fusion_h8.hip)?  A function of the weights and D alone, so
// the workspace sizing, the descriptor check and the stage agree
bool h8_route(const FusionStageH& w, long D) {
  return (D == 64 || D == 128) && w.Wf_fold && w.Wfs_fold && w.tf_fold && w.tfs_fold;
}
// a row-norm base: the fused kernel (fusion_h8_rn.hip) or the materialising route?  A function of the descriptor alone — AUTO
// is the fused kernel wherever the shape fits it (the faster route at both sizes measured, N = 10 k and 200 k: DESIGN.md 6,
// so there is no row threshold as on the fp32 path) — so the workspace sizing and the stage agree
bool rn_fused_h(const FusionStageH& w, long D, long F) {
  return (w.rn_route & 3) != YOLAT_RN_ROUTE_MATERIALISE && h8_route(w, D) && F % 64 == 0;
}
PlanH carve_h(const yolat_model_eval_bf16* mh, long N, long E, long P, void* ws) {
  const yolat_model_eval* m = mh->base;
  Carver c{reinterpret_cast<char*>(ws), 0};
  PlanH p;
  const long C = m->C, F = m->F, D = C * m->n_blocks_out, Ee = E > 0 ? E : 1;
  p.row_ptr = c.take<int>(N + 1); p.perm = c.take<int>(Ee); p.src = c.take<int>(Ee); p.dst = c.take<int>(Ee);
  p.attr = c.take<float>(Ee * 4); p.work = c.take<int>(yolat_graph_work_elems(N, E));
  p.seg_ptr = c.take<int>(P + 1); p.node_seg = c.take<int>(N);
  p.UV = c.take<u16>(N * 2 * C); p.root = c.take<float>(N * C);
  const int lo = m->n_blocks - m->n_blocks_out;
  for (int l = 0; l < m->n_blocks; ++l) {
    p.f_tmp[l] = (l < lo) ? c.take<u16>(N * C) : nullptr;
    p.s_tmp[l] = (l < lo) ? c.take<u16>(N * C) : nullptr;
  }
  p.feats = c.take<u16>(N * D); p.fsup = c.take<u16>(N * D);
  p.Z = c.take<float>(P * 2 * (F + D)); p.c1 = c.take<float>(P * m->H1); p.c2 = c.take<float>(P * m->H2);
  p.local_flag = c.take<int>(64);
  p.eptr = c.take<int>(P + 1);
  // (carved last and for a leaky descriptor only: a ReLU one keeps its layout and its size)
  p.act_work = nullptr;
  if (m->act != YOLAT_ACT_RELU && !h8_route(fusion_weights(mh), D))
    p.act_work = c.take<float>((long)yolat_fusion_pair_eval_act_work_elems(N, F));
  // (the same for a row-norm descriptor: the bf16 hidden activations, then the row range of the materialising route)
  p.rn_h1 = nullptr; p.rn_h2 = nullptr; p.rn_work = nullptr;
  if (m->norm != YOLAT_NORM_BATCH) {
    p.rn_h1 = c.take<u16>(P * m->H1); p.rn_h2 = c.take<u16>(P * m->H2);
    if (!rn_fused_h(fusion_weights(mh), D, F)) p.rn_work = c.take<float>((long)yolat_fusion_pair_eval_rn_work_elems(N, F));
  }
  p.bytes = c.off + 256;
  return p;
}

int model_ok(const yolat_model_eval_bf16* mh) {
  if (!mh || !mh->base) return YOLAT_E_INVALID;
  const yolat_model_eval* m = mh->base;
  if (m->n_blocks < 1 || m->n_blocks > YOLAT_MAX_LAYERS || m->n_blocks_out < 1 || m->n_blocks_out > m->n_blocks)
    return YOLAT_E_INVALID;
  // a row-norm base (rownorm.hip, fusion_h8_rn.hip) runs here when its author opted in (YOLAT_RN_ROUTE_BF16): ReLU only
  if (m->norm != YOLAT_NORM_BATCH) {
    if (m->norm != YOLAT_NORM_LAYER && m->norm != YOLAT_NORM_INSTANCE) return YOLAT_E_INVALID;
    if ((m->rn_route & YOLAT_RN_ROUTE_BF16) == 0) return YOLAT_E_UNSUPPORTED;
    const int route = m->rn_route & ~YOLAT_RN_ROUTE_BF16;
    if (route < YOLAT_RN_ROUTE_AUTO || route > YOLAT_RN_ROUTE_MATERIALISE || !(m->rn_eps >= 0.f)) return YOLAT_E_INVALID;
    if (m->act != YOLAT_ACT_RELU) return YOLAT_E_INVALID;
    for (int i = 0; i < 4; ++i) {
      if ((m->rn_gamma[i] == nullptr) != (m->rn_beta[i] == nullptr)) return YOLAT_E_INVALID;
      if (m->norm == YOLAT_NORM_LAYER && !m->rn_gamma[i]) return YOLAT_E_INVALID;
    }
  }
  // the activation of the four sites behind the conv stack (act.hip): every launch reads its slope through the address
  if (m->act != YOLAT_ACT_RELU && m->act != YOLAT_ACT_LEAKYRELU && m->act != YOLAT_ACT_PRELU) return YOLAT_E_INVALID;
  if (m->act != YOLAT_ACT_RELU)
    for (int i = 0; i < 4; ++i) if (!m->act_slope[i]) return YOLAT_E_INVALID;
  const long D = m->C * m->n_blocks_out;
  // shapes the bf16 kernels are written for (the reference's: n_filters 64, fusion 1024, classifier 512/256)
  if (m->C != 64 || m->F % 64 != 0 || D % 64 != 0 || (2 * (m->F + D)) % 64 != 0 || m->H1 % 64 != 0 || m->H2 % 64 != 0)
    return YOLAT_E_UNSUPPORTED;
  for (int l = 0; l < m->n_blocks; ++l) {
    const yolat_conv_eval& cv = m->conv[l];
    if (!cv.Wuv || !cv.Wc4 || !mh->W2[l] || !mh->t2f[l] || !mh->uv_scale[l] || !mh->uv_shift[l]) return YOLAT_E_INVALID;
    if (l == 0 ? (cv.Cin > 16) : (cv.Cin != 64)) return YOLAT_E_UNSUPPORTED;
    if (l > 0 && (!mh->Wuv[l] || !mh->Wr[l] || !mh->Wn[l])) return YOLAT_E_INVALID;
  }
  if (!mh->Wf || !mh->Wfs || !mh->Wc1 || !mh->Wc2 || !mh->Wc3) return YOLAT_E_INVALID;
  // (a leaky forward writes the pooled start values before the rows kernel: what that launch would decline is declined here)
  if (m->act != YOLAT_ACT_RELU && h8_route(fusion_weights(mh), D) && (!yl_aligned16(mh->Wf_fold) || !yl_aligned16(mh->Wfs_fold)))
    return YOLAT_E_UNSUPPORTED;
  // (the same for the fused row-norm launch, which comes after the conv stack's launches)
  if (m->norm != YOLAT_NORM_BATCH && rn_fused_h(fusion_weights(mh), D, m->F) &&
      (!yl_aligned16(mh->Wf_fold) || !yl_aligned16(mh->Wfs_fold)))
    return YOLAT_E_UNSUPPORTED;
  return 0;
}

// ---- fusion block (+ per-proposal max) | fusion_block_super in one launch, routed on D and the folded weights.  feats
// [N, ld] bf16; Z [P, ZW] with the pooled max at 0:F (zero before the launch), the super block's fp32 input at 2F+D and its
// output at F+D.  probe (tests): force_groups > 0 replaces the planned column groups of the rows routes, *route names the
// kernel (internal.hpp, yolat_debug_fusion_pair_eval_bf16), groups_ng receives the node problem's (groups, ng).
// A leaky model (act.hip; w.slope_f given): act(y) = y > 0 ? y : a * y per element before the maximum.  Z[:, 0:F] need not
// be prepared, its start values are written here from seg_ptr:
//   route 0  yolat_pool_init_signed (-inf where a proposal has nodes, 0 where it has none), then the ACT instantiation of
//            k_hfusion_rows8 (signed table, fusion_h8.hip)                                              2 launches
//   route 5  every other shape, the scheme of yolat_fusion_pair_eval_act: per column range (<= 64 MiB of `work`) the
//            BatchNorm output in fp32 by the bf16 tile GEMM, then yolat_segment_act_max (one writer per element); the super
//            block as a tile GEMM with the activation in its epilogue                                   2 x ranges + 1
struct FusionIoH {
  const u16* feats; long ld, N, D; const int *node_seg, *seg_ptr; float* Z; long ZW, P, F;
  float* work;         // leaky off the rows8 route: yolat_fusion_pair_eval_act_work_elems(N, F) floats
};
struct FusionProbe { int force_groups; int* route; int* groups_ng; };
// ---- the pair behind a row norm (w.norm != YOLAT_NORM_BATCH; ReLU): Z[:, 0:F] zero before the call.
//   route 6  k_hfusion_rows8_rn on the centred *_fold weights (fusion_h8_rn.hip)                        1 launch
//   route 7  every other shape, per row range (<= 64 MiB of `work`): the bf16 tile GEMM with the bias into fp32, the row norm
//            + ReLU in place (yolat_rownorm_act), the range maximum into the pool (k_rn_range_max); the super block as a
//            tile GEMM into its fp32 slot of Z and the row norm in place                                3 x ranges + 2
int fusion_stage_rn(const FusionStageH& w, const FusionIoH& io, hipStream_t st, const FusionProbe& probe) {
  const long ld = io.ld, N = io.N, D = io.D, ZW = io.ZW, P = io.P, F = io.F;
  float* const Z = io.Z;
  if (rn_fused_h(w, D, F)) {
    if (probe.route != nullptr) *probe.route = 6;
    return yl_hfusion_rows8_rn(io.feats, ld, N, D, w.Wf_fold, w.tf_fold, w.gamma_f, w.beta_f, io.node_seg, Z, ZW, F, Z + 2 * F + D,
                               ZW, P, w.Wfs_fold, w.tfs_fold, w.gamma_s, w.beta_s, Z + F + D, ZW, w.rn_eps, st);
  }
  if (io.work == nullptr) return YOLAT_E_INVALID;
  if (probe.route != nullptr) *probe.route = 7;
  const long rc = (long)(yolat_fusion_pair_eval_rn_work_elems(N, F) / (size_t)F);
  if (probe.groups_ng != nullptr) { probe.groups_ng[0] = (int)yl_cdiv(N, rc); probe.groups_ng[1] = (int)yl_cdiv(F, 64); }
  for (long r0 = 0; r0 < N; r0 += rc) {
    const long n = N - r0 < rc ? N - r0 : rc;
    Epilogue e = plain_epilogue();
    e.bias = w.bf; e.Y = io.work; e.ldy = F;
    YL_TRY(launch_hgemm(HOp{io.feats + r0 * ld, ld, (int)n}, HOp{w.Wf, D, (int)F}, e, n, F, D, st));
    YL_TRY(yolat_rownorm_act(io.work, F, n, F, w.gamma_f, w.beta_f, w.rn_eps, 1, io.work, F, nullptr, nullptr, (yolat_stream_t)st));
    YL_TRY(yl_rn_range_max(io.work, F, n, F, io.node_seg + r0, P, Z, ZW, st));
  }
  Epilogue e1 = plain_epilogue();
  e1.bias = w.bfs; e1.Y = Z + F + D; e1.ldy = ZW;
  YL_TRY(launch_hgemm(FOp{Z + 2 * F + D, ZW, (int)P}, HOp{w.Wfs, D, (int)F}, e1, P, F, D, st));
  return yolat_rownorm_act(Z + F + D, ZW, P, F, w.gamma_s, w.beta_s, w.rn_eps, 1, Z + F + D, ZW, nullptr, nullptr, (yolat_stream_t)st);
}
int yl_fusion_stage_bf16(const FusionStageH& w, const FusionIoH& io, hipStream_t st, const FusionProbe& probe = {}) {
  if (w.norm != YOLAT_NORM_BATCH) return fusion_stage_rn(w, io, st, probe);
  const u16* feats = io.feats;
  const long ld = io.ld, N = io.N, D = io.D, ZW = io.ZW, P = io.P, F = io.F;
  const int *node_seg = io.node_seg, force_groups = probe.force_groups;
  float* const Z = io.Z;
  int *const route = probe.route, *const groups_ng = probe.groups_ng;
  HOp a0{feats, ld, (int)N}, b0{w.Wf, D, (int)F}, b1{w.Wfs, D, (int)F};
  FOp a1{Z + 2 * F + D, ZW, (int)P};
  Epilogue e0 = plain_epilogue(), e1 = plain_epilogue();
  e0.bias = w.bf; e0.scale = w.sf; e0.shift = w.tf; e0.relu = 1; e0.seg = node_seg; e0.pool = Z; e0.ldpool = ZW;
  e1.bias = w.bfs; e1.scale = w.sfs; e1.shift = w.tfs; e1.relu = 1; e1.Y = Z + F + D; e1.ldy = ZW;
  if (w.slope_f != nullptr) {
    if (h8_route(w, D) && F % 64 == 0) {
      if (route != nullptr) *route = 0;
      YL_TRY(yolat_pool_init_signed(io.seg_ptr, P, F, Z, ZW, (yolat_stream_t)st));
      return yl_hfusion_rows8(feats, ld, N, D, w.Wf_fold, w.tf_fold, node_seg, Z, ZW, F, Z + 2 * F + D, ZW, P, w.Wfs_fold,
                              w.tfs_fold, Z + F + D, ZW, st, force_groups, groups_ng, w.slope_f, w.slope_s);
    }
    if (io.work == nullptr) return YOLAT_E_INVALID;
    if (route != nullptr) *route = 5;
    const long fc = (long)(yolat_fusion_pair_eval_act_work_elems(N, F) / (size_t)N);
    if (groups_ng != nullptr) { groups_ng[0] = (int)yl_cdiv(F, fc); groups_ng[1] = (int)yl_cdiv(fc, 64); }
    for (long c0 = 0; c0 < F; c0 += fc) {
      const long wd = F - c0 < fc ? F - c0 : fc;
      Epilogue e = plain_epilogue();
      e.bias = w.bf ? w.bf + c0 : nullptr; e.scale = w.sf + c0; e.shift = w.tf + c0; e.relu = 0; e.Y = io.work; e.ldy = wd;
      YL_TRY(launch_hgemm(a0, HOp{w.Wf + c0 * D, D, (int)wd}, e, N, wd, D, st));
      YL_TRY(yolat_segment_act_max(io.work, wd, N, wd, w.slope_f, io.seg_ptr, P, Z + c0, ZW, (yolat_stream_t)st));
    }
    e1.relu = 0;
    return launch_hgemm(a1, b1, e1, P, F, D, st, nullptr, w.slope_s);
  }
  const int tm1 = yl_cdiv(P, 64), tn1 = yl_cdiv(F, 64);
  const long n1p = ((long)tm1 * tn1 + 7) & ~7L;
  if (h8_route(w, D)) {
    // A-in-registers rows kernel on the BatchNorm-folded weights (fusion_h8.hip)
    if (route != nullptr) *route = 0;
    return yl_hfusion_rows8(feats, ld, N, D, w.Wf_fold, w.tf_fold, node_seg, Z, ZW, F, Z + 2 * F + D, ZW, P, w.Wfs_fold,
                            w.tfs_fold, Z + F + D, ZW, st, force_groups, groups_ng);
  } else if (D <= 256) {
    // A-resident rows kernel: at least 4 column groups, and as many as it takes to put >= ~1024 workgroups on
    // the GPU (each group walks tn / groups consecutive 64-column tiles)
    const int tn = yl_cdiv(F, 64);
    // measured at cfg 5 (N = 200k): 64-row tiles x 4 column groups 160 us, x 1 group 166 us, 128-row tiles 181 us
    // (x 1) / 161 us (x 4); cfg 2 (N = 10k): 8 groups 16.1 us, 16 groups 16.8 us, 2 groups 21.2 us
    const int tm0 = yl_cdiv(N, 64);
    int groups = 4;
    while ((long)tm0 * groups < 1024 && groups < tn) groups *= 2;
    if (force_groups > 0) groups = force_groups;
    if (groups > tn) groups = tn;
    const int ng = yl_cdiv(tn, groups);
    groups = yl_cdiv(tn, ng);
    const long total = (long)tm0 * groups + n1p;
    if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
    if (route != nullptr) *route = D <= 128 ? 1 : 2;
    if (groups_ng != nullptr) { groups_ng[0] = groups; groups_ng[1] = ng; }
    hipLaunchKernelGGL((D <= 128 ? k_hfusion_rows<1, 128> : k_hfusion_rows<1, 256>), dim3((unsigned)total), dim3(256), 0, st, a0,
                       b0, e0, (int)N, (int)F, (int)D, tm0, groups, ng, a1, b1, e1, (int)P, (int)F, (int)D, tm1, tn1);
  } else {
    const bool big = N >= 65536;                       // 128x128 tiles once there are enough of them to fill the GPU
    const int tm0 = yl_cdiv(N, big ? 128 : 64), tn0 = yl_cdiv(F, big ? 128 : 64);
    const long total = (long)tm0 * tn0 + n1p;
    if (total >= (1LL << 31)) return YOLAT_E_UNSUPPORTED;
    if (route != nullptr) *route = big ? 4 : 3;
    if (groups_ng != nullptr) { groups_ng[0] = tn0; groups_ng[1] = 1; }
    hipLaunchKernelGGL((big ? k_hgemm_two<2> : k_hgemm_two<1>), dim3((unsigned)total), dim3(256), 0, st, a0, b0, e0, (int)N,
                       (int)F, (int)D, tm0, tn0, a1, b1, e1, (int)P, (int)F, (int)D, tm1, tn1);
  }
  YL_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// one profiled stage: `body` is a statement block that may `return` an error code
#define YL_HSTAGE(name, flops, bytes, ...)                                    \
  do {                                                                        \
    const bool prof__ = yl_profile_on();                                      \
    if (prof__) yl_stage_begin(name, (double)(flops), (double)(bytes), stream); \
    __VA_ARGS__                                                               \
    if (prof__) yl_stage_end(stream);                                         \
  } while (0)

extern "C" size_t yolat_forward_eval_bf16_workspace_bytes(const yolat_model_eval_bf16* mh, int64_t N, int64_t E,
                                                          int64_t P) {
  if (!mh || !mh->base || N <= 0 || E < 0 || P <= 0) return 0;
  return carve_h(mh, N, E, P, nullptr).bytes;
}

// What one forward is called with.  The graph comes as a COO list (edge / e_attr / bbox_idx; g NULL) or prepared (g, whose
// node_seg stands in for bbox_idx); primed: the caller vouches for the workspace (below); loc: optional
struct ForwardArgsH {
  const yolat_model_eval_bf16* mh; const float* x; int64_t ldx;
  const int64_t* edge; int64_t stride_e, stride_c; const float* e_attr; const int64_t* bbox_idx;
  const yolat_graph_csr* g;
  int64_t N, E, P; float* logits; int64_t ld_logits; void* workspace; size_t workspace_bytes;
  int32_t* status; bool primed; const yolat_locality* loc; yolat_stream_t stream;
};
static int forward_eval_bf16_impl(const ForwardArgsH& a);

extern "C" int yolat_forward_eval_bf16(const yolat_model_eval_bf16* mh, const float* x, int64_t ldx,
                                       const int64_t* edge, int64_t stride_e, int64_t stride_c, const float* e_attr,
                                       const int64_t* bbox_idx, int64_t N, int64_t E, int64_t P, float* logits,
                                       int64_t ld_logits, void* workspace, size_t workspace_bytes, int32_t* status,
                                       yolat_stream_t stream) {
  return forward_eval_bf16_impl(ForwardArgsH{mh, x, ldx, edge, stride_e, stride_c, e_attr, bbox_idx, nullptr, N, E, P, logits,
                                             ld_logits, workspace, workspace_bytes, status, false, nullptr, stream});
}

// The same forward for a caller that vouches for the workspace: its previous use was yolat_forward_eval_bf16 /
// _bf16_primed with the same m layout, N, E and P on the same stream (every forward leaves the CSR-build counters zero,
// so the memset launch is skipped — the contract of yolat_forward_eval_primed).
extern "C" int yolat_forward_eval_bf16_primed(const yolat_model_eval_bf16* mh, const float* x, int64_t ldx,
                                              const int64_t* edge, int64_t stride_e, int64_t stride_c,
                                              const float* e_attr, const int64_t* bbox_idx, int64_t N, int64_t E,
                                              int64_t P, float* logits, int64_t ld_logits, void* workspace,
                                              size_t workspace_bytes, int32_t* status, yolat_stream_t stream) {
  return forward_eval_bf16_impl(ForwardArgsH{mh, x, ldx, edge, stride_e, stride_c, e_attr, bbox_idx, nullptr, N, E, P, logits,
                                             ld_logits, workspace, workspace_bytes, status, true, nullptr, stream});
}

extern "C" int yolat_forward_eval_bf16_csr(const yolat_model_eval_bf16* mh, const float* x, int64_t ldx,
                                           const yolat_graph_csr* g, int64_t N, int64_t E, int64_t P, float* logits,
                                           int64_t ld_logits, void* workspace, size_t workspace_bytes,
                                           yolat_stream_t stream) {
  YL_TRY(yl_adopt_graph<PlanH>(g, E, nullptr));
  int32_t unused_status = 0;
  return forward_eval_bf16_impl(ForwardArgsH{mh, x, ldx, nullptr, 0, 0, nullptr, reinterpret_cast<const int64_t*>(g->node_seg),
                                             g, N, E, P, logits, ld_logits, workspace, workspace_bytes, &unused_status, false,
                                             nullptr, stream});
}

extern "C" int yolat_forward_eval_bf16_loc(const yolat_model_eval_bf16* mh, const float* x, int64_t ldx,
                                           const int64_t* edge, int64_t stride_e, int64_t stride_c, const float* e_attr,
                                           const int64_t* bbox_idx, const yolat_graph_csr* g, int64_t N, int64_t E,
                                           int64_t P, float* logits, int64_t ld_logits, void* workspace,
                                           size_t workspace_bytes, int32_t* status, const yolat_locality* loc, int primed,
                                           yolat_stream_t stream) {
  if (g != nullptr) {
    YL_TRY(yl_adopt_graph<PlanH>(g, E, nullptr));
    if (!status) return YOLAT_E_INVALID;
    return forward_eval_bf16_impl(ForwardArgsH{mh, x, ldx, nullptr, 0, 0, nullptr, reinterpret_cast<const int64_t*>(g->node_seg),
                                               g, N, E, P, logits, ld_logits, workspace, workspace_bytes, status, false, loc,
                                               stream});
  }
  return forward_eval_bf16_impl(ForwardArgsH{mh, x, ldx, edge, stride_e, stride_c, e_attr, bbox_idx, nullptr, N, E, P, logits,
                                             ld_logits, workspace, workspace_bytes, status, primed != 0, loc, stream});
}

static int forward_eval_bf16_impl(const ForwardArgsH& args) {
  const yolat_model_eval_bf16* mh = args.mh;
  const float *x = args.x, *e_attr = args.e_attr;
  const int64_t *edge = args.edge, *bbox_idx = args.bbox_idx;
  const int64_t ldx = args.ldx, stride_e = args.stride_e, stride_c = args.stride_c, N = args.N, E = args.E, P = args.P;
  const yolat_graph_csr* g = args.g;
  const yolat_locality* loc = args.loc;
  float* const logits = args.logits;
  int32_t* const status = args.status;
  const yolat_stream_t stream = args.stream;
  if (!x || !bbox_idx || !logits || !args.workspace || !status || N <= 0 || E < 0 || P <= 0) return YOLAT_E_INVALID;
  YL_TRY(model_ok(mh));
  if (N > (1LL << 23) || E > (1LL << 29)) return YOLAT_E_UNSUPPORTED;     // 32-bit element offsets in the gathers
  if (P * 2 * (mh->base->F + mh->base->C * mh->base->n_blocks_out) >= (1LL << 32)) return YOLAT_E_UNSUPPORTED;
  const yolat_model_eval* m = mh->base;
  PlanH p = carve_h(mh, N, E, P, args.workspace);
  if (p.bytes > args.workspace_bytes) return YOLAT_E_INVALID;
  if (g != nullptr) YL_TRY(yl_adopt_graph(g, E, &p));      // prepared graph (collate.hip): the caller's arrays
  hipStream_t st = (hipStream_t)stream;
  const long C = m->C, F = m->F, D = C * m->n_blocks_out, ZW = 2 * (F + D);
  const int lo = m->n_blocks - m->n_blocks_out;
  auto f_slot = [&](int l) { return l - lo >= 0 ? p.feats + (l - lo) * C : p.f_tmp[l]; };
  auto s_slot = [&](int l) { return l - lo >= 0 ? p.fsup + (l - lo) * C : p.s_tmp[l]; };
  auto ld_slot = [&](int l) { return l - lo >= 0 ? D : C; };

  // ---- the one-launch conv stack (conv_local.hip) applies to models of its shapes on batches large enough to fill the
  // chip; whether THIS batch has the property (edges inside their proposal, proposals that fit a tile) is found out on the
  // device: the per-layer launches below stay enqueued, gated on the word the conv kernel raises
  const yolat_conv_eval& cv0 = m->conv[0];
  NodeUv a0;
  // the fp32 destinations are placeholders for the builder's checks; UV and the node branch go to bf16
  YL_TRY(yl_build_node_uv(&a0, x, ldx, x, ldx, N, cv0.Cin, cv0.Wuv, nullptr, cv0.Wr, cv0.br, cv0.Wn, cv0.bn, cv0.sn, cv0.tn, C,
                          p.root, 2 * C, p.root, C, p.root, C));
  a0.euv.Y = nullptr; a0.euv.Yh = p.UV; a0.euv.ldy = 2 * C;
  a0.euv.scale = mh->uv_scale[0]; a0.euv.shift = mh->uv_shift[0];
  a0.en.Y = nullptr; a0.en.Yh = s_slot(0); a0.en.ldy = ld_slot(0);
  const int local_mode = yl_conv_local_mode();
  const bool known = loc != nullptr && loc->known != 0;
  const bool fits = known && yolat_conv_local_fits(loc, P) != 0;
  // (a batch known NOT to have the property goes straight to the per-layer launches)
  const bool local = local_mode != 0 && mh->conv_local != nullptr && yl_conv_local_model_ok(mh) &&
                     yl_node3_smallk_shape_ok(a0) && D % 8 == 0 && ZW % 4 == 0 && (local_mode >= 2 || P >= 1024) &&
                     (!known || fits) && (g != nullptr || E == 0 || yl_aligned16(e_attr) || !fits);
  // vouched: the caller examined the batch (yolat_batch_locality / the host collate) — no gated fall-back launches, and
  // for a COO batch no global destination sort either: the tiles sort their edges themselves
  const bool vouched = local && fits && (g != nullptr || E > 0);      // (no edges: nothing to sort, the gated form has no cost)
  YlGate gate{nullptr, 0};
  int flag_val = 0;
  if (local) {
    // the word the conv kernel raises: a fresh value per forward instead of a reset launch.  High bit set: the workspace
    // is re-carved per shape and may hold stale int32 index data (< 2^30) at this address, which must never look raised
    static std::atomic<unsigned> epoch_counter{0};
    flag_val = (int)(0x80000000u | (++epoch_counter & 0x7FFFFFFFu));
    if (!vouched) { gate.p = p.local_flag; gate.val = flag_val; }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
      // a captured forward replays with THIS value: a replay on an unfit batch would leave the word raised for every later
      // replay (the fall-back would run for fit batches too) — reset it inside the graph (a kernel, not a memset node: §4)
      hipLaunchKernelGGL(k_zero_word, dim3(1), dim3(64), 0, (hipStream_t)stream, p.local_flag);
      YL_LAUNCH_CHECK();
    }
  }

  // ---- graph structure + node side of layer 0 (fp32 MFMA on the raw K = Cin0 features, bf16 / fp32 outputs)
  char nm[112];
  YL_HSTAGE("graph_prep[csr+attr+segments] + node_uv[layer 0, bf16 out]", 8.0 * N * m->conv[0].Cin * C,
            16.0 * E + 12.0 * E + 32.0 * E + 12.0 * N + 4.0 * N * m->conv[0].Cin + 2.0 * N * 3 * C + 4.0 * N * C, {
    const NodeUv& a = a0;
    if (vouched) {
      if (g == nullptr)
        YL_TRY(yl_local_prep(edge, stride_e, stride_c, bbox_idx, N, E, P, p.seg_ptr, p.node_seg, p.eptr, status, nullptr, true,
                             st));
    } else if (local) {
      if (g == nullptr)
        YL_TRY(yl_graph_prepare_impl(edge, stride_e, stride_c, e_attr, bbox_idx, E, N, P, p.row_ptr, p.perm, p.src, p.dst,
                                     p.attr, p.seg_ptr, p.node_seg, p.work, status, nullptr, args.primed, stream));
    } else if (g != nullptr && yl_node3_smallk_ok(a)) {
      YL_TRY(yl_node3_smallk(a, st));
    } else if (g != nullptr) {
      const dim3 grid(yl_cdiv(N, 64), 4);
      if (cv0.Cin <= 16) hipLaunchKernelGGL(k_gemm_nt_node3<16>, grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(k_gemm_nt_node3<32>, grid, dim3(256), 0, st, a);
      YL_LAUNCH_CHECK();
    } else {
    YL_TRY(yl_graph_prepare_impl(edge, stride_e, stride_c, e_attr, bbox_idx, E, N, P, p.row_ptr, p.perm, p.src, p.dst,
                                 p.attr, p.seg_ptr, p.node_seg, p.work, status, &a, args.primed, stream));
    }
  });
  if (local) {
    double fl = 0.0;
    for (int l = 0; l < m->n_blocks; ++l) fl += 2.0 * E * (4.0 * C + C * C) + 8.0 * N * m->conv[l].Cin * C;
    // bytes: what the stack has to move — x, ids, e_attr in; feats + the pooled rows out
    YL_HSTAGE("conv_local_bf16[all conv layers + pooling prologue, one launch]", fl,
              4.0 * N * cv0.Cin + 8.0 * E + 16.0 * E + 4.0 * N + 2.0 * N * D + 4.0 * P * (F + 2 * D), {
      YlLocalIn in{};
      in.seg_ptr = p.seg_ptr;
      if (vouched && g == nullptr) {
        in.attr = e_attr; in.edge = edge; in.se = stride_e; in.sc = stride_c; in.eptr = p.eptr;
      } else {
        in.row_ptr = p.row_ptr; in.src = p.src; in.dst = p.dst; in.attr = p.attr;
      }
      in.status = vouched ? status : nullptr;
      YL_TRY(yl_conv_local_bf16(mh, mh->conv_local, x, ldx, in, N, E, P, p.feats, D, p.Z, ZW, p.local_flag, flag_val, st));
    });
    // the fall-back's layer-0 node side (dead unless the flag was raised)
    if (local_mode != 3 && !vouched) YL_TRY(yl_node3_smallk(a0, st, gate));
  }
  const bool no_layers = local && (local_mode == 3 || vouched);
  for (int l = 0; l < m->n_blocks && !no_layers; ++l) {
    const yolat_conv_eval& cv = m->conv[l];
    if (l > 0) {
      snprintf(nm, sizeof nm, "node_uv_bf16[UV | lin_r | mlp_node, N x 64 -> %ld+%ld+%ld]%s", 2 * C, C, C,
               local ? " (gated fall-back)" : "");
      YL_HSTAGE(nm, 8.0 * N * 64 * C, 2.0 * (2.0 * N * 64 + 3.0 * N * C) + 4.0 * N * C, {
        YL_TRY(launch_node3_h(node3_h(HOp{f_slot(l - 1), ld_slot(l - 1), (int)N}, HOp{s_slot(l - 1), ld_slot(l - 1), (int)N},
                                      mh->Wuv[l], mh->Wr[l], mh->Wn[l], mh->uv_scale[l], mh->uv_shift[l], cv, p.UV, p.root,
                                      s_slot(l), ld_slot(l)), gate, st));
      });
    }
    snprintf(nm, sizeof nm, "edge_uv_mlp2_mean_bf16[E x (U+V+attr) -> %ld -> %ld -> mean]%s", C, C,
             local ? " (gated fall-back)" : "");
    // bytes: SURVEY.md 8(d) B_agg(l) of the UNFACTORISED layer at 2 bytes per feature element,
    // E ((2 Cin + 4) s + 2 * 4) + N C s — the credit figure; what the kernel has to move is priced in bench.py
    YL_HSTAGE(nm, 2.0 * E * (4.0 * C + C * C), E * ((2.0 * cv.Cin + 4.0) * 2.0 + 8.0) + 2.0 * N * C, {
      YL_TRY(yl_edge_uv_mlp2_mean_bf16_impl(p.UV, 2 * C, p.src, p.dst, p.attr, p.row_ptr, N, E, cv.Wc4, cv.s1, mh->W2[l],
                                            mh->t2f[l], p.root, C, f_slot(l), ld_slot(l), 0, st, gate));
    });
  }

  // ---- pooling prologue, fusion block (+ per-proposal max) | fusion_block_super, classifier
  if (!no_layers)
  YL_HSTAGE(local ? "pool_prepare_bf16[max(feats), mean(fsup), zero] (gated fall-back)"
                  : "pool_prepare_bf16[max(feats), mean(fsup), zero]", 2.0 * N * D, 4.0 * N * D + 4.0 * P * (F + 2 * D), {
    YL_TRY(launch_pool_prepare_h(p.feats, p.fsup, D, D, F, p.seg_ptr, P, p.Z, ZW, gate, st));
  });
  snprintf(nm, sizeof nm, "fusion_gemm_bf16+segmax[N x %ld -> %ld -> P] | super[P x %ld -> %ld]", D, F, D, F);
  YL_HSTAGE(nm, 2.0 * (N + P) * D * F, 2.0 * (N * D + 2.0 * D * F) + 4.0 * (2.0 * P * F + N + P * D), {
    YL_TRY(yl_fusion_stage_bf16(fusion_weights(mh), FusionIoH{p.feats, D, N, D, p.node_seg, p.seg_ptr, p.Z, ZW, P, F,
                                                              m->norm != YOLAT_NORM_BATCH ? p.rn_work : p.act_work}, st));
  });
  if (m->norm != YOLAT_NORM_BATCH) {
    // a row norm does not fold into its Linear: layers 1 and 2 are the tile GEMM with the bias into the fp32 buffers c1 / c2,
    // then ONE row-norm launch each that reads fp32 and writes the normalised, ReLU'd row as bf16 into a buffer of its own
    // (in place would be a race: bf16 row r overlaps fp32 row r / 2, which belongs to another wave).  Layer 3 as ever.
    Epilogue e = plain_epilogue();
    e.bias = m->bc1; e.Y = p.c1; e.ldy = m->H1;
    snprintf(nm, sizeof nm, "cls1_bf16[P x %ld -> %ld] + rownorm", ZW, (long)m->H1);
    YL_HSTAGE(nm, 2.0 * P * ZW * m->H1, 4.0 * P * ZW + 10.0 * P * m->H1 + 2.0 * ZW * m->H1, {
      YL_TRY(launch_hgemm(FOp{p.Z, ZW, (int)P}, HOp{mh->Wc1, ZW, (int)m->H1}, e, P, m->H1, ZW, st));
      YL_TRY(yl_rownorm_act_h(p.c1, m->H1, P, m->H1, m->rn_gamma[2], m->rn_beta[2], m->rn_eps, p.rn_h1, m->H1, st));
    });
    e.bias = m->bc2; e.Y = p.c2; e.ldy = m->H2;
    snprintf(nm, sizeof nm, "cls2_bf16[P x %ld -> %ld] + rownorm", (long)m->H1, (long)m->H2);
    YL_HSTAGE(nm, 2.0 * P * m->H1 * m->H2, 2.0 * P * m->H1 + 10.0 * P * m->H2 + 2.0 * m->H1 * m->H2, {
      YL_TRY(launch_hgemm(HOp{p.rn_h1, m->H1, (int)P}, HOp{mh->Wc2, m->H1, (int)m->H2}, e, P, m->H2, m->H1, st));
      YL_TRY(yl_rownorm_act_h(p.c2, m->H2, P, m->H2, m->rn_gamma[3], m->rn_beta[3], m->rn_eps, p.rn_h2, m->H2, st));
    });
    e = plain_epilogue();
    e.bias = m->bc3; e.Y = logits; e.ldy = args.ld_logits;
    snprintf(nm, sizeof nm, "cls3_bf16[P x %ld -> %d]", (long)m->H2, (int)m->n_classes);
    YL_HSTAGE(nm, 2.0 * P * m->H2 * m->n_classes, 2.0 * P * m->H2 + 4.0 * P * m->n_classes + 2.0 * m->H2 * m->n_classes, {
      YL_TRY(launch_hgemm(HOp{p.rn_h2, m->H2, (int)P}, HOp{mh->Wc3, m->H2, (int)m->n_classes}, e, P, m->n_classes, m->H2, st));
    });
  } else {
    Epilogue e = plain_epilogue();
    // the hidden activations of the classifier cross HBM as bf16 (in the fp32-sized buffers c1 / c2): the next Linear rounds
    // its rows to bf16 while staging anyway (FOp::pack — the same round-to-nearest-even), so the logits are the same bits
    u16* const c1h = reinterpret_cast<u16*>(p.c1);
    u16* const c2h = reinterpret_cast<u16*>(p.c2);
    auto slope = [&](int i) { return m->act != YOLAT_ACT_RELU ? m->act_slope[i] : nullptr; };
    e.bias = m->bc1; e.scale = m->sc1; e.shift = m->tc1; e.relu = 1; e.Y = nullptr; e.Yh = c1h; e.ldy = m->H1;
    snprintf(nm, sizeof nm, "cls1_bf16[P x %ld -> %ld]", ZW, (long)m->H1);
    YL_HSTAGE(nm, 2.0 * P * ZW * m->H1, 4.0 * P * ZW + 2.0 * P * m->H1 + 2.0 * ZW * m->H1,
    {
      // (a leaky model: the activation in fp32 before the bf16 store, k_hgemm_act)
      YL_TRY(launch_hgemm(FOp{p.Z, ZW, (int)P}, HOp{mh->Wc1, ZW, (int)m->H1}, e, P, m->H1, ZW, st, nullptr, slope(2)));
    });
    e.bias = m->bc2; e.scale = m->sc2; e.shift = m->tc2; e.Yh = c2h; e.ldy = m->H2;
    snprintf(nm, sizeof nm, "cls2_bf16[P x %ld -> %ld]", (long)m->H1, (long)m->H2);
    YL_HSTAGE(nm, 2.0 * P * m->H1 * m->H2, 2.0 * (P * m->H1 + P * m->H2) + 2.0 * m->H1 * m->H2,
    {
      YL_TRY(launch_hgemm(HOp{c1h, m->H1, (int)P}, HOp{mh->Wc2, m->H1, (int)m->H2}, e, P, m->H2, m->H1, st, nullptr, slope(3)));
    });
    e = plain_epilogue();
    e.bias = m->bc3; e.Y = logits; e.ldy = args.ld_logits;
    snprintf(nm, sizeof nm, "cls3_bf16[P x %ld -> %d]", (long)m->H2, (int)m->n_classes);
    YL_HSTAGE(nm, 2.0 * P * m->H2 * m->n_classes, 2.0 * P * m->H2 + 4.0 * P * m->n_classes + 2.0 * m->H2 * m->n_classes, {
      YL_TRY(launch_hgemm(HOp{c2h, m->H2, (int)P}, HOp{mh->Wc3, m->H2, (int)m->n_classes}, e, P, m->n_classes, m->H2, st));
    });
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The dense stages of the forward above as ops of their own (internal.hpp): the same launches, built the same way.
// ------------------------------------------------------------------------------------------------
// fusion pair, ReLU and leaky (the start values of Z[:, 0:F] are then the call's own; off the rows8 route the stage wants `work`)
static int debug_fusion_pair(const FusionStageH& w, const FusionIoH& io, bool leaky, const FusionProbe& probe,
                             yolat_stream_t stream) {
  const long D = io.D, F = io.F;
  if (!io.feats || !io.node_seg || !io.Z || !w.Wf || !w.Wfs || !w.sf || !w.tf || !w.sfs || !w.tfs || io.N <= 0 || io.P <= 0 ||
      F <= 0 || D <= 0 || probe.force_groups < 0 || (leaky && (!io.seg_ptr || !w.slope_f || !w.slope_s)))
    return YOLAT_E_INVALID;
  if (io.N >= (1LL << 31) || io.P >= (1LL << 31) || io.ld < D || io.ZW < 2 * (F + D)) return YOLAT_E_INVALID;
  if (io.P * io.ZW >= (1LL << 32)) return YOLAT_E_UNSUPPORTED;                // 32-bit element offsets into the pooled matrix
  if (D % 64 != 0 || F % 32 != 0 || io.ld % 8 != 0 || io.ZW % 4 != 0 || !yl_aligned16(io.feats) || !yl_aligned16(io.Z) ||
      !yl_aligned16(w.Wf) || !yl_aligned16(w.Wfs) || (w.Wf_fold && !yl_aligned16(w.Wf_fold)) ||
      (w.Wfs_fold && !yl_aligned16(w.Wfs_fold)) || (leaky && io.work && !yl_aligned16(io.work)))
    return YOLAT_E_UNSUPPORTED;
  return yl_fusion_stage_bf16(w, io, (hipStream_t)stream, probe);
}
extern "C" int yolat_debug_fusion_pair_eval_bf16(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                 const int32_t* node_seg, float* Z, int64_t ldz, int64_t P, int64_t F,
                                                 const uint16_t* Wf, const uint16_t* Wfs, const float* bf, const float* sf,
                                                 const float* tf, const float* bfs, const float* sfs, const float* tfs,
                                                 const uint16_t* Wf_fold, const float* tf_fold, const uint16_t* Wfs_fold,
                                                 const float* tfs_fold, int force_groups, int* route, int* groups_ng,
                                                 yolat_stream_t stream) {
  const FusionStageH w{Wf, Wfs, bf, sf, tf, bfs, sfs, tfs, Wf_fold, tf_fold, Wfs_fold, tfs_fold, nullptr, nullptr};
  return debug_fusion_pair(w, FusionIoH{feats, ld, N, D, node_seg, nullptr, Z, ldz, P, F, nullptr}, false,
                           FusionProbe{force_groups, route, groups_ng}, stream);
}
// the same for a leaky model (act.hip), launched as the forward launches it (routes 0 and 5 of yl_fusion_stage_bf16)
extern "C" int yolat_debug_fusion_pair_eval_bf16_act(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                     const int32_t* node_seg, const int32_t* seg_ptr, float* Z, int64_t ldz,
                                                     int64_t P, int64_t F, const uint16_t* Wf, const uint16_t* Wfs,
                                                     const float* bf, const float* sf, const float* tf, const float* bfs,
                                                     const float* sfs, const float* tfs, const uint16_t* Wf_fold,
                                                     const float* tf_fold, const uint16_t* Wfs_fold, const float* tfs_fold,
                                                     const float* slope_f, const float* slope_s, float* work,
                                                     int force_groups, int* route, int* groups_ng, yolat_stream_t stream) {
  const FusionStageH w{Wf, Wfs, bf, sf, tf, bfs, sfs, tfs, Wf_fold, tf_fold, Wfs_fold, tfs_fold, slope_f, slope_s};
  return debug_fusion_pair(w, FusionIoH{feats, ld, N, D, node_seg, seg_ptr, Z, ldz, P, F, work}, true,
                           FusionProbe{force_groups, route, groups_ng}, stream);
}

// the pair behind a row norm, launched as the forward launches it (routes 6 and 7 of fusion_stage_rn); rn_route: YOLAT_RN_ROUTE_*
extern "C" int yolat_debug_fusion_pair_eval_bf16_rn(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                    const int32_t* node_seg, float* Z, int64_t ldz, int64_t P, int64_t F,
                                                    const uint16_t* Wf, const uint16_t* Wfs, const float* bf, const float* bfs,
                                                    const uint16_t* Wf_fold, const float* tf_fold, const uint16_t* Wfs_fold,
                                                    const float* tfs_fold, const float* gamma_f, const float* beta_f,
                                                    const float* gamma_s, const float* beta_s, float eps, int rn_route,
                                                    float* work, int* route, int* groups_ng, yolat_stream_t stream) {
  FusionStageH w{Wf, Wfs, bf, nullptr, nullptr, bfs, nullptr, nullptr, Wf_fold, tf_fold, Wfs_fold, tfs_fold, nullptr, nullptr};
  w.norm = gamma_f != nullptr ? YOLAT_NORM_LAYER : YOLAT_NORM_INSTANCE;
  w.rn_route = rn_route; w.gamma_f = gamma_f; w.beta_f = beta_f; w.gamma_s = gamma_s; w.beta_s = beta_s; w.rn_eps = eps;
  if (!feats || !node_seg || !Z || !Wf || !Wfs || N <= 0 || P <= 0 || F <= 0 || D <= 0 || !(eps >= 0.f) || rn_route < 0 ||
      rn_route > YOLAT_RN_ROUTE_MATERIALISE || (gamma_f == nullptr) != (beta_f == nullptr) ||
      (gamma_s == nullptr) != (beta_s == nullptr) || (gamma_f == nullptr) != (gamma_s == nullptr))
    return YOLAT_E_INVALID;
  if (N >= (1LL << 31) - 512 || P >= (1LL << 31) - 512 || ld < D || ldz < 2 * (F + D)) return YOLAT_E_INVALID;
  if (P * ldz >= (1LL << 32)) return YOLAT_E_UNSUPPORTED;                     // 32-bit element offsets into the pooled matrix
  if (D % 64 != 0 || F % 64 != 0 || ld % 8 != 0 || ldz % 4 != 0 || !yl_aligned16(feats) || !yl_aligned16(Z) || !yl_aligned16(Wf) ||
      !yl_aligned16(Wfs) || (Wf_fold && !yl_aligned16(Wf_fold)) || (Wfs_fold && !yl_aligned16(Wfs_fold)) ||
      (work && !yl_aligned16(work)))
    return YOLAT_E_UNSUPPORTED;
  return yl_fusion_stage_bf16(w, FusionIoH{feats, ld, N, D, node_seg, nullptr, Z, ldz, P, F, work}, (hipStream_t)stream,
                              FusionProbe{0, route, groups_ng});
}
// the classifier's row norm: fp32 rows in, relu(rownorm(Y) gamma + beta) out as bf16 (k_rownorm_act_h, fusion_h8_rn.hip)
extern "C" int yolat_debug_rownorm_act_bf16(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* gamma,
                                            const float* beta, float eps, uint16_t* Z, int64_t ldz, yolat_stream_t stream) {
  return yl_rownorm_act_h(Y, ldy, M, C, gamma, beta, eps, Z, ldz, (hipStream_t)stream);
}

extern "C" int yolat_debug_pool_prepare_bf16(const uint16_t* feats, const uint16_t* fsup, int64_t ld, int64_t D, int64_t F,
                                             const int32_t* seg_ptr, int64_t P, float* Z, int64_t ldz, yolat_stream_t stream) {
  if (!feats || !fsup || !seg_ptr || !Z || P <= 0 || D <= 0 || F <= 0 || ld < D || ldz < 2 * (F + D)) return YOLAT_E_INVALID;
  if (P >= (1LL << 31) || F + 2 * D >= (1LL << 30)) return YOLAT_E_UNSUPPORTED;
  return launch_pool_prepare_h(feats, fsup, ld, D, F, seg_ptr, P, Z, ldz, YlGate{nullptr, 0}, (hipStream_t)stream);
}

extern "C" int yolat_debug_node_uv_eval_bf16(const uint16_t* f_in, int64_t ld_f, const uint16_t* s_in, int64_t ld_s, int64_t N,
                                             const uint16_t* Wuv, const uint16_t* Wr, const uint16_t* Wn,
                                             const float* uv_scale, const float* uv_shift, const float* br, const float* bn,
                                             const float* sn, const float* tn, uint16_t* UV, float* root, uint16_t* s_out,
                                             int64_t ld_so, yolat_stream_t stream) {
  const long C = 64;
  if (!f_in || !s_in || !Wuv || !Wr || !Wn || !uv_scale || !uv_shift || !sn || !tn || !UV || !root || !s_out || N <= 0 ||
      N >= (1LL << 31) || ld_f < C || ld_s < C || ld_so < C)
    return YOLAT_E_INVALID;
  if (ld_f % 8 != 0 || ld_s % 8 != 0 || ld_so % 2 != 0 || !yl_aligned16(f_in) || !yl_aligned16(s_in) || !yl_aligned16(Wuv) ||
      !yl_aligned16(Wr) || !yl_aligned16(Wn) || (((uintptr_t)UV) & 3) != 0 || (((uintptr_t)s_out) & 3) != 0)
    return YOLAT_E_UNSUPPORTED;
  yolat_conv_eval cv{};
  cv.br = br; cv.bn = bn; cv.sn = sn; cv.tn = tn;
  const NodeUvH a = node3_h(HOp{f_in, ld_f, (int)N}, HOp{s_in, ld_s, (int)N}, Wuv, Wr, Wn, uv_scale, uv_shift, cv, UV, root,
                            s_out, ld_so);
  return launch_node3_h(a, YlGate{nullptr, 0}, (hipStream_t)stream);
}

// the tile GEMM, ReLU-or-none and leaky.  A bf16 Y: paired stores (even ldy, 4-byte aligned) / leaky: element by element
struct DebugHgemm {
  const void* A; int a_f32; int64_t lda, M, K; const uint16_t* W; int64_t ldw, Nout; const float *bias, *scale, *shift;
  void* Y; int y_bf16; int64_t ldy; int* tile_form;
};
static int debug_hgemm(const DebugHgemm& g, int relu, const float* slope, bool leaky, yolat_stream_t stream) {
  if (!g.A || !g.W || !g.Y || (leaky && !slope) || g.M <= 0 || g.K <= 0 || g.Nout <= 0 || g.M >= (1LL << 31) ||
      g.Nout >= (1LL << 31) || g.lda < g.K || g.ldw < g.K || g.ldy < g.Nout || (g.scale == nullptr) != (g.shift == nullptr))
    return YOLAT_E_INVALID;
  const uintptr_t y = (uintptr_t)g.Y;
  const bool y_ok = !g.y_bf16 ? (y & 3) == 0 : leaky ? (y & 1) == 0 : (g.ldy % 2 == 0 && (y & 3) == 0);
  if (g.K % 64 != 0 || g.lda % (g.a_f32 ? 4 : 8) != 0 || g.ldw % 8 != 0 || !yl_aligned16(g.A) || !yl_aligned16(g.W) || !y_ok)
    return YOLAT_E_UNSUPPORTED;
  Epilogue e = plain_epilogue();
  e.bias = g.bias; e.scale = g.scale; e.shift = g.shift; e.relu = relu ? 1 : 0; e.ldy = g.ldy;
  if (g.y_bf16) e.Yh = reinterpret_cast<u16*>(g.Y);
  else e.Y = reinterpret_cast<float*>(g.Y);
  const HOp b{g.W, g.ldw, (int)g.Nout};
  if (g.a_f32)
    return launch_hgemm(FOp{reinterpret_cast<const float*>(g.A), g.lda, (int)g.M}, b, e, g.M, g.Nout, g.K, (hipStream_t)stream,
                        g.tile_form, slope);
  return launch_hgemm(HOp{reinterpret_cast<const u16*>(g.A), g.lda, (int)g.M}, b, e, g.M, g.Nout, g.K, (hipStream_t)stream,
                      g.tile_form, slope);
}
extern "C" int yolat_debug_hgemm_eval_bf16(const void* A, int a_f32, int64_t lda, int64_t M, int64_t K, const uint16_t* W,
                                           int64_t ldw, int64_t Nout, const float* bias, const float* scale,
                                           const float* shift, int relu, void* Y, int y_bf16, int64_t ldy, int* tile_form,
                                           yolat_stream_t stream) {
  return debug_hgemm(DebugHgemm{A, a_f32, lda, M, K, W, ldw, Nout, bias, scale, shift, Y, y_bf16, ldy, tile_form}, relu, nullptr,
                     false, stream);
}
extern "C" int yolat_debug_hgemm_eval_bf16_act(const void* A, int a_f32, int64_t lda, int64_t M, int64_t K, const uint16_t* W,
                                               int64_t ldw, int64_t Nout, const float* bias, const float* scale,
                                               const float* shift, const float* slope, void* Y, int y_bf16, int64_t ldy,
                                               int* tile_form, yolat_stream_t stream) {
  return debug_hgemm(DebugHgemm{A, a_f32, lda, M, K, W, ldw, Nout, bias, scale, shift, Y, y_bf16, ldy, tile_form}, 0, slope,
                     true, stream);
}

// the tile GEMM for bf16_linear.hip (internal.hpp): this file holds every k_hgemm instance
int yl_launch_hgemm(const HOp& A, const float* a_scale, const float* a_shift, float a_floor, const HOp& B, const Epilogue& ep,
                    long M, long N, long K, hipStream_t st) {
  if (a_scale != nullptr) return launch_hgemm(HProOp{A.p, A.ld, A.rows, a_scale, a_shift, a_floor}, B, ep, M, N, K, st);
  return launch_hgemm(A, B, ep, M, N, K, st);
}
