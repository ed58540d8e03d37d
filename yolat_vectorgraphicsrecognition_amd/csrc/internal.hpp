// internal.hpp — what one .hip of libyolat_hip.so defines and another one uses: the structures that cross files and EVERY
// non-static function that does.  A function is declared here once, with the file that defines it; the definer and
// every caller include this header, and default arguments appear only here.  No .hip declares such a function by hand
// (tests/test_csrc_decls_host.py).  The C ABI itself is include/yolat_hip.h.
#pragma once
#include "base.hpp"

struct NodeUv;        // gemm_nt.hpp: operands / epilogues of the node side of a factorised conv layer
struct Epilogue; struct HOp;      // epilogue.hpp; hgemm.hpp: bf16 rows as an operand of the tile GEMM

// fills the node side of a factorised conv layer (dense.hip)
int yl_build_node_uv(NodeUv* a, const float* f_in, int64_t ld_f, const float* s_in, int64_t ld_s, int64_t N,
                     int64_t Cin, const float* Wuv, const float* uv_bias, const float* Wr, const float* br,
                     const float* Wn, const float* bn, const float* sn, const float* tn, int64_t C, float* UV,
                     int64_t ld_uv, float* f_out, int64_t ld_fo, float* s_out, int64_t ld_so);
// the node side of the first conv layer (K = in_channels <= 8) of a large graph as an output stream (dense.hip)
bool yl_node3_smallk_ok(const NodeUv& a);
bool yl_node3_smallk_shape_ok(const NodeUv& a);
int yl_node3_smallk(const NodeUv& a, hipStream_t st, YlGate gate = YlGate{nullptr, 0});
// training-mode fusion GEMM with the key64 pooling epilogue on the bf16x6 rows kernel (fusion_x6.hip)
int yl_fusion_rows_x6_key64(const float* A, long lda, long N, long K, const float* W, const float* bias, long F,
                            const float* sgn, const int* node_seg, unsigned long long* keys, uint16_t* wsplit,
                            yolat_stream_t stream);
// the same on bf16 operands ("bf16_dense" training precision, bf16_train.hip): K == 128; wimg = F * K bfloat16
int yl_fusion_rows_bf16_key64(const float* A, long lda, long N, long K, const float* W, const float* bias, long F,
                              const float* sgn, const int* node_seg, unsigned long long* keys, uint16_t* wimg,
                              yolat_stream_t stream);
// ------------------------------------------------------------------------------------------------
// Pooling prologue as a RIDER of other launches (small graphs, where a launch of its own is ~5 us of latency):
// the parts of k_pool_prepare (segment.hip) done by `blocks` extra workgroups appended to a kernel whose own
// workgroups do not depend on them:
//   YL_POOL_ZERO  Z[p, 0:F] = 0                      } ride in the LAST conv layer's edge kernel (need the node branch
//   YL_POOL_MEAN  Z[p, 2F+D:2F+2D] = mean(fsup rows)  } of that layer, ready one launch earlier; read by the fusion launch)
//   YL_POOL_MAX   Z[p, F:F+D] = max(feats rows)        ride in the fusion launch itself (reads feats, like its GEMM)
// Same arithmetic, in the same (row) order, as k_pool_prepare.
// ------------------------------------------------------------------------------------------------
#define YL_POOL_ZERO 1
#define YL_POOL_MAX 2
#define YL_POOL_MEAN 4
struct PoolRider {
  const float* feats; const float* fsup; long ld; int D, F, P; const int* seg_ptr; float* Z; long ldz;
  int parts, blocks;
};
// virtual block vb of nvb, thread tid of nthreads (grid-stride over the items of the selected parts)
__device__ __forceinline__ void yl_pool_rider(const PoolRider& r, int vb, int nvb, int tid, int nthreads) {
  const int wz = (r.parts & YL_POOL_ZERO) ? r.F : 0, wx = (r.parts & YL_POOL_MAX) ? r.D : 0,
            wm = (r.parts & YL_POOL_MEAN) ? r.D : 0;
  const int W = wz + wx + wm;
  const long total = (long)r.P * W;
  for (long i = (long)vb * nthreads + tid; i < total; i += (long)nvb * nthreads) {
    const int p = (int)(i / W), c = (int)(i - (long)p * W);
    float* z = r.Z + (long)p * r.ldz;
    if (c < wz) { z[c] = 0.f; continue; }
    const bool is_max = c < wz + wx;
    const int k = is_max ? c - wz : c - wz - wx;
    const float* src = (is_max ? r.feats : r.fsup) + k;
    const int r0 = r.seg_ptr[p], r1 = r.seg_ptr[p + 1];
    float best = 0.f, sm = 0.f;
    bool any = false;
    int q = r0;
    for (; q + 8 <= r1; q += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(long)(q + j) * r.ld];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!any || v[j] > best) { best = v[j]; any = true; }
        sm += v[j];
      }
    }
    for (; q < r1; ++q) {
      const float v = src[(long)q * r.ld];
      if (!any || v > best) { best = v; any = true; }
      sm += v;
    }
    if (is_max) z[r.F + k] = best;
    else {
      const int cnt = r1 - r0;
      z[2 * r.F + r.D + k] = sm / (float)(cnt > 1 ? cnt : 1);
    }
  }
}
// The node side of the NEXT conv layer computed inside the edge launch (small graphs, node tiles of <= 16 nodes), so
// that a conv layer is ONE launch instead of two (k_gemm_nt_node3 was ~10 us of latency at N = 10 k):
//  * UV' / root': a tile owns its destination nodes, so once their rows of f_out are final it multiplies them by the next
//    layer's stacked [Wuv' ; Wr'] (192 x 64) — 12 column tiles x 16 v_mfma_f32_16x16x4_f32, B fragments prefetched from the
//    packed weight — and writes the next UV rows and the next root term;
//      Wp   Wp[(ct * 16 + ks) * 64 + l] = W'[ct * 16 + (l & 15)][4 * ks + (l >> 4)]   (coalesced B fragments)
//      bias [192] = [uvb' ; br'];  UV [N, 2C] of the next layer (NOT the buffer this launch gathers from), root = next f_out
//  * the node branch s' = relu(bn(s . Wn'^T)) of the next layer does not depend on this layer's messages at all: s_tiles
//    extra workgroups run it as 64 x 64 x 64 tiles on the edge kernel's own LDS tiles and MFMA loop.
struct EdgeNext {
  const float* Wp; const float* bias; float* UV; long ld_uv; float* root; long ld_root;
  const float* s_in; long ld_si; const float* Wn; const float* bn; const float* sn; const float* tn;
  float* s_out; long ld_so; int s_tiles;
};
// 0: the automatic choice is not the node-tile kernel; 1 / 4: node tiles with <= 16 / <= 64 nodes (edge.hip)
int yl_edge_tile_groups(int64_t N, int64_t E);
// nodes per workgroup of the node-tile edge kernels, fp32 and bf16 (edge.hip); 64 for a graph without edges
long yl_edge_tile_npt(long N, long E);
// yolat_edge_uv_mlp2_mean_eval_variant with an optional rider / next-layer node side (edge.hip): *rode = 1 when the
// launched kernel carried the rider, *did_next = 1 when it computed `next`; tiles_per_wg > 1: the several-tiles-per-workgroup
// kernel where the tiles hold <= 16 nodes (the throughput regime's shape, same results)
int yl_edge_uv_mlp2_mean_eval_impl(const float* UV, int64_t ld_uv, const int32_t* src_csr, const int32_t* dst_csr,
                                   const float* attr_csr, const int32_t* row_ptr, int64_t N, int64_t E, const float* Wc4,
                                   const float* b1, const float* s1, const float* t1, const float* W2, const float* b2,
                                   const float* s2, const float* t2, int64_t C, float* f_out, int64_t ld_fo, int variant,
                                   const PoolRider* rider, int* rode, const EdgeNext* next, int* did_next,
                                   yolat_stream_t stream, int tiles_per_wg = 1);
// yolat_fusion_pair_eval_x6 with an optional rider (fusion_x6.hip); slope_f / slope_s (both or none): the activation-aware
// instantiation for a leaky activation — `pool` then starts from yolat_pool_init_signed, not from zeros
int yl_fusion_pair_eval_x6_impl(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh, const uint16_t* Wm,
                                const uint16_t* Wl, const float* tfold, int64_t F, const int32_t* node_seg, float* pool,
                                int64_t ldpool, const float* S, int64_t lds, int64_t P, const uint16_t* Wsh,
                                const uint16_t* Wsm, const uint16_t* Wsl, const float* tsfold, float* Ys, int64_t ldys,
                                const PoolRider* rider, yolat_stream_t stream, const float* slope_f = nullptr,
                                const float* slope_s = nullptr);
// the same launch with the GEMM emulated by three half-precision products (fusion_f16x3.hip k_fusion_rows_f16x3): the weights
// as yolat_split_f16x2 gives them
int yl_fusion_pair_eval_f16x3_impl(const float* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wh, const uint16_t* Wl,
                                   const int32_t* Wexp, const float* tfold, int64_t F, const int32_t* node_seg, float* pool,
                                   int64_t ldpool, const float* S, int64_t lds, int64_t P, const uint16_t* Wsh,
                                   const uint16_t* Wsl, const int32_t* Wsexp, const float* tsfold, float* Ys, int64_t ldys,
                                   const PoolRider* rider, yolat_stream_t stream, const float* slope_f = nullptr,
                                   const float* slope_s = nullptr);
// what the two launches above share before the launch (fusion_x6.hip): the argument check — w_null / w_unaligned: the
// weights' NULL and alignment terms, ys_span32: P * ldys >= 2^32 is declined too — then the grid (row tiles of both
// problems, fx_plan's split of the node problem, the small problem's tn column groups of one tile, the workgroup count
// with the rider's) and the copy of a rider with blocks
struct FxPairGrid { int tm0, full, groups, ng, tm1, tn; unsigned total; PoolRider rider; };
int yl_fx_pair_setup(const float* A, int64_t lda, int64_t N, int64_t D, const float* tfold, int64_t F, const int32_t* node_seg,
                     float* pool, int64_t ldpool, const float* S, int64_t lds, int64_t P, const float* tsfold, float* Ys,
                     int64_t ldys, bool w_null, bool w_unaligned, bool ys_span32, const PoolRider* rider, const float* slope_f,
                     const float* slope_s, FxPairGrid* g);
// the fusion pair behind a row norm (rownorm.hip): does a batch of N nodes run the fused kernel (true) or the materialising
// route?  The descriptor's rn_route, or N >= YOLAT_RN_FUSED_MIN_ROWS when that is YOLAT_RN_ROUTE_AUTO: a function of the
// descriptor and N alone, so the workspace sizing and the forward always agree.
bool yl_rn_fused(const yolat_model_eval* m, int64_t N);
// k_pool_prepare restricted to `parts` (segment.hip)
int yl_pool_prepare_parts(const float* feats, const float* fsup, int64_t ld, int64_t D, int64_t F, const int32_t* seg_ptr,
                          int64_t P, float* Z, int64_t ldz, int parts, yolat_stream_t stream);
// stage profiler hooks (forward_eval.hip): HIP-event pair around one stage of a whole-forward entry point
bool yl_profile_on();
void yl_stage_begin(const char* name, double flops, double bytes, yolat_stream_t stream);
void yl_stage_end(yolat_stream_t stream);

// inputs of the one-launch conv stack (conv_local.hip): a prepared destination-sorted graph (row_ptr / src / dst / attr in
// CSR order), or — edge != nullptr — the raw COO list (attr in COO order) with per-proposal edge ranges eptr
struct YlLocalIn {
  const int32_t *row_ptr, *src, *dst; const float* attr; const int32_t* seg_ptr;
  const int64_t* edge; int64_t se, sc; const int32_t* eptr;
  int32_t* status;         // non-null: the caller vouched for the batch, a violation is reported as YOLAT_STATUS_NOT_LOCAL
};
// seg_ptr / node_seg / eptr of a COO batch grouped by proposal + YOLAT_LOC_* violations (conv_local.hip)
int yl_local_prep(const int64_t* edge, int64_t se, int64_t sc, const int64_t* bbox_idx, int64_t N, int64_t E, int64_t P,
                  int32_t* seg_ptr, int32_t* node_seg, int32_t* eptr, int32_t* status, int32_t* info, bool vouched,
                  hipStream_t st);

// The launch regime of the fp32 eval forward (forward_eval.hip, yolat_eval_regime_observe): one forward at a time, or
// several in flight on several streams.  Every shape a regime selects computes bit-identical results.
#define YL_REGIME_LATENCY 0
#define YL_REGIME_THROUGHPUT 1
// yolat_graph_prepare with an optional co-scheduled node-side GEMM set (graph.hip); `regime` plans k_prep_small
int yl_graph_prepare_impl(const int64_t* edge, int64_t stride_e, int64_t stride_c, const float* e_attr,
                          const int64_t* bbox_idx, int64_t E, int64_t N, int64_t P, int32_t* row_ptr, int32_t* perm,
                          int32_t* src_csr, int32_t* dst_csr, float* attr_csr, int32_t* seg_ptr, int32_t* node_seg,
                          int32_t* work, int32_t* status, const NodeUv* extra, bool primed, yolat_stream_t stream,
                          int regime = YL_REGIME_LATENCY);

// edge stage of the bf16 forward on folded weights (edge_chain.hip): variant 0 = automatic, 1 = node tiles, 2 = chained waves
int yl_edge_uv_mlp2_mean_bf16_impl(const uint16_t* UV, long ld_uv, const int* src, const int* dst, const float* attr,
                                   const int* row_ptr, long N, long E, const float* Wc4, const float* s1,
                                   const uint16_t* W2f, const float* t2f, const float* root, long ld_r, uint16_t* f_out,
                                   long ld_fo, int variant, hipStream_t st, YlGate gate = YlGate{nullptr, 0});
// the bf16 tile GEMM (hgemm.hpp) for a caller in another file: bf16_eval.hip holds every k_hgemm instance.  a_scale given:
// A's rows pass the producer's BatchNorm (a_scale, a_shift) and the floor while staging (HProOp)
int yl_launch_hgemm(const HOp& A, const float* a_scale, const float* a_shift, float a_floor, const HOp& B, const Epilogue& ep,
                    long M, long N, long K, hipStream_t st);
// can the one-launch conv stack run this model at all (conv_local.hip)
bool yl_conv_local_model_ok(const yolat_model_eval_bf16* mh);
// the one-launch conv stack; *flag = flag_val when the batch turns out not to be proposal-local (conv_local.hip)
int yl_conv_local_bf16(const yolat_model_eval_bf16* mh, const void* pack, const float* x, int64_t ldx, const YlLocalIn& in,
                       int64_t N, int64_t E, int64_t P, uint16_t* feats, int64_t ld_feats, float* Z, int64_t ldz, int32_t* flag,
                       int32_t flag_val, hipStream_t st);
// bf16 fusion block with the per-proposal max, nodes and proposals in one launch (fusion_h8.hip); force_groups > 0
// replaces the planned column groups of the N-row problem, groups_ng receives that problem's (groups, ng); slope_f /
// slope_s (both or none): the activation-aware instantiation for a leaky activation — `pool` then starts from
// yolat_pool_init_signed, not from zeros
int yl_hfusion_rows8(const uint16_t* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wf, const float* tf,
                     const int32_t* seg, float* pool, int64_t ld_pool, int64_t F, const float* As, int64_t lda_s, int64_t P,
                     const uint16_t* Wfs, const float* tfs, float* sup_out, int64_t ld_sup, hipStream_t st,
                     int force_groups = 0, int* groups_ng = nullptr, const float* slope_f = nullptr,
                     const float* slope_s = nullptr);
// the same pair behind a ROW norm (fusion_h8_rn.hip, k_hfusion_rows8_rn): Wf / Wfs centred over their F outputs before the
// bf16 rounding, tf / tfs the centred bias, gamma / beta both NULL for the instance norm; `pool` starts from zeros.
// yl_hfusion_rows8_rn_ok: the shapes and alignments the launch takes (everything else is declined before anything is written)
bool yl_hfusion_rows8_rn_ok(const void* A, int64_t lda, int64_t N, int64_t D, const void* Wf, int64_t F, const void* As,
                            int64_t lda_s, int64_t P, const void* Wfs);
int yl_hfusion_rows8_rn(const uint16_t* A, int64_t lda, int64_t N, int64_t D, const uint16_t* Wf, const float* tf,
                        const float* gamma_f, const float* beta_f, const int32_t* seg, float* pool, int64_t ld_pool, int64_t F,
                        const float* As, int64_t lda_s, int64_t P, const uint16_t* Wfs, const float* tfs, const float* gamma_s,
                        const float* beta_s, float* sup_out, int64_t ld_sup, float eps, hipStream_t st);
// Z (bf16, a buffer of its own) = relu(rownorm(Y) * gamma + beta) of fp32 rows, one rounding (fusion_h8_rn.hip)
int yl_rownorm_act_h(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* gamma, const float* beta, float eps,
                     uint16_t* Z, int64_t ldz, hipStream_t st);
// per-proposal maximum of <= 2^20 materialised ReLU'd rows merged into the zero-started pool (rownorm.hip, k_rn_range_max)
int yl_rn_range_max(const float* Zr, int64_t ldz, int64_t rows, int64_t F, const int32_t* node_seg, int64_t P, float* pool,
                    int64_t ldpool, hipStream_t st);
// the weight gradient of a wide Linear on the bf16x6 GEMM: worthwhile?, its workspace, the launch (gemm_x6.hip)
bool yl_bwd_w_x6_ok(int64_t M, int64_t Nout, int64_t K);
size_t yl_bwd_w_x6_work_elems(int64_t M, int64_t Nout, int64_t K);
int yl_bwd_w_x6(const float* dY, int64_t lddy, int64_t M, int64_t Nout, const float* A, int64_t lda, int64_t K, float* dW,
                int64_t lddw, float* db, int accumulate_db, float* work, hipStream_t st);
// per-workgroup clock stamps of k_gemm_nt_sk_dma, nullptr unless a measurement asked for them (dense.hip)
long long* yl_gemm_sk_dma_stamps();
// switch of the LDS-DMA skinny GEMM and its stamps; exported for tools and tests, not part of the C ABI header (dense.hip)
extern "C" void yolat_debug_gemm_sk_dma(int on, long long* stamps);
// yolat_edge_uv_mlp2_mean_eval_mt with an EdgeNext built from plain arguments (s_in == nullptr: no node-branch tiles), the way
// the eval forward's chain launches it; exported for tools and tests, not part of the C ABI header (edge.hip)
extern "C" int yolat_debug_edge_uv_mlp2_mean_eval_next(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                                       const int32_t* dst_csr, const float* attr_csr, const int32_t* row_ptr,
                                                       int64_t N, int64_t E, const float* Wc4, const float* b1, const float* s1,
                                                       const float* t1, const float* W2, const float* b2, const float* s2,
                                                       const float* t2, int64_t C, float* f_out, int64_t ld_fo, int tiles_per_wg,
                                                       const float* Wp, const float* bias, float* UVn, int64_t ld_uvn,
                                                       float* root, int64_t ld_root, const float* s_in, int64_t ld_si,
                                                       const float* Wn, const float* bn, const float* sn, const float* tn,
                                                       float* s_out, int64_t ld_so, int* did_next, yolat_stream_t stream);
// The last two classifier layers of the fp32 eval forward as one launch (cls_tail.hip): layer 2 on the split-K tiles of
// k_gemm_nt_sk, layer 3 as per-tile partial products that the last workgroup of a row tile sums.  yl_cls_tail_on: the
// YOLAT_CLS_TAIL_FOLD switch; yl_cls_tail_shape_ok: a function of the sizes alone, so the workspace sizing and the forward
// agree; tickets (yl_cls_tail_ticket_elems words, zero before the launch unless !primed, zero after it) and slabs
// (yl_cls_tail_slab_elems floats, 16-byte aligned) are the caller's.  c2_dbg != nullptr: the c2 tile is stored as well.
bool yl_cls_tail_on();
bool yl_cls_tail_shape_ok(int64_t P, int64_t H1, int64_t H2, int64_t n_classes);
size_t yl_cls_tail_ticket_elems(int64_t P);
size_t yl_cls_tail_slab_elems(int64_t P, int64_t H2);
int yl_cls_tail_eval_impl(const float* c1, int64_t ldc1, int64_t P, int64_t H1, const float* W2, int64_t ldw2, const float* b2,
                          const float* s2, const float* t2, int64_t H2, const float* W3, int64_t ldw3, const float* b3,
                          int64_t n_classes, float* logits, int64_t ld_logits, uint32_t* tickets, float* slabs, bool primed,
                          float* c2_dbg, int64_t ld_dbg, yolat_stream_t stream);
// layers 2 + 3 as an op over one work buffer, routed like the forward (fold or two launches); exported for tools and tests, not part of the C ABI header (cls_tail.hip)
extern "C" size_t yolat_debug_cls_tail_work_bytes(int64_t P, int64_t H2);
extern "C" int yolat_debug_cls_tail_eval(const float* c1, int64_t ldc1, int64_t P, int64_t H1, const float* W2, int64_t ldw2,
                                         const float* b2, const float* s2, const float* t2, int64_t H2, const float* W3,
                                         int64_t ldw3, const float* b3, int64_t n_classes, float* logits, int64_t ld_logits,
                                         void* work, int primed, float* c2_dbg, int64_t ld_dbg, int* folded,
                                         yolat_stream_t stream);
// Stages of the bf16-storage eval forward as ops of their own, launched the way yolat_forward_eval_bf16 launches them
// (bf16_eval.hip); exported for tools and tests, not part of the C ABI header.
//   fusion pair: the forward's route on D and the fold pointers.  Z [P, ldz] in the forward's column layout (pooled max at
//     0:F, zero before the call; super output at F+D:2F+D; super input, fp32, at 2F+D:2F+2D).  force_groups > 0 replaces
//     the planned column groups of the rows routes.  *route: 0 = k_hfusion_rows8, 1 = k_hfusion_rows<1,128>,
//     2 = k_hfusion_rows<1,256>, 3 = k_hgemm_two<1>, 4 = k_hgemm_two<2>; groups_ng[2] = (groups, ng) of the node problem
//     ((column tiles, 1) on the tile routes).
extern "C" int yolat_debug_fusion_pair_eval_bf16(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                 const int32_t* node_seg, float* Z, int64_t ldz, int64_t P, int64_t F,
                                                 const uint16_t* Wf, const uint16_t* Wfs, const float* bf, const float* sf,
                                                 const float* tf, const float* bfs, const float* sfs, const float* tfs,
                                                 const uint16_t* Wf_fold, const float* tf_fold, const uint16_t* Wfs_fold,
                                                 const float* tfs_fold, int force_groups, int* route, int* groups_ng,
                                                 yolat_stream_t stream);
//   pooling prologue: Z[p, 0:F] = 0, Z[p, F:F+D] = max(feats rows), Z[p, 2F+D:2F+2D] = mean(fsup rows), ungated, in the
//     forward's chunks of 65535 proposals
extern "C" int yolat_debug_pool_prepare_bf16(const uint16_t* feats, const uint16_t* fsup, int64_t ld, int64_t D, int64_t F,
                                             const int32_t* seg_ptr, int64_t P, float* Z, int64_t ldz, yolat_stream_t stream);
//   node side of a conv layer > 0 (C = Cin = 64): UV [N, 128] bf16 = (f_in . Wuv^T) * uv_scale + uv_shift, root [N, 64] fp32 =
//     f_in . Wr^T + br, s_out bf16 = relu((s_in . Wn^T + bn) * sn + tn)
extern "C" int yolat_debug_node_uv_eval_bf16(const uint16_t* f_in, int64_t ld_f, const uint16_t* s_in, int64_t ld_s, int64_t N,
                                             const uint16_t* Wuv, const uint16_t* Wr, const uint16_t* Wn,
                                             const float* uv_scale, const float* uv_shift, const float* br, const float* bn,
                                             const float* sn, const float* tn, uint16_t* UV, float* root, uint16_t* s_out,
                                             int64_t ld_so, yolat_stream_t stream);
//   the classifier's GEMM: Y = epi(A . W^T), A fp32 rows rounded while staging (a_f32 != 0) or bf16 rows, W [Nout, K] bf16,
//     Y bf16 (y_bf16 != 0) or fp32; scale and shift both or none.  *tile_form: 0 = k_hgemm<1,1>, 1 = k_hgemm<1,2>
extern "C" int yolat_debug_hgemm_eval_bf16(const void* A, int a_f32, int64_t lda, int64_t M, int64_t K, const uint16_t* W,
                                           int64_t ldw, int64_t Nout, const float* bias, const float* scale,
                                           const float* shift, int relu, void* Y, int y_bf16, int64_t ldy, int* tile_form,
                                           yolat_stream_t stream);
//   the two stages above for a leaky model (act.hip): the slopes by address, as every launch reads them.  Fusion pair: the
//     start values of Z[:, 0:F] are written by the call (seg_ptr [P+1]); *route: 0 = yolat_pool_init_signed + the ACT
//     instantiation of k_hfusion_rows8 (D in {64, 128}, F % 64 == 0, fold pointers given), 5 = the materialising form for
//     every other shape on `work` (yolat_fusion_pair_eval_act_work_elems(N, F) floats; groups_ng = (column ranges, tiles per
//     range)).  Tile GEMM: Y = act(epi(A . W^T)) computed in fp32 before a bf16 store
extern "C" int yolat_debug_fusion_pair_eval_bf16_act(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                     const int32_t* node_seg, const int32_t* seg_ptr, float* Z, int64_t ldz,
                                                     int64_t P, int64_t F, const uint16_t* Wf, const uint16_t* Wfs,
                                                     const float* bf, const float* sf, const float* tf, const float* bfs,
                                                     const float* sfs, const float* tfs, const uint16_t* Wf_fold,
                                                     const float* tf_fold, const uint16_t* Wfs_fold, const float* tfs_fold,
                                                     const float* slope_f, const float* slope_s, float* work,
                                                     int force_groups, int* route, int* groups_ng, yolat_stream_t stream);
extern "C" int yolat_debug_hgemm_eval_bf16_act(const void* A, int a_f32, int64_t lda, int64_t M, int64_t K, const uint16_t* W,
                                               int64_t ldw, int64_t Nout, const float* bias, const float* scale,
                                               const float* shift, const float* slope, void* Y, int y_bf16, int64_t ldy,
                                               int* tile_form, yolat_stream_t stream);
//   the fusion pair and the classifier norm behind a ROW norm (--norm layer / instance; fusion_stage_rn, fusion_h8_rn.hip).
//     Fusion pair: Z as above, the pooled max zero before the call; gamma / beta [F] of the two sites, all four NULL for the
//     instance norm; rn_route YOLAT_RN_ROUTE_*.  *route: 6 = k_hfusion_rows8_rn on the CENTRED fold weights (D in {64, 128}, the
//     four fold pointers given, rn_route not MATERIALISE), 7 = the materialising form on `work`
//     (yolat_fusion_pair_eval_rn_work_elems(N, F) floats; groups_ng = (row ranges, column tiles)) with the plain Wf / Wfs and
//     bf / bfs.  Row norm: Z [M, ldz] bf16 = relu(rownorm(Y) gamma + beta) of fp32 rows, one rounding; Z must not overlap Y
extern "C" int yolat_debug_fusion_pair_eval_bf16_rn(const uint16_t* feats, int64_t ld, int64_t N, int64_t D,
                                                    const int32_t* node_seg, float* Z, int64_t ldz, int64_t P, int64_t F,
                                                    const uint16_t* Wf, const uint16_t* Wfs, const float* bf, const float* bfs,
                                                    const uint16_t* Wf_fold, const float* tf_fold, const uint16_t* Wfs_fold,
                                                    const float* tfs_fold, const float* gamma_f, const float* beta_f,
                                                    const float* gamma_s, const float* beta_s, float eps, int rn_route,
                                                    float* work, int* route, int* groups_ng, yolat_stream_t stream);
extern "C" int yolat_debug_rownorm_act_bf16(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* gamma,
                                            const float* beta, float eps, uint16_t* Z, int64_t ldz, yolat_stream_t stream);
