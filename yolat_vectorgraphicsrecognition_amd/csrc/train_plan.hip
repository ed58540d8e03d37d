// train_plan.hip — the training step as ONE native call (round 6): graph preparation + forward + loss + backward
// (+ Adam) enqueued from C on two streams, exactly the schedule engine.py issues from Python (same kernels, same operands,
// same order per stream -> bit-identical losses, gradients and parameters), without ~150-230 ctypes calls, tensor
// allocations and record_stream marks per step on the host.
//
// Reference: the loop body of cad_recognition/train.py:263-284 (forward, loss, backward, optimizer.step) over
// SparseCADGCN.forward (architecture3cc_rpn_gp_iter2.py:44-71,106-137), AttrRelativeEdgeConvGlobalPool2
// (gcn_lib/sparse/torch_vertex.py:288-341), MLP (torch_nn.py:50-71), DetectionLoss (arch:358-379), torch.optim.Adam
// (train.py:212).  Every launch below goes through the library's own C entry points (include/yolat_hip.h) — this file is
// the HOST schedule only; the kernels are where they were.
//
// Covered: the reference recipe's shapes on the default schedule of engine.py — n_filters 64, n_blocks_out 2 (fusion dims
// 128: the fused fusion block), Linear biases and BatchNorm everywhere, no dropout, E >= N (the factorised backward of the
// first edge Linear), the softmax / CrossEntropy head or the sigmoid / BCELoss head of classifier != 'softmax' (half bit 4:
// yolat_sigmoid_bce in place of yolat_softmax_ce, nothing else changes) — fp32 and bf16 storage of the per-edge tensors, and the "bf16_dense"
// precision (half bit 2: fusion_block, fusion_block_super and prediction_cls.0 / .1 on the bf16-operand kernels of
// bf16_train.hip and the _bf16 fusion entry points, as engine.py issues them for that mode; needs F % 64 == 0,
// H1 % 32 == 0, H2 % 32 == 0 and 16-byte aligned weights of those layers).  Anything else returns YOLAT_E_UNSUPPORTED
// and the caller keeps the Python schedule (trainer.Trainer does).  Every such decision is taken in precheck(), in front
// of the first launch: UNSUPPORTED means nothing was enqueued.  A failure behind it joins the side stream and is never
// reported as UNSUPPORTED (yolat_train_step, at the end of this file).
//
// Streams.  `side` != NULL: the weight gradients and the node branches run on it beside the dX chain, forked behind an
// event on `stream` at every hand-over and joined in front of the classifier, before the head bucket is declared complete
// and at the end of the backward — engine._on_side / _join_side.  The side stream also takes what the Python schedule
// leaves on the main one although nothing on the critical path waits for it: weight-only / graph-only preparation at the
// start of the step, the pooling of feats / the node branches and fusion_block_super beside the fusion block (forward),
// fusion_block_super's backward and the per-proposal mean's beside the fusion block's backward.  Same kernels, same
// operands, so the results stay bit-identical; only WHERE a launch waits changes.  Every temporary has its own range of
// the workspace (nothing is recycled inside a step), so the two streams never share scratch.
//
// Phases (for the data-parallel exchange, which stays with the caller's process group): 1 = everything up to the point
// where the gradients of the fusion blocks and the classifier (the "head" bucket, 93 % of the bytes) are final on `stream`;
// 2 = the conv layers' backward; 4 = Adam.  The caller issues its all-reduces between the calls.
#include "base.hpp"
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

namespace {

constexpr int TP_MAXL = YOLAT_MAX_LAYERS;

// the model's widths: C per conv layer, D = concat of the output layers, ZW = width of the classifier's input Z
struct Dims {
  long C, F, D, ZW, L, lo, K, H1, H2;
  explicit Dims(const yolat_train_model* m)
      : C(m->C), F(m->F), D(C * m->n_blocks_out), ZW(2 * (F + D)), L(m->n_blocks), lo(L - m->n_blocks_out), K(m->n_classes),
        H1(m->H1), H2(m->H2) {}
};

// BatchNorm coefficients of one layer as yolat_bn_finalize leaves them, from a [4C] block: scale | shift | mean | invstd
struct Coef {
  float* scale; float* shift; float* mean; float* invstd;
  Coef(float* c, long C) : scale(c), shift(c + C), mean(c + 2 * C), invstd(c + 3 * C) {}
};

struct ConvBuf {
  bool fact_fwd, half;
  float* f_tmp; float* s_tmp;              // outputs of layers below the concat (slot < 0)
  void* H1; void* H2; float* st1; float* st2; float* c1; float* c2;
  float* wuv; float* wc4; float* uv; uint16_t* wwork_f;
  // node branch: statistics, coef [4C]; scale / shift of an output layer live in its slice of sup_coef (the per-proposal
  // mean reads all output layers' as one vector), of a layer below the concat in cn
  float* st_n; float* cn; float* cn_scale; float* cn_shift;
  // backward
  void* dA1; float* coef2; float* coef1; float* w_stats; float* w_l2; float* dUV; float* dwc4; float* w_apply;
  float* wuv_b; float* wc4_b; float* dwuv; float* w_dwuv; float* w_root; float* w_node_bn; float* w_node_w;
  float* dx_tmp; float* dxn_tmp;
  Coef node_coef(long C) const {
    Coef k(cn, C);
    k.scale = cn_scale; k.shift = cn_shift;
    return k;
  }
};

struct TrainBuf {
  // graph
  int* row_ptr; int* perm; int* src; int* dst; float* attr; int* zblock; int* seg_ptr; int* node_seg; int* gwork;
  int* col_ptr; int* slots; int* cwork; float* inv_deg;
  float* feats; float* fsup; float* sup_coef;
  ConvBuf cv[TP_MAXL];
  float* Z; int* arg_feat; float* fus_coef; float* fus_saved; float* fus_work;
  float* fs_y; float* fs_st; float* fs_c;
  float* c1y; float* c1st; float* c1c; uint16_t* c1pack;
  float* c2y; float* c2st; float* c2c;
  float* dl; float* ce_work;
  // backward
  float* d2; float* d1; float* dZ; float* d_fsup; float* d_feats;
  float* w3; float* w2bn; float* w2w; uint16_t* p2; float* x2w; float* w1bn; float* w1w; uint16_t* p1; float* x1w;
  float* wfsbn; float* wfsw;
  float* bt_w2; float* bt_w1; float* bt_wfs;     // "bf16_dense": split-K / column-sum scratch of the three dW GEMMs
  size_t bytes;
};

// a scratch query that answers 0 still takes one element: every piece keeps an address (and a 256-byte slot) of its own
size_t nz(size_t n) { return n > 0 ? n : 1; }

// The workspace of one step: a pure function of (m, N, E, P, ws) — phases issued as separate calls find the same ranges.
TrainBuf carve(const yolat_train_model* m, long N, long E, long P, void* ws) {
  Carver c{reinterpret_cast<char*>(ws), 0};
  TrainBuf b;
  memset(&b, 0, sizeof b);
  const Dims d(m);
  const long C = d.C, F = d.F, D = d.D, ZW = d.ZW, K = d.K, Ee = E > 0 ? E : 1;
  b.row_ptr = c.take<int>(N + 1); b.perm = c.take<int>(Ee); b.src = c.take<int>(Ee); b.dst = c.take<int>(Ee);
  b.attr = c.take<float>(Ee * 4);
  const long n_seg = (P + 1 + 3) / 4 * 4;
  b.zblock = c.take<int>(n_seg + N);
  b.seg_ptr = b.zblock; b.node_seg = b.zblock + n_seg;
  b.gwork = c.take<int>(nz(yolat_graph_work_elems(N, E)));
  b.col_ptr = c.take<int>(N + 1); b.slots = c.take<int>(Ee); b.cwork = c.take<int>(nz(yolat_csc_work_elems(N)));
  b.inv_deg = c.take<float>(N);
  b.feats = c.take<float>(N * D); b.fsup = c.take<float>(N * D); b.sup_coef = c.take<float>(2 * D);
  for (long l = 0; l < d.L; ++l) {
    ConvBuf& v = b.cv[l];
    const long Cin = m->conv[l].Cin, slot = l - d.lo;
    v.fact_fwd = C == 64 && (double)E >= 2.0 * (double)N;
    v.half = (m->half & 3) != 0 && v.fact_fwd;
    const size_t es = v.half ? 2 : 4;
    v.f_tmp = slot < 0 ? c.take<float>(N * C) : nullptr;
    v.s_tmp = slot < 0 ? c.take<float>(N * C) : nullptr;
    v.H1 = c.take<char>(Ee * C * es); v.H2 = c.take<char>(Ee * C * es);
    v.st1 = c.take<float>(nz(yolat_bn_stats_elems(Ee, C))); v.st2 = c.take<float>(nz(yolat_bn_stats_elems(Ee, C)));
    v.c1 = c.take<float>(4 * C); v.c2 = c.take<float>(4 * C);
    v.wuv = c.take<float>(2 * C * Cin); v.wc4 = c.take<float>(C * 4); v.uv = c.take<float>(N * 2 * C);
    v.wwork_f = c.take<uint16_t>(C * C);
    v.st_n = c.take<float>(nz(yolat_bn_stats_elems(N, C))); v.cn = c.take<float>(4 * C);
    v.cn_scale = slot >= 0 ? b.sup_coef + slot * C : v.cn;
    v.cn_shift = slot >= 0 ? b.sup_coef + D + slot * C : v.cn + C;
    v.dA1 = c.take<char>(Ee * C * es); v.coef2 = c.take<float>(2 * C); v.coef1 = c.take<float>(2 * C);
    v.w_stats = c.take<float>(nz(yolat_bn_csr_work_elems(Ee, C)));
    v.w_l2 = c.take<float>(nz(yolat_bn_csr_l2_bwd_work_elems()));
    v.dUV = c.take<float>(N * 2 * C); v.dwc4 = c.take<float>(C * 4);
    v.w_apply = c.take<float>(nz(yolat_bn_apply_edge_sums_work_elems(N)));
    v.wuv_b = c.take<float>(2 * C * Cin); v.wc4_b = c.take<float>(C * 4);
    v.dwuv = c.take<float>(2 * C * Cin); v.w_dwuv = c.take<float>(nz(yolat_linear_bwd_w_work_elems(N, 2 * C, Cin)));
    v.w_root = c.take<float>(nz(yolat_linear_bwd_w_work_elems(N, C, Cin)));
    v.w_node_bn = c.take<float>(nz(yolat_bn_bwd_work_elems(N, C)));
    v.w_node_w = c.take<float>(nz(yolat_linear_bwd_w_work_elems(N, C, Cin)));
    // gradients flowing into a layer below the concat: one buffer each (d_f_next / d_s_next of engine.model_bwd)
    v.dx_tmp = (l > 0 && slot - 1 < 0) ? c.take<float>(N * Cin) : nullptr;
    v.dxn_tmp = (l > 0 && slot - 1 < 0) ? c.take<float>(N * Cin) : nullptr;
  }
  b.Z = c.take<float>(P * ZW); b.arg_feat = c.take<int>(P * D);
  b.fus_coef = c.take<float>(4 * F); b.fus_saved = c.take<float>(nz(yolat_fusion_pool_train_saved_elems(D, F, P)));
  b.fus_work = c.take<float>(nz(yolat_fusion_pool_train_work_elems(N, D, F, P)));
  b.fs_y = c.take<float>(P * F); b.fs_st = c.take<float>(nz(yolat_bn_stats_elems(P, F))); b.fs_c = c.take<float>(4 * F);
  b.c1y = c.take<float>(P * d.H1); b.c1st = c.take<float>(nz(yolat_bn_stats_elems(P, d.H1))); b.c1c = c.take<float>(4 * d.H1);
  b.c1pack = c.take<uint16_t>(nz(yolat_gemm_x6_packed_elems(d.H1, ZW)));
  b.c2y = c.take<float>(P * d.H2); b.c2st = c.take<float>(nz(yolat_bn_stats_elems(P, d.H2))); b.c2c = c.take<float>(4 * d.H2);
  b.dl = c.take<float>(P * K); b.ce_work = c.take<float>(nz(std::max(yolat_softmax_ce_work_elems(P), yolat_bce_work_elems(P))));
  b.d2 = c.take<float>(P * d.H2); b.d1 = c.take<float>(P * d.H1); b.dZ = c.take<float>(P * ZW);
  b.d_fsup = c.take<float>(N * D); b.d_feats = c.take<float>(N * D);
  b.w3 = c.take<float>(nz(yolat_linear_bwd_w_work_elems(P, K, d.H2)));
  b.w2bn = c.take<float>(nz(yolat_bn_bwd_work_elems(P, d.H2)));
  b.w2w = c.take<float>(nz(yolat_linear_bwd_w_work_elems(P, d.H2, d.H1)));
  b.p2 = c.take<uint16_t>(nz(yolat_gemm_x6_packed_elems(d.H1, d.H2)));
  b.x2w = c.take<float>(yolat_gemm_x6_work_elems(P, d.H1, d.H2) + 1);
  b.w1bn = c.take<float>(nz(yolat_bn_bwd_work_elems(P, d.H1)));
  b.w1w = c.take<float>(nz(yolat_linear_bwd_w_work_elems(P, d.H1, ZW)));
  b.p1 = c.take<uint16_t>(nz(yolat_gemm_x6_packed_elems(ZW, d.H1)));
  b.x1w = c.take<float>(yolat_gemm_x6_work_elems(P, ZW, d.H1) + 1);
  b.wfsbn = c.take<float>(nz(yolat_bn_bwd_work_elems(P, F))); b.wfsw = c.take<float>(nz(yolat_linear_bwd_w_work_elems(P, F, D)));
  if (m->half & 2) {
    b.bt_w2 = c.take<float>(nz(yolat_bt_linear_bwd_w_work_elems(P, d.H2, d.H1)));
    b.bt_w1 = c.take<float>(nz(yolat_bt_linear_bwd_w_work_elems(P, d.H1, ZW)));
    b.bt_wfs = c.take<float>(nz(yolat_bt_linear_bwd_w_work_elems(P, F, D)));
  }
  b.bytes = c.off + 256;
  return b;
}

int model_ok(const yolat_train_model* m) {
  if (!m || !m->param_base || !m->grad_base) return YOLAT_E_INVALID;
  if (m->n_blocks < 1 || m->n_blocks > TP_MAXL || m->n_blocks_out < 1 || m->n_blocks_out > m->n_blocks || m->n_classes < 1)
    return YOLAT_E_INVALID;
  if (m->C != 64 || m->n_blocks_out != 2 || m->F <= 0 || m->F % 4 != 0 || m->H1 <= 0 || m->H2 <= 0) return YOLAT_E_UNSUPPORTED;
  if ((m->half & ~7) != 0) return YOLAT_E_INVALID;
  if ((m->half & 2) && (m->F % 64 != 0 || m->H1 % 32 != 0 || m->H2 % 32 != 0)) return YOLAT_E_UNSUPPORTED;
  auto lin_ok = [](const yolat_train_lin& l) { return l.W != nullptr && l.b != nullptr; };
  auto bn_ok = [](const yolat_train_bn& b) { return b.gamma != nullptr && b.beta != nullptr; };
  for (int l = 0; l < m->n_blocks; ++l) {
    const yolat_train_conv& cv = m->conv[l];
    if (cv.Cin < 1 || (l > 0 && cv.Cin != 64)) return YOLAT_E_UNSUPPORTED;
    if (!lin_ok(cv.nn0) || !bn_ok(cv.bn1) || !lin_ok(cv.nn3) || !bn_ok(cv.bn4) || !lin_ok(cv.lin_r) || !lin_ok(cv.node) ||
        !bn_ok(cv.bn_node))
      return YOLAT_E_UNSUPPORTED;
  }
  if (!lin_ok(m->fus) || !bn_ok(m->fus_bn) || !lin_ok(m->fus_s) || !bn_ok(m->fus_s_bn) || !lin_ok(m->c1) || !bn_ok(m->c1_bn) ||
      !lin_ok(m->c2) || !bn_ok(m->c2_bn) || !lin_ok(m->c3))
    return YOLAT_E_UNSUPPORTED;
  return 0;
}

// the arguments of yolat_train_step
struct Step {
  const yolat_train_model* m; const float* x; long ldx; const int64_t* edge; long stride_e, stride_c; const float* e_attr;
  const int64_t* bbox_idx; const yolat_graph_csr* g; const int64_t* labels; long N, E, P; float* logits; long ld_logits;
  float* loss; void* workspace; size_t workspace_bytes; int32_t* status; const yolat_adam_args* adam; int phases;
};

// Every decision to reject (YOLAT_E_INVALID) or to decline (YOLAT_E_UNSUPPORTED) a step, in front of the first launch;
// carves the workspace on the way.
int precheck(const Step& a, TrainBuf* b) {
  const yolat_train_model* m = a.m;
  YL_TRY(model_ok(m));
  if (!a.x || !a.labels || !a.logits || !a.loss || !a.workspace || !a.status || a.N <= 0 || a.E <= 0 || a.P <= 0 ||
      (a.phases & 7) == 0)
    return YOLAT_E_INVALID;
  if (!a.g && (!a.edge || !a.e_attr || !a.bbox_idx)) return YOLAT_E_INVALID;
  if ((a.phases & 4) && (!a.adam || !a.adam->exp_avg || !a.adam->exp_avg_sq || a.adam->n <= 0 || a.adam->step < 1))
    return YOLAT_E_INVALID;
  if (a.E < a.N || a.N >= (1LL << 30) || a.E >= (1LL << 30)) return YOLAT_E_UNSUPPORTED;   // (E >= N: the factorised backward)
  if (a.ld_logits < m->n_classes) return YOLAT_E_INVALID;
  *b = carve(m, a.N, a.E, a.P, a.workspace);
  if (b->bytes > a.workspace_bytes || (((uintptr_t)a.workspace) & 255) != 0) return YOLAT_E_INVALID;
  // the fused backward kernels read parameter / coefficient vectors with 16-byte loads (engine.conv_bwd's `aligned` gate)
  for (long l = 0; l < m->n_blocks; ++l)
    if (!yl_aligned16(m->conv[l].nn3.W)) return YOLAT_E_UNSUPPORTED;
  if (!yl_aligned16(m->fus.W)) return YOLAT_E_UNSUPPORTED;
  // "bf16_dense": the bf16-operand GEMMs read the weights in 16-byte pieces (ops._bt_aligned copies an unaligned view)
  if ((m->half & 2) && !(yl_aligned16(m->fus_s.W) && yl_aligned16(m->c1.W) && yl_aligned16(m->c2.W))) return YOLAT_E_UNSUPPORTED;
  if (a.g) {
    const yolat_graph_csr* g = a.g;
    if (!g->row_ptr || !g->src || !g->dst || !g->attr || !g->seg_ptr || !g->node_seg) return YOLAT_E_INVALID;
    if (!yl_aligned16(g->attr)) return YOLAT_E_UNSUPPORTED;      // (the workspace's own attr is 256-byte aligned)
  }
  return 0;
}

__global__ void k_tp_zero(int* p, long n, int* status) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
  if (i == 0 && status) *status = 0;
}
struct NbtList { long long* p[4 * TP_MAXL + 8]; int n; };
__global__ void k_tp_nbt(NbtList l) {
  if ((int)threadIdx.x < l.n && l.p[threadIdx.x] != nullptr) *l.p[threadIdx.x] += 1;
}

// two streams, forked / joined through events (engine._on_side / _join_side)
struct Streams {
  hipStream_t main, side;
  hipEvent_t ev_fork, ev_join;
  bool dirty;
  hipStream_t fork() {                 // the side stream, ordered behind everything issued on main so far
    if (!side) return main;
    (void)hipEventRecord(ev_fork, main);
    (void)hipStreamWaitEvent(side, ev_fork, 0);
    dirty = true;
    return side;
  }
  void join() {                        // main waits for the side-stream work issued so far
    if (!side || !dirty) return;
    (void)hipEventRecord(ev_join, side);
    (void)hipStreamWaitEvent(main, ev_join, 0);
    dirty = false;
  }
};

// the two events of a (main, side) pair, created once per process and pair of streams.  An entry is published complete and
// never destroyed: a step of another thread may be recording into it.
struct EvCache { hipStream_t m, s; hipEvent_t f, j; };
std::vector<EvCache> g_ev;
std::mutex g_ev_mu;
bool events_for(Streams* S) {
  std::lock_guard<std::mutex> lock(g_ev_mu);       // (trainers on several devices / host threads share the table)
  for (const EvCache& e : g_ev)
    if (e.m == S->main && e.s == S->side) { S->ev_fork = e.f; S->ev_join = e.j; return true; }
  EvCache e{S->main, S->side, nullptr, nullptr};
  if (hipEventCreateWithFlags(&e.f, hipEventDisableTiming) != hipSuccess) return false;
  if (hipEventCreateWithFlags(&e.j, hipEventDisableTiming) != hipSuccess) {
    (void)hipEventDestroy(e.f);
    return false;
  }
  g_ev.push_back(e);
  S->ev_fork = e.f; S->ev_join = e.j;
  return true;
}

inline float* grad_of(const yolat_train_model* m, const float* p) {
  return p ? m->grad_base + (p - m->param_base) : nullptr;
}

int finalize(const float* stats, long M, long C, const yolat_train_bn& bn, const Coef& k, hipStream_t s) {
  return yolat_bn_finalize(stats, M, C, bn.gamma, bn.beta, bn.running_mean, bn.running_var, bn.momentum, bn.eps, k.mean, k.invstd,
                           k.scale, k.shift, s);
}

// an activation the consumer reads through the producer's BatchNorm + ReLU (engine.Lazy)
struct Lazy { const float* t; long ld; const float* scale; const float* shift; int relu; };

// One Linear (+ BatchNorm1d + ReLU) block of the model with the workspace ranges it uses: what engine.lbr_fwd saves.
struct Lbr {
  const yolat_train_lin* lin; const yolat_train_bn* bn;     // bn == NULL: Linear only
  long M, K, Nout;                                          // rows, in_features, out_features
  Lazy a;                                                   // the input as the forward reads it
  float* y; long ldy; float* stats; Coef k;                 // pre-BatchNorm output, its statistics and coefficients
  bool dense;                                               // the three GEMMs on bf16 operands (yolat_bt_*)
  const uint16_t* pack_f;                                   // bf16x6 image of W for the forward, or NULL
  float* w_bn; float* w_dw;                                 // scratch of bn_relu_bwd / of the weight gradient
  const uint16_t* pack_t; float* w_dx;                      // bf16x6 image of W^T for the input gradient (+ scratch), or NULL
};

// ops.linear_fwd's choice of the bf16x6 LDS-tiled GEMM (many rows x long K in front of a training BatchNorm) for the
// forward of a block that has a weight image to run it on; asked when the image is packed and when the block runs
bool x6_fwd(const Lbr& B) {
  return B.pack_f && !yl_strict_fp32() && B.stats && !B.a.scale && B.lin->b && B.M >= 1024 && B.K >= 256 && B.K % 16 == 0 &&
         B.Nout >= 128 && B.a.ld % 4 == 0 && yl_aligned16(B.a.t) && yolat_gemm_x6_work_elems(B.M, B.Nout, B.K) == 0;
}
// ops.linear_fwd_wt's, for the input gradient dx (+)= dz . W
bool x6_wt(const Lbr& B, const float* dz, long lddz, int acc) {
  return B.pack_t && !yl_strict_fp32() && !acc && B.M >= 1024 && B.Nout >= 256 && B.Nout % 16 == 0 && B.K >= 512 && lddz % 4 == 0 &&
         yl_aligned16(dz);
}

// engine.lbr_fwd (training): Linear with BatchNorm statistics, finalize; out != NULL: the activation, materialised.  The
// bf16x6 GEMM (ops.linear_fwd's choice) runs on the weight image the side stream packed at the start of the step — the same
// kernel on the same weights, issued sooner.
int lbr_fwd(const Lbr& B, float* out, long ldo, hipStream_t st) {
  const Lazy& a = B.a;
  const float* W = B.lin->W;
  const float* bias = B.lin->b;
  if (B.dense)
    YL_TRY(yolat_bt_linear_fwd(a.t, a.ld, B.M, B.K, a.scale, a.shift, a.relu, W, B.K, bias, B.Nout, B.y, B.ldy, B.stats, st));
  else if (x6_fwd(B))
    YL_TRY(yolat_gemm_x6_stats(a.t, a.ld, B.M, B.K, B.pack_f, bias, B.Nout, B.y, B.ldy, B.stats, st));
  else
    YL_TRY(yolat_linear_fwd(a.t, a.ld, B.M, B.K, a.scale, a.shift, a.relu, W, B.K, bias, B.Nout, nullptr, nullptr, 0, B.y, B.ldy, 0,
                            B.stats, st));
  if (!B.bn) return 0;
  YL_TRY(finalize(B.stats, B.M, B.Nout, *B.bn, B.k, st));
  if (out) YL_TRY(yolat_scale_shift_relu(B.y, B.ldy, B.M, B.Nout, B.k.scale, B.k.shift, 1, out, ldo, st));
  return 0;
}

// engine.lbr_bwd: BatchNorm + ReLU backward in place on dz, the weight gradient, the input gradient into dx (NULL: not
// needed).  `chain` carries dz -> dx; fork_dw: the weight gradient goes to the side stream, forked behind the BatchNorm
// backward (engine._on_side) — false: it stays on `chain` (a block that sits behind a fork as a whole).
int lbr_bwd(const yolat_train_model* m, const Lbr& B, float* dz, long lddz, float* dx, long lddx, int acc, hipStream_t chain,
            bool fork_dw, Streams& S) {
  const Lazy& a = B.a;
  if (B.bn)
    YL_TRY(yolat_bn_relu_bwd(dz, lddz, B.y, B.ldy, B.M, B.Nout, B.bn->gamma, B.k.mean, B.k.invstd, B.k.scale, B.k.shift, 1,
                             grad_of(m, B.bn->gamma), grad_of(m, B.bn->beta), 0, dz, lddz, B.w_bn, chain));
  hipStream_t ws = fork_dw ? S.fork() : chain;
  float* dW = grad_of(m, B.lin->W);
  float* db = grad_of(m, B.lin->b);
  if (B.dense)
    YL_TRY(yolat_bt_linear_bwd_w(dz, lddz, B.M, B.Nout, a.t, a.ld, B.K, a.scale, a.shift, a.relu, dW, B.K, db, B.w_dw, ws));
  else
    YL_TRY(yolat_linear_bwd_w(dz, lddz, B.M, B.Nout, a.t, a.ld, B.K, a.scale, a.shift, a.relu, dW, B.K, db, 0, B.w_dw, ws));
  if (!dx) return 0;
  if (B.dense) return yolat_bt_linear_fwd_wt(dz, lddz, B.M, B.Nout, B.lin->W, B.K, B.K, dx, lddx, acc, chain);
  if (x6_wt(B, dz, lddz, acc))
    return yolat_gemm_x6(dz, lddz, B.M, B.Nout, B.pack_t, nullptr, 0, B.K, dx, lddx, B.w_dx, chain);
  return yolat_linear_fwd_wt(dz, lddz, B.M, B.Nout, B.lin->W, B.K, B.K, dx, lddx, acc, chain);
}

// The schedule of one step over its arguments, workspace and streams.
struct Sched {
  const Step& a;
  const yolat_train_model* m;
  const Dims d;
  const TrainBuf& b;
  Streams& S;
  hipStream_t st;
  const bool dense;
  const long N, E, P;
  const int* row_ptr; const int* src; const int* dst; const float* attr; const int* seg_ptr; const int* node_seg;

  Sched(const Step& a_, const TrainBuf& b_, Streams& S_)
      : a(a_), m(a_.m), d(a_.m), b(b_), S(S_), st(S_.main), dense((a_.m->half & 2) != 0), N(a_.N), E(a_.E), P(a_.P),
        row_ptr(b_.row_ptr), src(b_.src), dst(b_.dst), attr(b_.attr), seg_ptr(b_.seg_ptr), node_seg(b_.node_seg) {
    if (const yolat_graph_csr* g = a.g) {
      row_ptr = g->row_ptr; src = g->src; dst = g->dst; attr = g->attr; seg_ptr = g->seg_ptr; node_seg = g->node_seg;
    }
  }

  // ---- where a conv layer's two outputs live: a column slot of feats / fsup (output layers) or a buffer of their own
  float* f_out(long l) const { return l - d.lo >= 0 ? b.feats + (l - d.lo) * d.C : b.cv[l].f_tmp; }
  float* s_out(long l) const { return l - d.lo >= 0 ? b.fsup + (l - d.lo) * d.C : b.cv[l].s_tmp; }
  long ld_out(long l) const { return l - d.lo >= 0 ? d.D : d.C; }
  // ---- and its two inputs as the forward saw them
  Lazy feat_in(long l) const { return l == 0 ? Lazy{a.x, a.ldx, nullptr, nullptr, 0} : Lazy{f_out(l - 1), ld_out(l - 1), nullptr, nullptr, 0}; }
  Lazy node_in(long l) const {
    return l == 0 ? Lazy{a.x, a.ldx, nullptr, nullptr, 0}
                  : Lazy{s_out(l - 1), ld_out(l - 1), b.cv[l - 1].cn_scale, b.cv[l - 1].cn_shift, 1};
  }

  // ---- the Linear (+ BatchNorm + ReLU) blocks
  Lbr root(long l) const {             // lin_r of conv layer l: the aggregation accumulates onto its output
    return Lbr{&m->conv[l].lin_r, nullptr, N, m->conv[l].Cin, d.C, feat_in(l), f_out(l), ld_out(l), nullptr, Coef(nullptr, 0),
               false, nullptr, nullptr, b.cv[l].w_root, nullptr, nullptr};
  }
  Lbr node(long l) const {             // mlp_node of conv layer l
    const ConvBuf& v = b.cv[l];
    return Lbr{&m->conv[l].node, &m->conv[l].bn_node, N, m->conv[l].Cin, d.C, node_in(l), s_out(l), ld_out(l), v.st_n,
               v.node_coef(d.C), false, nullptr, v.w_node_bn, v.w_node_w, nullptr, nullptr};
  }
  Lbr fus_s() const {                  // fusion_block_super: input sup = Z[:, 2F+D:], post-activation output Z[:, F+D:2F+D]
    return Lbr{&m->fus_s, &m->fus_s_bn, P, d.D, d.F, Lazy{b.Z + 2 * d.F + d.D, d.ZW, nullptr, nullptr, 0}, b.fs_y, d.F, b.fs_st,
               Coef(b.fs_c, d.F), dense, nullptr, b.wfsbn, dense ? b.bt_wfs : b.wfsw, nullptr, nullptr};
  }
  Lbr cls0() const {                   // prediction_cls.0
    return Lbr{&m->c1, &m->c1_bn, P, d.ZW, d.H1, Lazy{b.Z, d.ZW, nullptr, nullptr, 0}, b.c1y, d.H1, b.c1st, Coef(b.c1c, d.H1),
               dense, b.c1pack, b.w1bn, dense ? b.bt_w1 : b.w1w, b.p1, b.x1w};
  }
  Lbr cls1() const {                   // prediction_cls.1
    return Lbr{&m->c2, &m->c2_bn, P, d.H1, d.H2, Lazy{b.c1y, d.H1, b.c1c, b.c1c + d.H1, 1}, b.c2y, d.H2, b.c2st,
               Coef(b.c2c, d.H2), dense, nullptr, b.w2bn, dense ? b.bt_w2 : b.w2w, b.p2, b.x2w};
  }
  Lbr cls2() const {                   // prediction_cls.2 (Linear only)
    return Lbr{&m->c3, nullptr, P, d.H2, d.K, Lazy{b.c2y, d.H2, b.c2c, b.c2c + d.H2, 1}, a.logits, a.ld_logits, nullptr,
               Coef(nullptr, 0), false, nullptr, nullptr, b.w3, nullptr, nullptr};
  }

  int prepare();
  int conv_fwd(long l);
  int head_fwd();
  int head_bwd();
  int conv_bwd(long l, float* d_f_next, float* d_s_next, float** dx_out, float** dxn_out);
  int run();
};

// ================================ graph + what depends on the weights or the graph only ================================
int Sched::prepare() {
  if (!a.g) {
    const long n_seg = (P + 1 + 3) / 4 * 4;
    hipLaunchKernelGGL(k_tp_zero, dim3(yl_cdiv(n_seg + N, 256)), dim3(256), 0, st, b.zblock, n_seg + N, a.status);
    YL_LAUNCH_CHECK();
    YL_TRY(yolat_graph_prepare(a.edge, a.stride_e, a.stride_c, a.e_attr, a.bbox_idx, E, N, P, b.row_ptr, b.perm, b.src, b.dst,
                               b.attr, b.seg_ptr, b.node_seg, b.gwork, a.status, st));
  }
  // Off the critical path: the side stream takes it now, the forward's join (before the classifier) is long past it.  (The
  // Python schedule issues the same launches where their results are first needed, on the main stream; same kernels, same
  // operands.)
  hipStream_t ss = S.fork();
  if (!dense) {      // (bf16_dense: the classifier GEMMs read the fp32 weights and round them themselves)
    const long ZW = d.ZW, H1 = d.H1, H2 = d.H2;
    if (x6_fwd(cls0())) YL_TRY(yolat_gemm_x6_pack(m->c1.W, ZW, H1, ZW, nullptr, b.c1pack, ss));
    if (x6_wt(cls1(), b.d2, H2, 0)) YL_TRY(yolat_gemm_x6_pack_t(m->c2.W, H1, H1, H2, b.p2, ss));
    if (x6_wt(cls0(), b.d1, H1, 0)) YL_TRY(yolat_gemm_x6_pack_t(m->c1.W, ZW, ZW, H1, b.p1, ss));
  }
  for (long l = 0; l < d.L; ++l)
    if (!b.cv[l].fact_fwd) YL_TRY(yolat_conv_split_w1(m->conv[l].nn0.W, m->conv[l].Cin, d.C, b.cv[l].wuv_b, b.cv[l].wc4_b, ss));
  // CSC by source + 1 / deg for the backward (ops.Graph.ensure_csc / inv_deg)
  YL_TRY(yolat_inv_degree(row_ptr, N, b.inv_deg, ss));
  YL_TRY(yolat_csc_by_source(src, E, N, b.col_ptr, b.slots, b.cwork, ss));
  return 0;
}

// ================================ forward of conv layer l (engine.conv_fwd) ================================
int Sched::conv_fwd(long l) {
  const yolat_train_conv& cv = m->conv[l];
  const ConvBuf& v = b.cv[l];
  const long C = d.C, Cin = cv.Cin, ldo = ld_out(l);
  const Lazy f = feat_in(l);
  float* of = f_out(l);
  const Coef k1(v.c1, C), k2(v.c2, C);
  // root term first, the aggregation accumulates onto it (torch_vertex.py:325)
  YL_TRY(lbr_fwd(root(l), nullptr, 0, st));
  if (v.fact_fwd) {
    YL_TRY(yolat_conv_split_w1(cv.nn0.W, Cin, C, v.wuv, v.wc4, st));
    YL_TRY(yolat_linear_fwd(f.t, f.ld, N, Cin, nullptr, nullptr, 0, v.wuv, Cin, nullptr, 2 * C, nullptr, nullptr, 0, v.uv, 2 * C, 0,
                            nullptr, st));
    if (v.half)
      YL_TRY(yolat_edge_uv_lin1_fwd_h(v.uv, 2 * C, src, dst, attr, E, v.wc4, cv.nn0.b, C, (uint16_t*)v.H1, C, v.st1, st));
    else
      YL_TRY(yolat_edge_uv_lin1_fwd(v.uv, 2 * C, src, dst, attr, E, v.wc4, cv.nn0.b, C, (float*)v.H1, C, v.st1, st));
  } else {
    YL_TRY(yolat_edge_lin1_fwd(f.t, f.ld, N, Cin, src, dst, attr, E, cv.nn0.W, 2 * Cin + 4, cv.nn0.b, C, nullptr, nullptr, 0,
                               (float*)v.H1, C, v.st1, st));
  }
  YL_TRY(finalize(v.st1, E, C, cv.bn1, k1, st));
  if (v.half)
    YL_TRY(yolat_linear_fwd_h((const uint16_t*)v.H1, C, E, C, k1.scale, k1.shift, 1, cv.nn3.W, C, cv.nn3.b, C, (uint16_t*)v.H2, C,
                              v.st2, v.wwork_f, st));
  else
    YL_TRY(yolat_linear_fwd((const float*)v.H1, C, E, C, k1.scale, k1.shift, 1, cv.nn3.W, C, cv.nn3.b, C, nullptr, nullptr, 0,
                            (float*)v.H2, C, 0, v.st2, st));
  YL_TRY(finalize(v.st2, E, C, cv.bn4, k2, st));
  if (v.half)
    YL_TRY(yolat_csr_mean_fwd_h((const uint16_t*)v.H2, C, C, k2.scale, k2.shift, 1, row_ptr, N, of, ldo, 1, st));
  else
    YL_TRY(yolat_csr_mean_fwd((const float*)v.H2, C, C, k2.scale, k2.shift, 1, row_ptr, N, of, ldo, 1, st));
  // node branch (mlp_node) on the side stream: read again only by the next layer's node branch and the per-proposal mean
  return lbr_fwd(node(l), nullptr, 0, S.fork());
}

// ================================ pooling, fusion blocks, classifier, loss ================================
int Sched::head_fwd() {
  const long F = d.F, D = d.D, ZW = d.ZW;
  // Everything between the conv layers and the classifier that does NOT go through the fusion block — the per-proposal max
  // of feats, the per-proposal mean of the node branches (computed on the side stream anyway) and fusion_block_super on its
  // P rows — runs on the side stream BESIDE the fusion block (428 us at cfg 3; disjoint column ranges of Z), joined in
  // front of the classifier.  (The Python schedule issues them on the main stream behind it; same kernels and operands.)
  {
    hipStream_t ss = S.fork();       // (behind the last conv layer's aggregation: feats is complete)
    YL_TRY(yolat_segment_max_fwd(b.feats, D, D, nullptr, nullptr, 0, seg_ptr, P, N, b.Z + F, ZW, b.arg_feat, ss));
    YL_TRY(yolat_segment_mean_fwd(b.fsup, D, D, b.sup_coef, b.sup_coef + D, 1, seg_ptr, P, b.Z + 2 * F + D, ZW, ss));
    YL_TRY(lbr_fwd(fus_s(), b.Z + F + D, ZW, ss));
  }
  // fusion block over nodes + per-proposal max (arch:61-63,122): fused, no [N, F] activation
  YL_TRY((dense ? yolat_fusion_pool_train_fwd_bf16 : yolat_fusion_pool_train_fwd)(
      b.feats, D, N, D, m->fus.W, m->fus.b, F, m->fus_bn.gamma, m->fus_bn.beta, m->fus_bn.running_mean, m->fus_bn.running_var,
      m->fus_bn.momentum, m->fus_bn.eps, node_seg, P, b.Z, ZW, b.fus_coef, b.fus_saved, b.fus_work, st));
  S.join();                          // Z is complete: node branches, pooled rows, fusion_block_super, the weight packs
  // classifier (arch:91-93,128)
  YL_TRY(lbr_fwd(cls0(), nullptr, 0, st));
  YL_TRY(lbr_fwd(cls1(), nullptr, 0, st));
  YL_TRY(lbr_fwd(cls2(), nullptr, 0, st));
  {   // BatchNorm1d.num_batches_tracked += 1 for every layer of the forward, one launch
    NbtList nl;
    nl.n = 0;
    auto add = [&](const yolat_train_bn& bn) { if (bn.num_batches_tracked) nl.p[nl.n++] = (long long*)bn.num_batches_tracked; };
    for (long l = 0; l < d.L; ++l) { add(m->conv[l].bn1); add(m->conv[l].bn4); add(m->conv[l].bn_node); }
    add(m->fus_bn); add(m->fus_s_bn); add(m->c1_bn); add(m->c2_bn);
    if (nl.n > 0) {
      hipLaunchKernelGGL(k_tp_nbt, dim3(1), dim3(64), 0, st, nl);
      YL_LAUNCH_CHECK();
    }
  }
  if (m->half & 4)     // classifier != 'softmax': sigmoid + BCELoss (arch:132-133,362-376); logits stay raw, dl = dLoss/dlogits
    return yolat_sigmoid_bce(a.logits, a.ld_logits, a.labels, P, d.K, a.loss, b.dl, d.K, nullptr, 0, b.ce_work, st);
  return yolat_softmax_ce(a.logits, a.ld_logits, a.labels, P, d.K, a.loss, b.dl, d.K, b.ce_work, st);
}

// ================================ backward: classifier, fusion blocks ================================
int Sched::head_bwd() {
  const long F = d.F, D = d.D, ZW = d.ZW;
  // classifier: the dX chain on the main stream, every weight gradient forked to the side stream
  YL_TRY(lbr_bwd(m, cls2(), b.dl, d.K, b.d2, d.H2, 0, st, true, S));
  YL_TRY(lbr_bwd(m, cls1(), b.d2, d.H2, b.d1, d.H1, 0, st, true, S));
  YL_TRY(lbr_bwd(m, cls0(), b.d1, d.H1, b.dZ, ZW, 0, st, true, S));
  // fusion_block_super: its whole backward and the per-proposal mean's feed nothing but the node branches' backward chain,
  // which lives on the side stream: so do they, beside the fusion block's backward (their columns of dZ are disjoint from
  // the ones the main stream reads)
  {
    hipStream_t ss = S.fork();
    float* d_sup = b.dZ + 2 * F + D;
    YL_TRY(lbr_bwd(m, fus_s(), b.dZ + F + D, ZW, d_sup, ZW, 1, ss, false, S));
    YL_TRY(yolat_segment_mean_bwd(d_sup, ZW, D, seg_ptr, node_seg, N, b.d_fsup, D, ss));
  }
  // fusion_block + max pooling
  YL_TRY(yolat_segment_max_bwd(b.dZ + F, ZW, D, b.arg_feat, node_seg, N, b.d_feats, D, st));
  auto fus_part = [&](int mask, hipStream_t s) {
    return (dense ? yolat_fusion_pool_train_bwd_parts_bf16 : yolat_fusion_pool_train_bwd_parts)(
        b.feats, D, N, D, m->fus.W, m->fus_bn.gamma, F, b.fus_coef, b.fus_saved, node_seg, seg_ptr, P, b.dZ, ZW,
        grad_of(m, m->fus.W), grad_of(m, m->fus.b), grad_of(m, m->fus_bn.gamma), grad_of(m, m->fus_bn.beta), b.d_feats, D,
        b.fus_work, mask, s);
  };
  // (column reductions both halves read, then the weight gradient on the side stream beside the input gradient)
  YL_TRY(fus_part(1, st));
  YL_TRY(fus_part(2, S.fork()));
  YL_TRY(fus_part(4, st));
  return 0;
}

// ================================ backward of conv layer l (engine.conv_bwd) ================================
// d_f_next / d_s_next: the gradients a layer below the concat received from the layer above it; *dx_out / *dxn_out: what
// this layer hands down.
int Sched::conv_bwd(long l, float* d_f_next, float* d_s_next, float** dx_out, float** dxn_out) {
  const yolat_train_conv& cv = m->conv[l];
  const ConvBuf& v = b.cv[l];
  const long C = d.C, D = d.D, Cin = cv.Cin, slot = l - d.lo;
  float* d_f = slot >= 0 ? b.d_feats + slot * C : d_f_next;
  float* d_s = slot >= 0 ? b.d_fsup + slot * C : d_s_next;
  const long ldd = slot >= 0 ? D : C;
  // gradients w.r.t. the layer's inputs: accumulated into the output slot of the layer below, or a buffer of their own
  float* dx = nullptr;
  float* dxn = nullptr;
  long lddx = Cin;
  int acc = 0;
  if (l > 0) {
    if (slot - 1 >= 0) { dx = b.d_feats + (slot - 1) * C; dxn = b.d_fsup + (slot - 1) * C; lddx = D; acc = 1; }
    else { dx = v.dx_tmp; dxn = v.dxn_tmp; }
  }
  const Lazy xin = feat_in(l);
  const Coef k1(v.c1, C), k2(v.c2, C);
  // node branch: a chain of its own through the layers -> side stream
  YL_TRY(lbr_bwd(m, node(l), d_s, ldd, dxn, lddx, acc, S.fork(), false, S));
  // root term
  YL_TRY(lbr_bwd(m, root(l), d_f, ldd, dx, lddx, acc, st, true, S));
  // edge side: the gradient w.r.t. H2 (mean -> ReLU -> BatchNorm backward) is formed inside its consumers (bn_csr.hip)
  yolat_bn_csr_grad dg;
  dg.d_out = d_f; dg.ld_out = ldd; dg.dst = dst; dg.inv_deg = b.inv_deg; dg.Y = v.H2; dg.ldy = C;
  dg.mean = k2.mean; dg.invstd = k2.invstd; dg.scale = k2.scale; dg.shift = k2.shift; dg.coef = v.coef2; dg.relu = 1;
  dg.half = v.half ? 1 : 0;
  YL_TRY(yolat_bn_csr_bwd_stats(&dg, E, C, grad_of(m, cv.bn4.gamma), grad_of(m, cv.bn4.beta), 0, v.coef2, v.w_stats, st));
  YL_TRY(yolat_bn_csr_l2_bwd(&dg, E, v.H1, C, k1.scale, k1.shift, 1, cv.nn3.W, C, grad_of(m, cv.nn3.W), C, grad_of(m, cv.nn3.b), 0,
                             v.dA1, C, v.w_l2, k1.mean, k1.invstd, grad_of(m, cv.bn1.gamma), grad_of(m, cv.bn1.beta), v.coef1, st));
  // BatchNorm-1 backward apply + per-node dU sums + attr weight gradient + db1 in one pass
  YL_TRY(yolat_bn_apply_edge_sums(v.dA1, C, v.H1, C, v.dA1, C, v.half ? 1 : 0, E, k1.mean, k1.invstd, k1.scale, k1.shift, 1, v.coef1,
                                  row_ptr, attr, N, v.dUV, 2 * C, v.dwc4, grad_of(m, cv.nn0.b), v.w_apply, st));
  // first edge Linear through the per-node products (ops.edge_lin1_bwd_factorised with partial = (dUV, dWc4))
  YL_TRY(yolat_edge_uv_sums_v(v.dA1, C, v.half ? 1 : 0, b.col_ptr, b.slots, N, C, v.dUV, 2 * C, st));
  {
    hipStream_t ss = S.fork();
    YL_TRY(yolat_linear_bwd_w(v.dUV, 2 * C, N, 2 * C, xin.t, xin.ld, Cin, nullptr, nullptr, 0, v.dwuv, Cin, nullptr, 0, v.w_dwuv, ss));
    YL_TRY(yolat_conv_merge_dw1(v.dwuv, v.dwc4, Cin, C, grad_of(m, cv.nn0.W), 2 * Cin + 4, 0, ss));
  }
  if (dx) YL_TRY(yolat_linear_fwd_wt(v.dUV, 2 * C, N, 2 * C, v.fact_fwd ? v.wuv : v.wuv_b, Cin, Cin, dx, lddx, 1, st));
  *dx_out = dx;
  *dxn_out = dxn;
  return 0;
}

int Sched::run() {
  if (a.phases & 1) {
    YL_TRY(prepare());
    for (long l = 0; l < d.L; ++l) YL_TRY(conv_fwd(l));
    YL_TRY(head_fwd());
    YL_TRY(head_bwd());
    S.join();                          // the head bucket's gradients are complete on `stream`
  }
  if (a.phases & 2) {
    // conv layers, last to first (CSC by source, 1 / deg and the weight splits were prepared by phase 1 on the side stream,
    // joined at its end)
    float* d_f = nullptr;
    float* d_s = nullptr;
    for (long l = d.L - 1; l >= 0; --l) YL_TRY(conv_bwd(l, d_f, d_s, &d_f, &d_s));
    S.join();                          // every gradient is complete on `stream`
  }
  if (a.phases & 4) {
    const yolat_adam_args* o = a.adam;
    YL_TRY(yolat_adam_step(const_cast<float*>(m->param_base), m->grad_base, o->exp_avg, o->exp_avg_sq, o->n, o->lr, o->beta1,
                           o->beta2, o->eps, o->weight_decay, o->step, o->grad_scale, st));
  }
  return 0;
}

}  // namespace

extern "C" size_t yolat_train_step_workspace_bytes(const yolat_train_model* m, int64_t N, int64_t E, int64_t P) {
  if (model_ok(m) != 0 || N <= 0 || E < 0 || P <= 0) return 0;
  return carve(m, N, E, P, nullptr).bytes;
}

extern "C" int yolat_train_step(const yolat_train_model* m, const float* x, int64_t ldx, const int64_t* edge,
                                int64_t stride_e, int64_t stride_c, const float* e_attr, const int64_t* bbox_idx,
                                const yolat_graph_csr* g, const int64_t* labels, int64_t N, int64_t E, int64_t P,
                                float* logits, int64_t ld_logits, float* loss, void* workspace, size_t workspace_bytes,
                                int32_t* status, const yolat_adam_args* adam, int phases, yolat_stream_t stream,
                                yolat_stream_t side_stream) {
  const Step a{m, x, ldx, edge, stride_e, stride_c, e_attr, bbox_idx, g, labels, N, E, P, logits, ld_logits, loss, workspace,
               workspace_bytes, status, adam, phases};
  TrainBuf b;
  YL_TRY(precheck(a, &b));             // nothing has been enqueued: the only place YOLAT_E_UNSUPPORTED comes from
  Streams S{(hipStream_t)stream, (side_stream && side_stream != stream) ? (hipStream_t)side_stream : nullptr, nullptr, nullptr,
            false};
  if (S.side && !events_for(&S)) return YOLAT_E_INVALID;
  int rc = Sched(a, b, S).run();
  if (rc != 0) {
    // part of the step is enqueued: leave the side stream joined, and never report "nothing happened" (an entry point
    // that declined its operands in mid-schedule is a fault of this file, not a shape the caller may retry elsewhere)
    S.join();
    if (rc == YOLAT_E_UNSUPPORTED) rc = YOLAT_E_INVALID;
  }
  return rc;
}
