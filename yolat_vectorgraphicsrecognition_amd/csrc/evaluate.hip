// evaluate.hip — the evaluation of one batch (cad_recognition/train.py:343-460, evaluation.evaluate_batch) enqueued in ONE
// call, nothing read back, nothing sized by a number the device computes (SparseCADGCN.evaluate_submit):
//
//   a. yolat_detect (detect.hip): predict's selection, the pred rows, the batched NMS -> sel, pred, det, det_count;
//   b. the ROWS STAGE, new here: for the rows the selection kept — labels[rows[r]], the loss term, the arg-max, the top-1
//      hit and the confusion cell — and the final sum of the loss;
//   c. yolat_detect_match (detect.hip): the true-positive flags of every (image, IoU threshold) pair -> tp.
//
// The rows stage.  One thread per row r < R_cap = R + Ctot, the bound the host knows from the tree it uploaded, 256 rows per
// workgroup; the total and the row list of sel (sel_record.hpp) are read on the device, as k_detect_rows reads them.
// Row r < total: the loss term of logits[rows[r]] against labels[rows[r]] with the row bodies of loss_rows.hpp — the text
// k_softmax_ce_rows<32> / k_bce_rows<32, false> are made of — the workgroup's fixed-order tree into work[wg], and
// k_eval_final adds the partials in k_ce_final's / k_bce_final's order and divides by total (total * K for BCE) with the
// same fp32 steps.  DetectionLoss on the gathered rows has row r at tree position r as well, so the loss is bit-equal to it;
// the partials of workgroups that hold spare rows only are +0.0f, and a + 0.0f = a.
// A SPARE row r >= total (rows[r] is uninitialised) reads neither rows[r] nor a label and adds +0.0f / no count.
// Counts: stats = [n_true, n_total, confusion K * K] int32 (rows = true class, columns = predicted), zeroed by the call;
// a workgroup counts in LDS (K <= 32: 4 KB) and issues one global integer atomic per non-zero cell — integer adds commute,
// two runs are bit-identical.  A label outside [0, K) poisons the loss with NaN (yolat_softmax_ce's contract), enters no
// confusion cell and is never a hit; nothing is read or written through it.
#include "sel_record.hpp"
#include "loss_rows.hpp"

constexpr int EVAL_KMAX = 32;                 // the register-resident row of the loss kernels
constexpr int64_t EVAL_MAX_TARGETS = 262144;  // yolat_detect_match's limits
constexpr int64_t EVAL_MAX_THRESHOLDS = 65535;

template <bool SOFTMAX>
static __global__ void __launch_bounds__(256) k_eval_rows(const float* logits, long ld, int K, int P, const int64_t* labels,
                                                          const int* sel, int B, int R_cap, float* work, int* stats,
                                                          int* y_pred, int* y_true) {
  __shared__ int cells[EVAL_KMAX * EVAL_KMAX];
  __shared__ int hits;
  const int tid = threadIdx.x;
  const int r = blockIdx.x * 256 + tid;
  const int total = yl_clamp(sel[YL_SEL_TOTAL], R_cap);
  for (int c = tid; c < K * K; c += 256) cells[c] = 0;
  if (tid == 0) hits = 0;
  __syncthreads();
  float row_loss = 0.f;
  if (r < total) {
    const int row = yl_clamp(yl_sel_rows(sel, B)[r], P - 1);
    const float* z = logits + (long)row * ld;
    float* const no_grad = nullptr;
    if (SOFTMAX) {
      YL_CE_ROW_LOSS(EVAL_KMAX, z, K, labels, row, 1, no_grad, 0l, row_loss)
    } else {
      YL_BCE_ROW_LOSS(EVAL_KMAX, false, z, K, labels, row, 0.f, no_grad, 0l, no_grad, 0l, row_loss)
    }
    const int arg = yl_argmax_row(z, K);      // torch's max(1)[1] (sel_record.hpp)
    const int64_t label = labels[row];
    y_pred[r] = arg;
    y_true[r] = label < INT32_MIN ? INT32_MIN : (label > INT32_MAX ? INT32_MAX : (int)label);
    if (label >= 0 && label < K) {
      atomicAdd(&cells[(int)label * K + arg], 1);
      if ((int)label == arg) atomicAdd(&hits, 1);
    }
  }
  yl_rows_tree256(tid, row_loss, work + blockIdx.x);      // (its barriers also close the LDS counts)
  for (int c = tid; c < K * K; c += 256) {
    const int n = cells[c];
    if (n != 0) atomicAdd(&stats[2 + c], n);
  }
  if (tid == 0) {
    if (hits != 0) atomicAdd(&stats[0], hits);
    if (blockIdx.x == 0) stats[1] = total;
  }
}

// the partials in k_ce_final's / k_bce_final's order; the divisor is read on the device
template <bool SOFTMAX>
static __global__ void __launch_bounds__(1024) k_eval_final(const float* work, int n, const int* sel, int R_cap, int K,
                                                            float* loss) {
  yl_partials_tree1024(work, n, threadIdx.x, [=](float sum) {
    const int total = yl_clamp(sel[YL_SEL_TOTAL], R_cap);
    if (SOFTMAX) {
      loss[0] = sum / (float)total;
    } else {
      const float inv_n = 1.f / (float)((long)total * (long)K);
      loss[0] = inv_n * sum;
    }
  });
}

namespace {
bool eval_rows_shape_ok(int64_t P, int64_t K, int64_t R_cap) {
  return K >= 2 && K <= EVAL_KMAX && P > 0 && P < (1LL << 30) && R_cap >= 0 && R_cap < (1LL << 30);
}
size_t eval_work_bytes(int64_t R_cap) { return ((sizeof(float) * (size_t)((R_cap + 255) / 256 + 1)) + 255) & ~(size_t)255; }

// zeroing + rows + final: at most three launches.  Every argument has been checked by the caller.
int eval_rows_launch(const float* logits, int64_t ld, int64_t P, int64_t K, const int64_t* labels, const int32_t* sel,
                     int64_t B, int64_t R_cap, int softmax, int32_t* stats, float* loss, int32_t* y_pred, int32_t* y_true,
                     float* work, hipStream_t st) {
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(int32_t) * (size_t)(2 + K * K), st);
  if (e != hipSuccess) return (int)e;
  const int nwg = yl_cdiv(R_cap, 256);
  if (nwg > 0) {
    if (softmax)
      hipLaunchKernelGGL(k_eval_rows<true>, dim3(nwg), dim3(256), 0, st, logits, (long)ld, (int)K, (int)P, labels, sel, (int)B,
                         (int)R_cap, work, stats, y_pred, y_true);
    else
      hipLaunchKernelGGL(k_eval_rows<false>, dim3(nwg), dim3(256), 0, st, logits, (long)ld, (int)K, (int)P, labels, sel,
                         (int)B, (int)R_cap, work, stats, y_pred, y_true);
    YL_LAUNCH_CHECK();
  }
  if (softmax)
    hipLaunchKernelGGL(k_eval_final<true>, dim3(1), dim3(1024), 0, st, work, nwg, sel, (int)R_cap, (int)K, loss);
  else
    hipLaunchKernelGGL(k_eval_final<false>, dim3(1), dim3(1024), 0, st, work, nwg, sel, (int)R_cap, (int)K, loss);
  YL_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int yolat_eval_rows(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const int64_t* labels,
                               const int32_t* sel, int64_t B, int64_t R_cap, int softmax, int32_t* stats, float* loss,
                               int32_t* y_pred, int32_t* y_true, float* work, yolat_stream_t stream) {
  if (R_cap < 0 || P <= 0 || K < 2 || ld_logits < K || B < 1) return YOLAT_E_INVALID;
  if (!sel || !stats || !loss || !work) return YOLAT_E_INVALID;
  if (R_cap > 0 && (!logits || !labels || !y_pred || !y_true)) return YOLAT_E_INVALID;
  if (!eval_rows_shape_ok(P, K, R_cap)) return YOLAT_E_UNSUPPORTED;
  return eval_rows_launch(logits, ld_logits, P, K, labels, sel, B, R_cap, softmax, stats, loss, y_pred, y_true, work,
                          (hipStream_t)stream);
}

extern "C" size_t yolat_evaluate_workspace_bytes(int64_t N, int64_t P, int64_t R, int64_t Ctot, int64_t K, int64_t B,
                                                 int64_t G, int64_t T) {
  if (K > EVAL_KMAX || G < 0 || G > EVAL_MAX_TARGETS || T < 1 || T > EVAL_MAX_THRESHOLDS) return 0;
  const size_t det = yolat_detect_workspace_bytes(N, P, R, Ctot, K, B);      // declines K < 2 and every size of its own
  if (det == 0) return 0;
  return ((det + 255) & ~(size_t)255) + eval_work_bytes(R + Ctot);
}

extern "C" int yolat_evaluate(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const float* bbox,
                              const int64_t* edge, int64_t stride_e, int64_t stride_c, const int64_t* bbox_idx, int64_t N,
                              int64_t E, const yolat_predict_tree* tree, const float* scale, int softmax, float conf_thres,
                              float iou_thres, const int64_t* labels, const float* gt_boxes, const float* gt_labels, int64_t G,
                              const int32_t* gt_ptr, const float* thresholds, int64_t T, int32_t* sel, float* pred,
                              float* det_out, int32_t* det_count, int32_t* stats, float* loss, int32_t* y_pred,
                              int32_t* y_true, uint8_t* tp_out, void* workspace, size_t workspace_bytes,
                              yolat_stream_t stream) {
  // everything any of the three stages can refuse is decided here, in front of the first launch
  if (!logits || !bbox || !bbox_idx || !tree || !scale || !sel || !det_out || !det_count || !workspace || P <= 0 || K < 2 ||
      N <= 0 || E < 0 || (E > 0 && !edge) || ld_logits < K)
    return YOLAT_E_INVALID;
  const yolat_predict_tree& t = *tree;
  if (!yl_predict_tree_ok(t, 1)) return YOLAT_E_INVALID;
  const int64_t R_cap = t.R + t.Ctot;
  if (!labels || !stats || !loss || !tp_out || !gt_ptr || !thresholds || G < 0 || T < 1) return YOLAT_E_INVALID;
  if (G > 0 && (!gt_boxes || !gt_labels)) return YOLAT_E_INVALID;
  if (R_cap > 0 && (!pred || !y_pred || !y_true)) return YOLAT_E_INVALID;
  const size_t need = yolat_evaluate_workspace_bytes(N, P, t.R, t.Ctot, K, t.B, G, T);
  if (need == 0 || E >= (1LL << 30) || !eval_rows_shape_ok(P, K, R_cap) || (((uintptr_t)workspace) & 255) != 0)
    return YOLAT_E_UNSUPPORTED;
  if (workspace_bytes < need) return YOLAT_E_INVALID;
  const size_t det_bytes = need - eval_work_bytes(R_cap);
  char* base = reinterpret_cast<char*>(workspace);
  float* work = reinterpret_cast<float*>(base + det_bytes);
  YL_TRY(yolat_detect(logits, ld_logits, P, K, bbox, edge, stride_e, stride_c, bbox_idx, N, E, tree, scale, softmax,
                      conf_thres, iou_thres, 0, sel, pred, det_out, det_count, base, det_bytes, stream));
  YL_TRY(eval_rows_launch(logits, ld_logits, P, K, labels, sel, t.B, R_cap, softmax, stats, loss, y_pred, y_true, work,
                          (hipStream_t)stream));
  return yolat_detect_match(det_out, det_count, t.B, gt_boxes, gt_labels, G, gt_ptr, thresholds, T, tp_out, stream);
}
