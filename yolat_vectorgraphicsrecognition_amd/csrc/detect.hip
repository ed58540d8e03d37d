// detect.hip — the detection post-processing of one evaluation batch on the device, all images in one call per stage
// (evaluation.evaluate_batch(device_post=True), postprocess.non_max_suppression_batched / get_batch_statistics_batched):
//
//   1. yolat_detect_scores  logits -> the `pred` rows of the reference's loop (cad_recognition/train.py:423-433):
//        (box * scale[image], 1 - p[K-1], p[0 .. K-2]),  p = softmax(logits) or the logits themselves;
//   2. yolat_nms_batched    the class-aware non_max_suppression of train.py:34-121 (classes=None, labels=()) per image;
//   3. yolat_detect_match   the true-positive walk of utils/det_util.py:154-202 for every (image, IoU threshold) pair.
// and yolat_detect (2b, 2c): predict's selection, 1. and 2. of one batch enqueued in one call, no size read by the host.
//
// Batched NMS.  A (row, class) pair is a SLOT, slot = row * nc + class: row-major order = the candidate order of the
// reference.  k_det_keys gives every slot the 64-bit key (image << 32 | ~orderable(score)); a slot that is no candidate
// gets the low word 0xFFFFFFFF, which no candidate has (it would be the image of a NaN), so it sorts behind the image's
// candidates.  ONE stable rocPRIM radix sort of (key, slot) over the bits in use then leaves, for image i, its candidates
// in descending score order (ties: ascending slot) at the slots' own range [image_ptr[i] * nc, image_ptr[i + 1] * nc) —
// no compaction, no per-image launch, no host read.  k_det_nms: one workgroup per image walks that range 1024 candidates
// at a time.  The evaluation keeps at most MAX_DET = 300 boxes per image and the first 300 kept boxes of a greedy NMS
// depend only on earlier kept boxes, so a candidate is tested against the kept list (<= 300 boxes, LDS) and against the
// boxes kept in its own chunk, and the walk stops at the 300th keep: O(n * 300) IoU tests and O(n) memory, where the
// n x n / 64 suppression mask of nms.hip is 112 MB per image at the 30 000-candidate cap.  The predicate is nms.hip's.
// Workspace: 24 bytes per slot (keys and slots, in and out) + rocPRIM's own temporary storage.
#include "sel_record.hpp"

#include <rocprim/device/device_radix_sort.hpp>

typedef unsigned long long u64;

constexpr int DET_MAX_DET = 300;       // train.py:45
constexpr int DET_MAX_NMS = 30000;     // train.py:47
constexpr float DET_MAX_WH = 4096.f;   // train.py:44
constexpr int DET_CHUNK = 1024;        // candidates per step of the walk = threads of k_det_nms
constexpr int64_t DET_MAX_SLOTS = (int64_t)1 << 27;
constexpr int64_t DET_MAX_IMAGES = 65536;
constexpr int64_t DET_MAX_CLASSES = 4096;
constexpr int64_t DET_MAX_TARGETS = 262144;   // claimed-set of k_det_match: one bit per target in LDS (32 KB)

// the image of row r: the last i in [0, B) with image_ptr[i] <= r, r < image_ptr[i + 1]; B when no image holds the row
__device__ __forceinline__ int det_image_of(const int* __restrict__ image_ptr, int B, int R, int r) {
  int lo = 0, hi = B;                  // invariant: image_ptr[lo] <= r (or lo == 0), first i with image_ptr[i] > r is in (lo, hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (yl_clamp(image_ptr[mid], R) <= r) lo = mid; else hi = mid;
  }
  return (r >= yl_clamp(image_ptr[lo], R) && r < yl_clamp(image_ptr[lo + 1], R)) ? lo : B;
}

// ------------------------------------------------------------------------------------------------
// 1. scores.  One thread per row; K is small (the classes of the model), three passes over the row.
// ------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_det_scores(const float* __restrict__ logits, int R, int K, long ld,
                                                          const float* __restrict__ boxes,
                                                          const int* __restrict__ image_ptr, int B,
                                                          const float* __restrict__ scale, int softmax,
                                                          float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* x = logits + (long)r * ld;
  float* o = out + (long)r * (4 + K);
  const int img = det_image_of(image_ptr, B, R, r);
  const float* sc = scale + 4 * (img < B ? img : 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = img < B ? boxes[(long)r * 4 + j] * sc[j] : 0.f;
  if (softmax) {
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmaxf(m, x[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(x[k] - m);
    for (int k = 0; k < K - 1; ++k) o[5 + k] = expf(x[k] - m) / s;
    o[4] = 1.f - expf(x[K - 1] - m) / s;
  } else {
    for (int k = 0; k < K - 1; ++k) o[5 + k] = x[k];
    o[4] = 1.f - x[K - 1];
  }
}

// ------------------------------------------------------------------------------------------------
// 2. batched NMS
// ------------------------------------------------------------------------------------------------
// descending-order image of a score: larger score -> smaller word; 0xFFFFFFFF only for the bit pattern 0xFFFFFFFF (a NaN)
__device__ __forceinline__ unsigned det_desc_bits(float s) {
  const unsigned u = __float_as_uint(s);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

static __global__ void __launch_bounds__(256) k_det_keys(const float* __restrict__ pred, int R, int nc,
                                                        const int* __restrict__ image_ptr, int B, float conf_thres,
                                                        u64* __restrict__ keys, unsigned* __restrict__ slots, long S) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int r = (int)(s / nc), c = (int)(s - (long)r * nc);
  const float* row = pred + (long)r * (5 + nc);
  const float obj = row[4];
  const float conf = yl_mul_rn(row[5 + c], obj);
  const int img = det_image_of(image_ptr, B, R, r);
  const bool cand = img < B && obj > conf_thres && conf > conf_thres;      // NaN passes neither test
  keys[s] = ((u64)(unsigned)img << 32) | (u64)(cand ? det_desc_bits(conf) : 0xFFFFFFFFu);
  slots[s] = (unsigned)s;
}

__device__ __forceinline__ bool det_over(const float4& a, const float4& b, float thr) {      // nms_over of nms.hip
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
  const float inter = yl_mul_rn(w, h);
  const float sa = yl_mul_rn(a.z - a.x, a.w - a.y), sb = yl_mul_rn(b.z - b.x, b.w - b.y);
  return inter / (sa + sb - inter) > thr;
}

// One workgroup per image.  Per chunk of 1024 sorted candidates (one per thread): (A) every thread tests its candidate
// against the kept list; (B) the survivors are resolved in order — the first surviving candidate of the chunk is kept
// (its thread writes the detection row), every later survivor is tested against it, and so on: one barrier per kept
// box, at most 300 over the whole walk, plus one closing round per chunk.
static __global__ void __launch_bounds__(DET_CHUNK) k_det_nms(const float* __restrict__ pred, int R, int nc,
                                                             const int* __restrict__ image_ptr,
                                                             const u64* __restrict__ keys,
                                                             const unsigned* __restrict__ slots, float iou_thres,
                                                             int agnostic, float* __restrict__ det_out,
                                                             int* __restrict__ det_count) {
  __shared__ float4 kept[DET_MAX_DET];
  __shared__ float4 cbox[DET_CHUNK];
  __shared__ int wfirst[2][DET_CHUNK / 64];
  __shared__ int n_s;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = yl_clamp(image_ptr[img], R), r1 = yl_clamp(image_ptr[img + 1], R);
  const int rbase = yl_clamp(image_ptr[0], R);
  // the image's slots in sorted order start where its rows' slots start (rows before image_ptr[0] sort last)
  const long s0 = (long)(r0 - rbase) * nc;
  const long len = r1 > r0 && r0 >= rbase ? (long)(r1 - r0) * nc : 0;
  if (tid == 0) {
    long lo = 0, hi = len;             // first position whose low word is 0xFFFFFFFF (no candidate)
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if ((unsigned)(keys[s0 + mid] & 0xFFFFFFFFull) == 0xFFFFFFFFu) hi = mid; else lo = mid + 1;
    }
    n_s = (int)(lo < DET_MAX_NMS ? lo : DET_MAX_NMS);
  }
  __syncthreads();
  const int n = n_s;
  float* out = det_out + (long)img * DET_MAX_DET * 6;
  int nk = 0, par = 0;                 // boxes kept so far; parity of the wfirst buffer (both uniform over the workgroup)
  for (int c0 = 0; c0 < n && nk < DET_MAX_DET; c0 += DET_CHUNK) {
    const int i = c0 + tid;
    bool alive = i < n;
    float4 raw = make_float4(0.f, 0.f, 0.f, 0.f), box = raw;
    float conf = 0.f, cls = 0.f;
    if (alive) {
      const unsigned s = slots[s0 + i];
      const int r = (int)(s / (unsigned)nc), c = (int)(s - (unsigned)r * (unsigned)nc);
      const float* row = pred + (long)r * (5 + nc);
      raw = make_float4(row[0], row[1], row[2], row[3]);
      conf = yl_mul_rn(row[5 + c], row[4]);
      cls = (float)c;
      const float shift = agnostic ? 0.f : cls * DET_MAX_WH;      // exact: c < 4096
      box = make_float4(raw.x + shift, raw.y + shift, raw.z + shift, raw.w + shift);
    }
    cbox[tid] = box;
    for (int k = 0; k < nk && alive; ++k)                        // (A)
      if (det_over(kept[k], box, iou_thres)) alive = false;
    for (int it = 0; it <= DET_CHUNK; ++it) {                     // (B) every round keeps one box or ends the chunk
      const u64 b = __ballot(alive);
      if (lane == 0) wfirst[par][wave] = b ? wave * 64 + (__ffsll((long long)b) - 1) : DET_CHUNK;
      __syncthreads();
      int first = DET_CHUNK;
#pragma unroll
      for (int w = 0; w < DET_CHUNK / 64; ++w) first = yl_min(first, wfirst[par][w]);
      par ^= 1;
      if (first >= DET_CHUNK) break;
      const float4 kb = cbox[first];
      if (tid == first) {
        kept[nk] = box;
        float* o = out + (long)nk * 6;
        o[0] = raw.x; o[1] = raw.y; o[2] = raw.z; o[3] = raw.w; o[4] = conf; o[5] = cls;
        alive = false;
      } else if (alive && det_over(kb, box, iou_thres)) {
        alive = false;
      }
      if (++nk >= DET_MAX_DET) break;
    }
    __syncthreads();                   // kept[] complete, cbox[] free
  }
  for (int j = nk * 6 + tid; j < DET_MAX_DET * 6; j += DET_CHUNK) out[j] = 0.f;
  if (tid == 0) det_count[img] = nk;
}

// ------------------------------------------------------------------------------------------------
// 2b. the pred rows of yolat_detect: k_predict_gather (subgraph.hip) + k_det_scores in one launch with every size read on
// the device.  One thread per row r < R_cap = R + Ctot, the bound the host knows from the tree it uploaded; the record of
// yolat_predict_select (sel_record.hpp) says how many of them exist and which proposal each is.  Row r < total: the
// proposal's box enlarged by 5 % about its centre with the fp32 steps of k_predict_gather (w / 2 is exact, nothing else is
// a multiply feeding an add), times the image's scale, and the scores of k_det_scores — bit for bit the row the two calls
// produce.  A SPARE row r >= total belongs to no image (det_image_of gives B behind image_off[B] = total): rows[r] is
// uninitialised and is not read, the row is written as zeros for k_det_keys, and it can never be a candidate.
// (A variant in which this kernel also wrote the sort keys — one launch fewer — was measured and is no faster: DESIGN.md.)
// ------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_detect_rows(const float* __restrict__ logits, long ld, int K, int P,
                                                             const float* __restrict__ bbox, const int* __restrict__ sel,
                                                             int B, int R_cap, const float* __restrict__ scale, int softmax,
                                                             float* __restrict__ pred) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R_cap) return;
  const int total = yl_clamp(sel[YL_SEL_TOTAL], R_cap);
  const int* rows = yl_sel_rows(sel, B);
  float* o = pred + (long)r * (4 + K);
  if (r < total) {
    const int row = yl_clamp(rows[r], P - 1);
    const float x1 = bbox[4l * row], y1 = bbox[4l * row + 1], x2 = bbox[4l * row + 2], y2 = bbox[4l * row + 3];
    const float w = (x2 - x1) * 1.05f, h = (y2 - y1) * 1.05f, cx = (x2 + x1) / 2.f, cy = (y2 + y1) / 2.f;
    const float e[4] = {cx - w / 2.f, cy - h / 2.f, cx + w / 2.f, cy + h / 2.f};
    const int img = det_image_of(yl_sel_image_off(sel), B, R_cap, r);
    const float* sc = scale + 4 * (img < B ? img : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = img < B ? e[j] * sc[j] : 0.f;
    const float* x = logits + (long)row * ld;
    if (softmax) {
      float m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmaxf(m, x[k]);
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += expf(x[k] - m);
      for (int k = 0; k < K - 1; ++k) o[5 + k] = expf(x[k] - m) / s;
      o[4] = 1.f - expf(x[K - 1] - m) / s;
    } else {
      for (int k = 0; k < K - 1; ++k) o[5 + k] = x[k];
      o[4] = 1.f - x[K - 1];
    }
  } else {
    for (int j = 0; j < 4 + K; ++j) o[j] = 0.f;
  }
}

namespace {
struct DetPlan { size_t off_keys, off_slots, off_skeys, off_sslots, off_tmp, tmp_bytes, total; int end_bit; };
bool det_shape_ok(int64_t R, int64_t nc, int64_t B) {
  return R >= 0 && nc >= 1 && nc <= DET_MAX_CLASSES && B >= 1 && B <= DET_MAX_IMAGES && R * nc <= DET_MAX_SLOTS;
}
DetPlan det_plan(int64_t R, int64_t nc, int64_t B) {
  DetPlan p;
  const size_t S = (size_t)(R * nc);
  p.end_bit = 32;
  while (((int64_t)1 << (p.end_bit - 32)) <= B) ++p.end_bit;      // image ids 0 .. B (B = a row of no image)
  size_t tmp = 0;
  if (S > 0)
    (void)rocprim::radix_sort_pairs(nullptr, tmp, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                    (unsigned*)nullptr, S, 0, (unsigned)p.end_bit, (hipStream_t)0);
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off = 0;
  p.off_keys = off; off = al(off + sizeof(u64) * S);
  p.off_skeys = off; off = al(off + sizeof(u64) * S);
  p.off_slots = off; off = al(off + sizeof(unsigned) * S);
  p.off_sslots = off; off = al(off + sizeof(unsigned) * S);
  p.off_tmp = off; off = al(off + tmp);
  p.tmp_bytes = tmp; p.total = off + 256;
  return p;
}
}  // namespace

extern "C" int yolat_detect_scores(const float* logits, int64_t R, int64_t K, int64_t ld, const float* boxes,
                                   const int32_t* image_ptr, int64_t B, const float* scale, int softmax,
                                   float* pred_out, yolat_stream_t stream) {
  if (R < 0 || K < 2 || ld < K || B < 1) return YOLAT_E_INVALID;
  if (!image_ptr || !scale) return YOLAT_E_INVALID;
  if (R == 0) return 0;
  if (!logits || !boxes || !pred_out) return YOLAT_E_INVALID;
  if (R > DET_MAX_SLOTS || K > DET_MAX_CLASSES || B > DET_MAX_IMAGES) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_det_scores, dim3(yl_cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, logits, (int)R, (int)K,
                     (long)ld, boxes, image_ptr, (int)B, scale, softmax, pred_out);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t yolat_nms_batched_work_bytes(int64_t R, int64_t nc, int64_t B) {
  if (!det_shape_ok(R, nc, B)) return 0;
  return det_plan(R, nc, B).total;
}

extern "C" int yolat_nms_batched(const float* pred, int64_t R, int64_t nc, const int32_t* image_ptr, int64_t B,
                                 float conf_thres, float iou_thres, int agnostic, float* det_out, int32_t* det_count,
                                 void* work, size_t work_bytes, yolat_stream_t stream) {
  if (R < 0 || nc < 1 || B < 1) return YOLAT_E_INVALID;
  if (!image_ptr || !det_out || !det_count || !work) return YOLAT_E_INVALID;
  if (R > 0 && !pred) return YOLAT_E_INVALID;
  if (!det_shape_ok(R, nc, B) || (((uintptr_t)work) & 255) != 0) return YOLAT_E_UNSUPPORTED;
  const DetPlan p = det_plan(R, nc, B);
  if (work_bytes < p.total) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(work);
  u64* keys = reinterpret_cast<u64*>(base + p.off_keys);
  u64* skeys = reinterpret_cast<u64*>(base + p.off_skeys);
  unsigned* slots = reinterpret_cast<unsigned*>(base + p.off_slots);
  unsigned* sslots = reinterpret_cast<unsigned*>(base + p.off_sslots);
  const long S = (long)(R * nc);
  if (S > 0) {
    hipLaunchKernelGGL(k_det_keys, dim3(yl_cdiv(S, 256)), dim3(256), 0, st, pred, (int)R, (int)nc, image_ptr, (int)B,
                       conf_thres, keys, slots, S);
    YL_LAUNCH_CHECK();
    size_t tmp = p.tmp_bytes;
    if (rocprim::radix_sort_pairs(base + p.off_tmp, tmp, keys, skeys, slots, sslots, (size_t)S, 0, (unsigned)p.end_bit,
                                  st) != hipSuccess)
      return YOLAT_E_INVALID;
  }
  hipLaunchKernelGGL(k_det_nms, dim3((int)B), dim3(DET_CHUNK), 0, st, pred, (int)R, (int)nc, image_ptr, skeys, sslots,
                     iou_thres, agnostic, det_out, det_count);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// 2c. yolat_detect: logits -> det [B, 300, 6] of one batch, enqueued in one go (SparseCADGCN.detect_submit).  The
// launches of yolat_predict_select, k_detect_rows over R_cap = R + Ctot rows, then keys / radix sort / k_det_nms over the
// same R_cap rows with image_ptr = the record's offsets: a spare row is a non-candidate of image B, the stable sort puts
// those slots behind every image's own range, and k_det_nms reads an image's range only.  Nothing is read back.
// ------------------------------------------------------------------------------------------------
namespace {
struct DetectPlan { size_t sel_bytes, off_nms, nms_bytes, total; };
bool detect_shape_ok(int64_t N, int64_t P, int64_t R, int64_t Ctot, int64_t K, int64_t B) {
  if (N <= 0 || P <= 0 || R < 0 || Ctot < 0 || K < 2) return false;
  if (N >= (1LL << 30) || P >= (1LL << 30) || R + Ctot >= (1LL << 30)) return false;      // yolat_predict_select's limits
  return det_shape_ok(R + Ctot, K - 1, B);
}
DetectPlan detect_plan(int64_t N, int64_t P, int64_t R, int64_t Ctot, int64_t K, int64_t B) {
  DetectPlan p;
  p.sel_bytes = yolat_predict_select_workspace_bytes(N, P, R);
  p.off_nms = (p.sel_bytes + 255) & ~(size_t)255;
  p.nms_bytes = det_plan(R + Ctot, K - 1, B).total;
  p.total = p.off_nms + p.nms_bytes;
  return p;
}
}  // namespace

extern "C" int yolat_detect_rows(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const float* bbox,
                                 const int32_t* sel, int64_t B, int64_t R_cap, const float* scale, int softmax,
                                 float* pred_out, yolat_stream_t stream) {
  if (R_cap < 0 || P <= 0 || K < 2 || ld_logits < K || B < 1) return YOLAT_E_INVALID;
  if (!sel || !scale) return YOLAT_E_INVALID;
  if (R_cap == 0) return 0;
  if (!logits || !bbox || !pred_out) return YOLAT_E_INVALID;
  if (P >= (1LL << 30) || !det_shape_ok(R_cap, K - 1, B)) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_detect_rows, dim3(yl_cdiv(R_cap, 256)), dim3(256), 0, (hipStream_t)stream, logits, (long)ld_logits,
                     (int)K, (int)P, bbox, sel, (int)B, (int)R_cap, scale, softmax, pred_out);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t yolat_detect_workspace_bytes(int64_t N, int64_t P, int64_t R, int64_t Ctot, int64_t K, int64_t B) {
  if (!detect_shape_ok(N, P, R, Ctot, K, B)) return 0;
  return detect_plan(N, P, R, Ctot, K, B).total;
}

extern "C" int yolat_detect(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const float* bbox,
                            const int64_t* edge, int64_t stride_e, int64_t stride_c, const int64_t* bbox_idx, int64_t N,
                            int64_t E, const yolat_predict_tree* tree, const float* scale, int softmax, float conf_thres,
                            float iou_thres, int agnostic, int32_t* sel, float* pred, float* det_out, int32_t* det_count,
                            void* workspace, size_t workspace_bytes, yolat_stream_t stream) {
  // everything either half can refuse is decided here, in front of the first launch
  if (!logits || !bbox || !bbox_idx || !tree || !scale || !sel || !det_out || !det_count || !workspace || P <= 0 || K < 2 ||
      N <= 0 || E < 0 || (E > 0 && !edge) || ld_logits < K)
    return YOLAT_E_INVALID;
  const yolat_predict_tree& t = *tree;
  if (!yl_predict_tree_ok(t, 1)) return YOLAT_E_INVALID;
  const int64_t R_cap = t.R + t.Ctot;
  if (R_cap > 0 && !pred) return YOLAT_E_INVALID;
  if (E >= (1LL << 30) || !detect_shape_ok(N, P, t.R, t.Ctot, K, t.B) || (((uintptr_t)workspace) & 255) != 0)
    return YOLAT_E_UNSUPPORTED;
  const DetectPlan p = detect_plan(N, P, t.R, t.Ctot, K, t.B);
  if (workspace_bytes < p.total) return YOLAT_E_INVALID;
  char* base = reinterpret_cast<char*>(workspace);
  YL_TRY(yolat_predict_select(logits, ld_logits, P, K, edge, stride_e, stride_c, bbox_idx, N, E, tree, sel, base,
                              p.sel_bytes, stream));
  if (R_cap > 0) {
    hipLaunchKernelGGL(k_detect_rows, dim3(yl_cdiv(R_cap, 256)), dim3(256), 0, (hipStream_t)stream, logits, (long)ld_logits,
                       (int)K, (int)P, bbox, sel, (int)t.B, (int)R_cap, scale, softmax, pred);
    YL_LAUNCH_CHECK();
  }
  return yolat_nms_batched(pred, R_cap, K - 1, yl_sel_image_off(sel), t.B, conf_thres, iou_thres, agnostic, det_out,
                           det_count, base + p.off_nms, p.nms_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// 3. true-positive flags.  One wave per (image, threshold): the detections in order, the image's targets over the lanes.
// IoU with the +1-pixel box sizes of bbox_iou (det_util.py:213-240), fp32, every product rounded on its own; the threshold
// is an fp32 value and the comparison is fp32, as torch compares an fp32 tensor with a Python float.
// ------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(64) k_det_match(const float* __restrict__ det, const int* __restrict__ det_count,
                                                        int B, const float* __restrict__ gt_boxes,
                                                        const float* __restrict__ gt_labels, int G,
                                                        const int* __restrict__ gt_ptr, const float* __restrict__ thresholds,
                                                        unsigned char* __restrict__ tp_out) {
  extern __shared__ unsigned claimed[];          // one bit per target of the image
  const int img = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
  const int g0 = yl_clamp(gt_ptr[img], G), g1 = yl_max(yl_clamp(gt_ptr[img + 1], G), g0);
  const int m = g1 - g0;
  const int nd = yl_clamp(det_count[img], DET_MAX_DET);
  const float thr = thresholds[t];
  for (int w = lane; w < (m + 31) / 32; w += 64) claimed[w] = 0u;
  __syncthreads();
  const float* d = det + (long)img * DET_MAX_DET * 6;
  unsigned tp_bits = 0u;                         // bit j: detection lane + 64 j is a true positive
  int n_claimed = 0;
  for (int di = 0; di < nd && n_claimed < m; ++di) {
    const float px1 = d[di * 6], py1 = d[di * 6 + 1], px2 = d[di * 6 + 2], py2 = d[di * 6 + 3], pl = d[di * 6 + 5];
    const float a1 = yl_mul_rn(px2 - px1 + 1.f, py2 - py1 + 1.f);
    float best = -INFINITY;
    int best_j = 0x7FFFFFFF;
    bool same_any = false;
    for (int j = lane; j < m; j += 64) {
      const float* g = gt_boxes + (long)(g0 + j) * 4;
      const float gx1 = g[0], gy1 = g[1], gx2 = g[2], gy2 = g[3];
      const bool same = gt_labels[g0 + j] == pl;
      same_any |= same;
      const float iw = fmaxf(fminf(px2, gx2) - fmaxf(px1, gx1) + 1.f, 0.f);
      const float ih = fmaxf(fminf(py2, gy2) - fmaxf(py1, gy1) + 1.f, 0.f);
      const float inter = yl_mul_rn(iw, ih);
      const float a2 = yl_mul_rn(gx2 - gx1 + 1.f, gy2 - gy1 + 1.f);
      const float iou = inter / (a1 + a2 - inter + 1e-16f);
      const float v = (same && iou >= thr) ? iou : 0.f;
      if (v > best) { best = v; best_j = j; }    // ascending j inside a lane: the first index wins ties
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oj = __shfl_xor(best_j, o);
      if (ov > best || (ov == best && oj < best_j)) { best = ov; best_j = oj; }
    }
    if (__ballot(same_any) == 0ull) continue;    // no target of this label (det_util.py:176-177)
    if (best >= thr && !((claimed[best_j >> 5] >> (best_j & 31)) & 1u)) {
      __syncthreads();                           // every lane has read the word
      if (lane == 0) claimed[best_j >> 5] |= 1u << (best_j & 31);
      __syncthreads();
      if (lane == (di & 63)) tp_bits |= 1u << (di >> 6);
      ++n_claimed;
    }
  }
  unsigned char* o = tp_out + ((long)t * B + img) * DET_MAX_DET;
  for (int j = 0; lane + 64 * j < DET_MAX_DET; ++j) o[lane + 64 * j] = (unsigned char)((tp_bits >> j) & 1u);
}

extern "C" int yolat_detect_match(const float* det, const int32_t* det_count, int64_t B, const float* gt_boxes,
                                  const float* gt_labels, int64_t G, const int32_t* gt_ptr, const float* thresholds,
                                  int64_t T, uint8_t* tp_out, yolat_stream_t stream) {
  if (B < 1 || G < 0 || T < 1) return YOLAT_E_INVALID;
  if (!det || !det_count || !gt_ptr || !thresholds || !tp_out) return YOLAT_E_INVALID;
  if (G > 0 && (!gt_boxes || !gt_labels)) return YOLAT_E_INVALID;
  if (B > DET_MAX_IMAGES || T > 65535 || G > DET_MAX_TARGETS) return YOLAT_E_UNSUPPORTED;
  const size_t lds = sizeof(unsigned) * (size_t)((G + 31) / 32 + 1);
  hipLaunchKernelGGL(k_det_match, dim3((int)B, (int)T), dim3(64), lds, (hipStream_t)stream, det, det_count, (int)B,
                     gt_boxes, gt_labels, (int)G, gt_ptr, thresholds, tp_out);
  YL_LAUNCH_CHECK();
  return 0;
}
