// metrics.hip — the metrics of an evaluation EPOCH on the device (cad_recognition/train.py:462-508 over
// utils/det_util.py:71-145; evaluation.EpochMetrics): what yolat_evaluate leaves on the device for a batch is appended to a
// caller-owned EPOCH RECORD, and at the end of the epoch AP, precision and recall per (IoU threshold, class), the mean loss
// and the summed counts are computed from the record and handed over in ONE contiguous block.
//
// The record (layout: include/yolat_hip.h, yolat_metrics_record_bytes).  Image i of the epoch owns the slots
// [300 i, 300 i + 300); a slot is (conf fp32, cls int32, tp uint32: bit t = true positive at threshold t); cls = -1 marks
// a slot nobody filled.  The HOST assigns the slots (image_base, batch_index are arguments): there is no device cursor,
// so submissions from several streams write disjoint slots and the record does not depend on how the streams interleave.
// Counts are added with integer atomics, floats are stored, never added atomically: two epochs are bit-identical.
//
//   k_metrics_append    B + 1 workgroups, ONE launch per batch: workgroup b < B packs image b, workgroup B the batch's
//                       targets (gt_hist), counts (stats), loss and flags.  sel[1] / sel[2] are read on the device; a
//                       flagged batch leaves its slots unfilled (the host fills them later, yolat_metrics_append_host).
//   yolat_metrics_finalize
//     k_metrics_keys    key = class << 32 | descending image of conf (an unfilled slot: class K, behind every class)
//     rocPRIM           ONE stable radix sort of (key, slot): the stable descending sort by conf followed by the stable
//                       regrouping by class give exactly this order — class runs, conf descending inside, ties in slot
//                       order (epoch image order, then detection rank)
//     k_metrics_gather  the tp masks in sorted order
//     k_metrics_ap      one workgroup per (t, c): the run's true positives are counted, then the run is walked in tiles of
//                       256 from its END with the cumulative count and the running maximum of the precision carried —
//                       tpc / fpc are integers (exact), recall = tpc / (n_gt + 1e-16), precision = tpc / (tpc + fpc), the
//                       envelope is the reverse running maximum, the area is summed where the recall changes; float64.
//                       One more workgroup: the mean loss (index order), the counts, the status word and the flags.
#include "sel_record.hpp"

#include <rocprim/device/device_radix_sort.hpp>

typedef unsigned long long u64;

constexpr int MET_SLOTS = YOLAT_METRICS_SLOTS;
constexpr int MET_KMAX = 32, MET_TMAX = 32;
constexpr int64_t MET_MAX_SLOTS = 1LL << 27;
constexpr int64_t MET_MAX_BATCHES = 1LL << 24;
constexpr int MET_TILE = 256;                 // elements of a run per step of the walk = threads of the workgroup

struct MetRecord {
  float* conf; int* cls; unsigned* tp; u64* gt_hist; u64* stats; float* loss; int* flags; int* status;
};

// a class id stored as fp32 (det column 5, gt_labels): its integer value, or -1 when it is not an integer in [0, K)
__device__ __forceinline__ int met_class_of(float v, int K) {
  return (v >= 0.f && v < (float)K && v == floorf(v)) ? (int)v : -1;
}

static __global__ void __launch_bounds__(256) k_metrics_append(MetRecord rec, const float* __restrict__ det,
                                                              const int* __restrict__ det_count,
                                                              const uint8_t* __restrict__ tp, const int* __restrict__ stats,
                                                              const float* __restrict__ loss,
                                                              const float* __restrict__ gt_labels, int G,
                                                              const int* __restrict__ sel, int B, int T, int K,
                                                              long image_base, int batch_index) {
  const int tid = threadIdx.x, b = blockIdx.x;
  int tree = 0, status = 0;
  if (sel != nullptr) { tree = sel[YL_SEL_TREE]; status = sel[YL_SEL_STATUS]; }
  const bool clean = tree == 0 && status == 0;
  if (b == B) {
    if (sel != nullptr && tid == 0) {
      rec.flags[2 * batch_index] = tree;
      rec.flags[2 * batch_index + 1] = status;
    }
    if (!clean) return;
    for (int g = tid; g < G; g += 256) {
      const int c = met_class_of(gt_labels[g], K);
      if (c >= 0) atomicAdd(&rec.gt_hist[c], 1ull);
      else atomicOr(rec.status, YOLAT_METRICS_BAD_GT_LABEL);
    }
    for (int c = tid; c < 2 + K * K; c += 256) {
      const int n = stats[c];
      if (n != 0) atomicAdd(&rec.stats[c], (u64)(long long)n);
    }
    if (tid == 0) rec.loss[batch_index] = loss[0];
    return;
  }
  if (!clean) return;
  const int n = yl_min(yl_max(det_count[b], 0), MET_SLOTS);
  const size_t slot0 = (size_t)(image_base + b) * MET_SLOTS;
  for (int r = tid; r < MET_SLOTS; r += 256) {
    float conf = 0.f;
    int cls = -1;
    unsigned mask = 0u;
    if (r < n) {
      const float* row = det + ((size_t)b * MET_SLOTS + r) * 6;
      conf = row[4];
      cls = met_class_of(row[5], K);         // a class outside [0, K) is a class no target has: the slot stays unfilled
      for (int t = 0; t < T; ++t) mask |= (tp[((size_t)t * B + b) * MET_SLOTS + r] != 0 ? 1u : 0u) << t;
    }
    rec.conf[slot0 + r] = conf;
    rec.cls[slot0 + r] = cls;
    rec.tp[slot0 + r] = mask;
  }
}

// descending-order image of a score: larger score -> smaller word.  -0 counts as +0 (numpy's -conf ties them); a NaN takes
// the largest word and so the end of its class run, where numpy's argsort puts it (-inf maps to 0xFF800000, below it)
__device__ __forceinline__ unsigned met_desc_bits(float s) {
  if (s != s) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(s + 0.f);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

static __global__ void __launch_bounds__(256) k_metrics_keys(const float* __restrict__ conf, const int* __restrict__ cls,
                                                            int n, int K, u64* __restrict__ keys,
                                                            unsigned* __restrict__ slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = cls[i];
  const bool filled = c >= 0 && c < K;
  keys[i] = ((u64)(unsigned)(filled ? c : K) << 32) | (u64)(filled ? met_desc_bits(conf[i]) : 0u);
  slots[i] = (unsigned)i;
}

static __global__ void __launch_bounds__(256) k_metrics_gather(const unsigned* __restrict__ tp,
                                                              const unsigned* __restrict__ order, int n,
                                                              unsigned* __restrict__ tps) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) tps[j] = tp[yl_min((int)order[j], n - 1)];
}

// ---- workgroup primitives of 4 waves x 64 lanes; every thread of the workgroup calls them ----
// inclusive prefix sum over the 256 threads; total = the sum of all
__device__ __forceinline__ int met_scan_sum(int v, int lane, int wave, int* wbuf, int& total) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) wbuf[wave] = v;
  __syncthreads();
  int add = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int s = wbuf[w];
    if (w < wave) add += s;
    tot += s;
  }
  total = tot;
  __syncthreads();
  return v + add;
}
// inclusive SUFFIX maximum over the 256 threads (thread i: max over threads >= i); total = the maximum of all
__device__ __forceinline__ double met_suffix_max(double v, int lane, int wave, double* wbuf, double& total) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_down(v, d, 64);
    if (lane + d < 64) v = fmax(v, o);
  }
  if (lane == 0) wbuf[wave] = v;
  __syncthreads();
  double m = v, tot = wbuf[0];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const double s = wbuf[w];
    if (w > wave) m = fmax(m, s);
    tot = fmax(tot, s);
  }
  total = tot;
  __syncthreads();
  return m;
}
// the sum over the 256 threads in a fixed tree
__device__ __forceinline__ double met_block_sum(double v, int lane, int wave, double* wbuf) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane == 0) wbuf[wave] = v;
  __syncthreads();
  const double s = ((wbuf[0] + wbuf[1]) + wbuf[2]) + wbuf[3];
  __syncthreads();
  return s;
}

// first position of the sorted keys whose class is >= c
__device__ __forceinline__ int met_lower_bound(const u64* __restrict__ keys, int n, int c) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int)(keys[mid] >> 32) < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct MetOut {
  double *ap, *p, *r; long long *n_gt, *n_p; double* loss_mean; long long *stats, *status; int* flags;
};

static __global__ void __launch_bounds__(256) k_metrics_ap(MetRecord rec, const u64* __restrict__ keys,
                                                          const unsigned* __restrict__ tps, int n, int T, int K,
                                                          int n_batches, MetOut out) {
  __shared__ int run[2];
  __shared__ int wi[4];
  __shared__ double wd[4];
  __shared__ double chunk[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x == T * K) {
    // the epoch's scalars: the loss in index order, 256 values staged at a time and added by one thread
    double sum = 0.0;
    for (int b0 = 0; b0 < n_batches; b0 += 256) {
      chunk[tid] = b0 + tid < n_batches ? (double)rec.loss[b0 + tid] : 0.0;
      __syncthreads();
      if (tid == 0) {
        const int m = yl_min(256, n_batches - b0);
        for (int i = 0; i < m; ++i) sum += chunk[i];
      }
      __syncthreads();
    }
    if (tid == 0) {
      out.loss_mean[0] = sum / (double)n_batches;
      out.status[0] = (long long)rec.status[0];
    }
    for (int c = tid; c < 2 + K * K; c += 256) out.stats[c] = (long long)rec.stats[c];
    for (int i = tid; i < 2 * n_batches; i += 256) out.flags[i] = rec.flags[i];
    return;
  }
  const int t = blockIdx.x / K, c = blockIdx.x - t * K;
  if (tid == 0) {
    const int lo = met_lower_bound(keys, n, c);
    run[0] = lo;
    run[1] = met_lower_bound(keys, n, c + 1) - lo;
  }
  __syncthreads();
  const int start = run[0], n_p = run[1];
  const long long n_gt = (long long)rec.gt_hist[c];
  if (t == 0 && tid == 0) { out.n_gt[c] = n_gt; out.n_p[c] = n_p; }
  double ap = 0.0, prec_last = 0.0, rec_last = 0.0;
  if (n_gt > 0 && n_p > 0) {                    // (uniform over the workgroup)
    int mine = 0;
    for (int j = tid; j < n_p; j += MET_TILE) mine += (int)((tps[start + j] >> t) & 1u);
    int tp_total;
    (void)met_scan_sum(mine, lane, wave, wi, tp_total);
    const double denom = (double)n_gt + 1e-16;
    int end_tpc = tp_total;                     // true positives up to the end of the current tile
    double carry = 0.0;                         // the envelope behind the current tile; the sentinel mpre[-1] = 0
    for (int tile = (n_p - 1) / MET_TILE; tile >= 0; --tile) {
      const int j = tile * MET_TILE + tid;
      const bool live = j < n_p;
      const int bit = live ? (int)((tps[start + yl_min(j, n_p - 1)] >> t) & 1u) : 0;
      int tile_sum;
      const int incl = met_scan_sum(bit, lane, wave, wi, tile_sum);
      const int tpc = end_tpc - tile_sum + incl;                // tpc + fpc = j + 1
      const double prec = live ? (double)tpc / (double)(j + 1) : 0.0;
      double tile_max;
      const double env = fmax(met_suffix_max(prec, lane, wave, wd, tile_max), carry);
      const double r1 = (double)tpc / denom, r0 = (double)(tpc - bit) / denom;
      const double term = (live && r1 != r0) ? (r1 - r0) * env : 0.0;
      ap += met_block_sum(term, lane, wave, wd);
      carry = fmax(carry, tile_max);
      end_tpc -= tile_sum;
    }
    prec_last = (double)tp_total / (double)n_p;
    rec_last = (double)tp_total / denom;
  }
  if (tid == 0) {
    out.ap[t * K + c] = ap;
    out.p[t * K + c] = prec_last;
    out.r[t * K + c] = rec_last;
  }
}

namespace {
inline size_t met_al(size_t v) { return (v + 255) & ~(size_t)255; }
bool met_record_ok(int64_t cap, int64_t K, int64_t bcap) {
  return cap >= 1 && cap * MET_SLOTS <= MET_MAX_SLOTS && K >= 2 && K <= MET_KMAX && bcap >= 1 && bcap <= MET_MAX_BATCHES;
}
// conf | cls | tp | gt_hist | stats | loss | batch_flags | status, every section at a multiple of 256 bytes
size_t met_layout(int64_t cap, int64_t K, int64_t bcap, int64_t* offs) {
  const size_t S = (size_t)cap * MET_SLOTS;
  const size_t bytes[8] = {4 * S, 4 * S, 4 * S, 8 * (size_t)K, 8 * (size_t)(2 + K * K), 4 * (size_t)bcap,
                           8 * (size_t)bcap, 4};
  size_t o = 0;
  for (int i = 0; i < 8; ++i) {
    if (offs) offs[i] = (int64_t)o;
    o = met_al(o + bytes[i]);
  }
  return o;
}
MetRecord met_record(void* record, int64_t cap, int64_t K, int64_t bcap) {
  int64_t o[8];
  (void)met_layout(cap, K, bcap, o);
  char* b = reinterpret_cast<char*>(record);
  MetRecord r;
  r.conf = reinterpret_cast<float*>(b + o[0]); r.cls = reinterpret_cast<int*>(b + o[1]);
  r.tp = reinterpret_cast<unsigned*>(b + o[2]); r.gt_hist = reinterpret_cast<u64*>(b + o[3]);
  r.stats = reinterpret_cast<u64*>(b + o[4]); r.loss = reinterpret_cast<float*>(b + o[5]);
  r.flags = reinterpret_cast<int*>(b + o[6]); r.status = reinterpret_cast<int*>(b + o[7]);
  return r;
}
bool met_final_ok(int64_t n_images, int64_t T, int64_t K) {
  return n_images >= 1 && n_images * MET_SLOTS <= MET_MAX_SLOTS && T >= 1 && T <= MET_TMAX && K >= 2 && K <= MET_KMAX;
}
struct MetPlan { size_t off_keys, off_skeys, off_slots, off_order, off_tmp, tmp_bytes, total; };
MetPlan met_plan(int64_t n) {
  MetPlan p;
  size_t tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                  (unsigned*)nullptr, (size_t)n, 0, 38, (hipStream_t)0);
  size_t off = 0;
  p.off_keys = off; off = met_al(off + sizeof(u64) * n);
  p.off_skeys = off; off = met_al(off + sizeof(u64) * n);
  p.off_slots = off; off = met_al(off + sizeof(unsigned) * n);      // the iota, then the tp masks in sorted order
  p.off_order = off; off = met_al(off + sizeof(unsigned) * n);
  p.off_tmp = off; off = met_al(off + tmp);
  p.tmp_bytes = tmp; p.total = off + 256;
  return p;
}
size_t met_out_words(int64_t T, int64_t K) { return (size_t)(3 * T * K + 2 * K + 1 + 2 + K * K + 1); }

int met_append(void* record, int64_t cap, int64_t K, int64_t bcap, const float* det, const int32_t* det_count,
               const uint8_t* tp, const int32_t* stats, const float* loss, const float* gt_labels, int64_t G,
               const int32_t* sel, int64_t B, int64_t T, int64_t image_base, int64_t batch_index, hipStream_t st) {
  if (!record || !det || !det_count || !tp || !stats || !loss || G < 0 || (G > 0 && !gt_labels) || B < 1 || T < 1 ||
      image_base < 0 || batch_index < 0 || cap < 1 || bcap < 1 || K < 2)
    return YOLAT_E_INVALID;
  if (!met_record_ok(cap, K, bcap) || T > MET_TMAX || G >= (1LL << 30) || B > 65536 ||
      (((uintptr_t)record) & 255) != 0)
    return YOLAT_E_UNSUPPORTED;
  if (image_base + B > cap || batch_index >= bcap) return YOLAT_E_INVALID;      // slots the record does not have
  hipLaunchKernelGGL(k_metrics_append, dim3((unsigned)B + 1), dim3(256), 0, st, met_record(record, cap, K, bcap), det,
                     det_count, tp, stats, loss, gt_labels, (int)G, sel, (int)B, (int)T, (int)K, (long)image_base,
                     (int)batch_index);
  YL_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" size_t yolat_metrics_record_bytes(int64_t capacity_images, int64_t K, int64_t batch_cap, int64_t* offsets) {
  if (!met_record_ok(capacity_images, K, batch_cap)) return 0;
  return met_layout(capacity_images, K, batch_cap, offsets);
}

extern "C" int yolat_metrics_reset(void* record, int64_t capacity_images, int64_t K, int64_t batch_cap,
                                   yolat_stream_t stream) {
  if (!record || capacity_images < 1 || batch_cap < 1 || K < 2) return YOLAT_E_INVALID;
  if (!met_record_ok(capacity_images, K, batch_cap) || (((uintptr_t)record) & 255) != 0) return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  int64_t o[8];
  const size_t total = met_layout(capacity_images, K, batch_cap, o);
  hipError_t e = hipMemsetAsync(record, 0, total, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(reinterpret_cast<char*>(record) + o[1], 0xFF, 4 * (size_t)capacity_images * MET_SLOTS, st);   // cls = -1
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int yolat_metrics_append(void* record, int64_t capacity_images, int64_t K, int64_t batch_cap, const float* det,
                                    const int32_t* det_count, const uint8_t* tp, const int32_t* stats, const float* loss,
                                    const float* gt_labels, int64_t G, const int32_t* sel, int64_t B, int64_t T,
                                    int64_t image_base, int64_t batch_index, yolat_stream_t stream) {
  if (!sel) return YOLAT_E_INVALID;
  return met_append(record, capacity_images, K, batch_cap, det, det_count, tp, stats, loss, gt_labels, G, sel, B, T,
                    image_base, batch_index, (hipStream_t)stream);
}

extern "C" int yolat_metrics_append_host(void* record, int64_t capacity_images, int64_t K, int64_t batch_cap,
                                         const float* det, const int32_t* det_count, const uint8_t* tp,
                                         const int32_t* stats, const float* loss, const float* gt_labels, int64_t G,
                                         int64_t B, int64_t T, int64_t image_base, int64_t batch_index,
                                         yolat_stream_t stream) {
  return met_append(record, capacity_images, K, batch_cap, det, det_count, tp, stats, loss, gt_labels, G, nullptr, B, T,
                    image_base, batch_index, (hipStream_t)stream);
}

extern "C" size_t yolat_metrics_finalize_work_bytes(int64_t n_images, int64_t T, int64_t K) {
  if (!met_final_ok(n_images, T, K)) return 0;
  return met_plan(n_images * MET_SLOTS).total;
}

extern "C" size_t yolat_metrics_out_bytes(int64_t T, int64_t K, int64_t n_batches) {
  if (T < 1 || T > MET_TMAX || K < 2 || K > MET_KMAX || n_batches < 1 || n_batches > MET_MAX_BATCHES) return 0;
  return 8 * met_out_words(T, K) + 8 * (size_t)n_batches;
}

extern "C" int yolat_metrics_finalize(const void* record, int64_t capacity_images, int64_t K, int64_t batch_cap,
                                      int64_t n_images, int64_t n_batches, int64_t T, void* out, size_t out_bytes,
                                      void* work, size_t work_bytes, yolat_stream_t stream) {
  if (!record || !out || !work || capacity_images < 1 || batch_cap < 1 || K < 2 || n_images < 1 || n_batches < 1 || T < 1)
    return YOLAT_E_INVALID;
  if (!met_record_ok(capacity_images, K, batch_cap) || !met_final_ok(n_images, T, K) ||
      (((uintptr_t)record) & 255) != 0 || (((uintptr_t)work) & 255) != 0 || (((uintptr_t)out) & 7) != 0)
    return YOLAT_E_UNSUPPORTED;
  if (n_images > capacity_images || n_batches > batch_cap) return YOLAT_E_INVALID;
  const int64_t n = n_images * MET_SLOTS;
  const MetPlan p = met_plan(n);
  if (work_bytes < p.total || out_bytes < yolat_metrics_out_bytes(T, K, n_batches)) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const MetRecord rec = met_record(const_cast<void*>(record), capacity_images, K, batch_cap);
  char* base = reinterpret_cast<char*>(work);
  u64* keys = reinterpret_cast<u64*>(base + p.off_keys);
  u64* skeys = reinterpret_cast<u64*>(base + p.off_skeys);
  unsigned* slots = reinterpret_cast<unsigned*>(base + p.off_slots);
  unsigned* order = reinterpret_cast<unsigned*>(base + p.off_order);
  const int nwg = yl_cdiv(n, 256);
  hipLaunchKernelGGL(k_metrics_keys, dim3(nwg), dim3(256), 0, st, rec.conf, rec.cls, (int)n, (int)K, keys, slots);
  YL_LAUNCH_CHECK();
  size_t tmp = p.tmp_bytes;
  if (rocprim::radix_sort_pairs(base + p.off_tmp, tmp, keys, skeys, slots, order, (size_t)n, 0, 38, st) != hipSuccess)
    return YOLAT_E_INVALID;
  unsigned* tps = slots;                        // the iota has been consumed
  hipLaunchKernelGGL(k_metrics_gather, dim3(nwg), dim3(256), 0, st, rec.tp, order, (int)n, tps);
  YL_LAUNCH_CHECK();
  MetOut o;
  double* d = reinterpret_cast<double*>(out);
  long long* q = reinterpret_cast<long long*>(out);
  const size_t TK = (size_t)(T * K);
  o.ap = d; o.p = d + TK; o.r = d + 2 * TK;
  o.n_gt = q + 3 * TK; o.n_p = q + 3 * TK + K;
  o.loss_mean = d + 3 * TK + 2 * K;
  o.stats = q + 3 * TK + 2 * K + 1;
  o.status = o.stats + 2 + K * K;
  o.flags = reinterpret_cast<int*>(o.status + 1);
  hipLaunchKernelGGL(k_metrics_ap, dim3((unsigned)(T * K) + 1), dim3(256), 0, st, rec, skeys, tps, (int)n, (int)T, (int)K,
                     (int)n_batches, o);
  YL_LAUNCH_CHECK();
  return 0;
}
