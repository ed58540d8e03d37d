// subgraph.hip — device-side sub-batch extraction for the two-pass inference of SparseCADGCN.predict
// (cad_recognition/architecture3cc_rpn_gp_iter2.py:153-242).  The reference walks Python lists: `slice_pos`
// / `slice_edge` are concatenations of index ranges, `o2n` is a dict old node id -> new node id, every
// edge is re-indexed through it in a Python loop and `bbox_idx` is renumbered by run length.  Here the
// host only supplies the (start, exclusive-prefix) pairs of the selected ranges; everything of size O(nodes)
// or O(edges) is integer work on the GPU, bit-exact with the loops:
//   node_ids[i]  = start[j] + (i - prefix[j]),  j = the range that contains output slot i (binary search)
//   o2n[old]     = max new id among duplicates  (== "later assignment wins" of the dict, via atomicMax)
//   edge'[q]     = (o2n[edge[eid[q],0]], o2n[edge[eid[q],1]]);  an endpoint outside the subset raises the
//                  YOLAT_STATUS_EDGE_RANGE flag (the reference raises KeyError)
//   bbox_idx'[i] = number of positions 0 < t <= i with bbox_idx[node_ids[t]] != bbox_idx[node_ids[t-1]]
#include "sel_record.hpp"
#include "internal.hpp"

static __global__ void k_expand_ranges(const int* __restrict__ start, const int* __restrict__ prefix, int S,
                                       int total, int* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = S;              // largest j with prefix[j] <= i   (prefix[S] = total > i)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= i) lo = mid; else hi = mid;
  }
  out[i] = start[lo] + (i - prefix[lo]);
}

static __global__ void k_o2n_scatter(const int* __restrict__ node_ids, int n, int* o2n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicMax(&o2n[node_ids[i]], i);
}

static __global__ void k_edge_remap(const int64_t* __restrict__ edge, long se, long sc,
                                    const int* __restrict__ edge_ids, int m, const int* __restrict__ o2n, int N,
                                    int64_t* out, int* status) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;
  const long e = edge_ids[q];
  const int64_t a = edge[e * se], b = edge[e * se + sc];
  const int na = (a >= 0 && a < N) ? o2n[a] : -1;
  const int nb = (b >= 0 && b < N) ? o2n[b] : -1;
  if (na < 0 || nb < 0) atomicOr(status, YOLAT_STATUS_EDGE_RANGE);
  out[2 * (long)q] = na;
  out[2 * (long)q + 1] = nb;
}

// flag[i] = (i > 0 && bbox_idx[node_ids[i]] != bbox_idx[node_ids[i-1]])
static __global__ void k_change_flags(const int64_t* __restrict__ bbox_idx, const int* __restrict__ node_ids, int n,
                                      int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i > 0 && bbox_idx[node_ids[i]] != bbox_idx[node_ids[i - 1]]) ? 1 : 0;
}

// block-local exclusive scan (4096 elements per workgroup) + block totals, then the inclusive result
static __global__ void __launch_bounds__(1024) k_scan_local(const int* flag, int n, int* local, int* btot) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = blockIdx.x * 4096 + tid * 4;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (idx + j < n) ? flag[idx + j] : 0;
  const int t = v[0] + v[1] + v[2] + v[3];
  int incl = t;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int nb = __shfl_up(incl, off);
    if (lane >= off) incl += nb;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int woff = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const int s = wsum[w];
    if (w < wave) woff += s;
    total += s;
  }
  int excl = woff + incl - t;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (idx + j < n) local[idx + j] = excl;
    excl += v[j];
  }
  if (tid == 0) btot[blockIdx.x] = total;
}

static __global__ void k_renumber(const int* flag, const int* local, const int* btot, int n, int64_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int base = 0;
  for (int b = 0; b < i / 4096; ++b) base += btot[b];
  out[i] = (int64_t)(base + local[i] + flag[i]);
}

static __global__ void k_gather_rows_any(const char* __restrict__ src, long src_row_bytes,
                                         const int* __restrict__ idx, long rows, int row_bytes, char* dst,
                                         long dst_row_bytes) {
  // rows are multiples of 4 bytes (fp32 / int32 / int64 payloads): one 4-byte word per thread
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int words = row_bytes >> 2;
  const long r = i / words;
  const int w = (int)(i % words);
  if (r >= rows) return;
  reinterpret_cast<int*>(dst + r * dst_row_bytes)[w] =
      reinterpret_cast<const int*>(src + (long)idx[r] * src_row_bytes)[w];
}

extern "C" int yolat_expand_ranges(const int32_t* start, const int32_t* prefix, int64_t S, int64_t total,
                                   int32_t* out, yolat_stream_t stream) {
  if (S < 0 || total < 0 || total >= (1LL << 31)) return YOLAT_E_INVALID;
  if (total == 0) return 0;
  if (S == 0 || !start || !prefix || !out) return YOLAT_E_INVALID;
  hipLaunchKernelGGL(k_expand_ranges, dim3(yl_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, start, prefix,
                     (int)S, (int)total, out);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t yolat_subgraph_work_elems(int64_t N, int64_t n_sub) {
  return (size_t)(N + 2 * n_sub + (n_sub + 4095) / 4096 + 16);
}

extern "C" int yolat_subgraph_reindex(const int32_t* node_ids, int64_t n_sub, int64_t N, const int64_t* edge,
                                      int64_t stride_e, int64_t stride_c, const int32_t* edge_ids, int64_t m_sub,
                                      const int64_t* bbox_idx, int64_t* edge_out, int64_t* bbox_idx_out,
                                      int32_t* work, int32_t* status, yolat_stream_t stream) {
  if (N <= 0 || n_sub < 0 || m_sub < 0 || !work || !status || N >= (1LL << 31)) return YOLAT_E_INVALID;
  if (n_sub > 0 && (!node_ids || !bbox_idx || !bbox_idx_out)) return YOLAT_E_INVALID;
  if (m_sub > 0 && (!edge || !edge_ids || !edge_out)) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  int* o2n = work;                       // [N]
  int* flag = o2n + N;                   // [n_sub]
  int* local = flag + n_sub;             // [n_sub]
  int* btot = local + n_sub;             // [ceil(n_sub / 4096)]
  if (hipMemsetAsync(o2n, 0xFF, sizeof(int) * (size_t)N, st) != hipSuccess) return YOLAT_E_INVALID;   // -1
  if (n_sub > 0) {
    hipLaunchKernelGGL(k_o2n_scatter, dim3(yl_cdiv(n_sub, 256)), dim3(256), 0, st, node_ids, (int)n_sub, o2n);
    YL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_change_flags, dim3(yl_cdiv(n_sub, 256)), dim3(256), 0, st, bbox_idx, node_ids, (int)n_sub,
                       flag);
    YL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_local, dim3(yl_cdiv(n_sub, 4096)), dim3(1024), 0, st, flag, (int)n_sub, local, btot);
    YL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_renumber, dim3(yl_cdiv(n_sub, 256)), dim3(256), 0, st, flag, local, btot, (int)n_sub,
                       bbox_idx_out);
    YL_LAUNCH_CHECK();
  }
  if (m_sub > 0) {
    hipLaunchKernelGGL(k_edge_remap, dim3(yl_cdiv(m_sub, 256)), dim3(256), 0, st, edge, (long)stride_e, (long)stride_c,
                       edge_ids, (int)m_sub, o2n, (int)N, edge_out, status);
    YL_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int yolat_gather_rows_bytes(const void* src, int64_t src_row_bytes, const int32_t* idx, int64_t rows,
                                       int64_t row_bytes, void* dst, int64_t dst_row_bytes, yolat_stream_t stream) {
  if (rows < 0 || row_bytes <= 0 || row_bytes % 4 != 0 || src_row_bytes < row_bytes || dst_row_bytes < row_bytes)
    return YOLAT_E_INVALID;
  if (rows == 0) return 0;
  if (!src || !idx || !dst) return YOLAT_E_INVALID;
  hipLaunchKernelGGL(k_gather_rows_any, dim3(yl_cdiv(rows * (row_bytes / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                     (const char*)src, (long)src_row_bytes, idx, (long)rows, (int)row_bytes, (char*)dst,
                     (long)dst_row_bytes);
  YL_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Offset fix-up of a collated batch (cad_recognition/train.py:238-258): every edge endpoint of image b gets
// + node_off[b] (= slices['pos'][b]) and every bbox_idx entry + prop_off[b] (= slices['labels'][b]).  The
// reference loops over the images with sliced in-place adds; here one launch, the image of an element is
// found by binary search in the per-image slice pointers.  Integer, bit-exact.
// -------------------------------------------------------------------------------------------------
static __device__ __forceinline__ int item_of(const int64_t* ptr, int B, long i) {
  int lo = 0, hi = B;               // largest b with ptr[b] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

static __global__ void k_fixup_offsets(int64_t* edge, long E, const int64_t* edge_ptr, int64_t* bbox_idx, long N,
                                       const int64_t* node_ptr, const int64_t* node_off, const int64_t* prop_off,
                                       int B) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < E) {
    const int64_t o = node_off[item_of(edge_ptr, B, i)];
    edge[2 * i] += o;
    edge[2 * i + 1] += o;
  }
  if (i < N) bbox_idx[i] += prop_off[item_of(node_ptr, B, i)];
}

extern "C" int yolat_fixup_offsets(int64_t* edge, int64_t E, const int64_t* edge_ptr, int64_t* bbox_idx, int64_t N,
                                   const int64_t* node_ptr, const int64_t* node_off, const int64_t* prop_off,
                                   int64_t B, yolat_stream_t stream) {
  if (E < 0 || N < 0 || B <= 0 || !edge_ptr || !node_ptr || !node_off || !prop_off) return YOLAT_E_INVALID;
  if ((E > 0 && !edge) || (N > 0 && !bbox_idx)) return YOLAT_E_INVALID;
  const long n = E > N ? E : N;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_fixup_offsets, dim3(yl_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, edge, (long)E, edge_ptr,
                     bbox_idx, (long)N, node_ptr, node_off, prop_off, (int)B);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// predict() in ONE submission (round 6).  Reference: SparseCADGCN.predict, architecture3cc_rpn_gp_iter2.py:139-356 — pass 1
// over the root proposals, `has_object` (:259-281: arg-max == n_classes - 1) decides which roots get their children
// evaluated in pass 2, per image the root rows are followed by the child rows (:317-328).
//
// In eval mode a proposal's logits depend on nothing but its own nodes and edges (BatchNorm on running statistics,
// block-diagonal adjacency, per-proposal pooling: Datasets/graph_dict3.py:582-600,733), so the logits of every root and
// every child are rows of ONE forward over the whole batch, and the second pass's SIZE no longer has to reach the host
// before anything can be enqueued.  What is left of the two passes is integer work on the device:
//   k_predict_validate  the tree's (idx_pos, idx_edge) ranges must be exactly its proposals' node / edge ranges (seg_ptr /
//                       eptr of yl_local_prep) and no edge may leave its proposal — otherwise the sub-batches of the
//                       reference are NOT the proposals of the batch (duplicates, foreign edges -> its KeyError) and the
//                       caller falls back to the two-pass extraction (flag in out[1])
//   k_predict_select    has_object per root (yl_argmax_row == K - 1: torch's max(1)[1], the rule of the two-pass path),
//                       exclusive scan of the selected children, per image offsets
//                       (slice_image_bbox), and the proposal row of every output row (slice_bbox) in the reference's order
//   k_predict_gather    logits / boxes of those rows, boxes enlarged by 5 % about their centre (:341-346, same fp32 steps)
// One host read (out[]: total, flag, slice_image_bbox, rows) ends the call.
// ------------------------------------------------------------------------------------------------
static __global__ void k_predict_zero(int* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

static __global__ void __launch_bounds__(256) k_predict_validate(yolat_predict_tree t, const int* __restrict__ seg_ptr,
                                                                 const int* __restrict__ eptr, int P, const int* info,
                                                                 const int* status, int* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long R = t.R, C = t.Ctot;
  if (i == 0 && (info[0] != 0 || status[0] != 0)) atomicOr(out + YL_SEL_TREE, 2);
  if (i >= R + C) return;
  const bool root = i < R;
  const long j = root ? i : i - R;
  const int row = root ? t.root_row[j] : t.child_row[j];
  const int* rg = (root ? t.root_range : t.child_range) + 4 * j;       // pos_s, pos_e, edge_s, edge_e
  bool ok = row >= 0 && row < P;
  if (ok) ok = rg[0] == seg_ptr[row] && rg[1] == seg_ptr[row + 1] && rg[2] == eptr[row] && rg[3] == eptr[row + 1];
  if (!ok) atomicOr(out + YL_SEL_TREE, 1);
}

// one workgroup: R roots (a few thousand at most per batch)
static __global__ void __launch_bounds__(1024) k_predict_select(yolat_predict_tree t, const float* __restrict__ logits, long ld,
                                                                int K, int P, int* sel_off, int* out) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = (int)t.R, B = (int)t.B;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < R; r0 += 1024) {
    const int r = r0 + tid;
    int n = 0;
    if (r < R) {
      const int row = t.root_row[r];
      if (row >= 0 && row < P) {
        if (yl_argmax_row(logits + (long)row * ld, K) == K - 1) n = t.child_ptr[r + 1] - t.child_ptr[r];
      }
    }
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int nb = __shfl_up(incl, off);
      if (lane >= off) incl += nb;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int s = wsum[w];
      if (w < wave) woff += s;
      total += s;
    }
    const int carry = carry_s;
    if (r < R) sel_off[r] = carry + woff + incl - n;
    __syncthreads();
    if (tid == 0) carry_s = carry + total;
    __syncthreads();
  }
  if (tid == 0) sel_off[R] = carry_s;
  __syncthreads();
  const int total_children = carry_s;
  int* image_off = yl_sel_image_off(out);        // [B + 1]
  int* rows = yl_sel_rows(out, B);               // [R + Ctot]
  for (int i = tid; i <= B; i += 1024) {
    const int r = t.image_root_ptr[i];
    image_off[i] = r + sel_off[r];
  }
  if (tid == 0) out[YL_SEL_TOTAL] = R + total_children;
  for (int r = tid; r < R; r += 1024) {
    int lo = 0, hi = B;                          // image of root r: largest i with image_root_ptr[i] <= r
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (t.image_root_ptr[mid] <= r) lo = mid; else hi = mid;
    }
    const int r_lo = t.image_root_ptr[lo], r_hi = t.image_root_ptr[lo + 1];
    const int base = r_lo + sel_off[r_lo];
    rows[base + (r - r_lo)] = t.root_row[r];
    const int n = sel_off[r + 1] - sel_off[r];
    const int c0 = t.child_ptr[r];
    const int cb = base + (r_hi - r_lo) + (sel_off[r] - sel_off[r_lo]);
    for (int j = 0; j < n; ++j) rows[cb + j] = t.child_row[c0 + j];
  }
}

static __global__ void __launch_bounds__(256) k_predict_gather(const float* __restrict__ logits, long ld, int K,
                                                               const float* __restrict__ bbox, const int* __restrict__ rows,
                                                               int total, int P, float* out_cls, float* out_bbox) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)total * (K + 4)) return;
  const int r = (int)(i / (K + 4)), c = (int)(i - (long)r * (K + 4));
  int row = rows[r];
  row = row < 0 ? 0 : (row >= P ? P - 1 : row);
  if (c < K) { out_cls[(long)r * K + c] = logits[(long)row * ld + c]; return; }
  const float x1 = bbox[4l * row], y1 = bbox[4l * row + 1], x2 = bbox[4l * row + 2], y2 = bbox[4l * row + 3];
  // arch:341-346: w = (x2 - x1) * 1.05, h = ..., cx = (x2 + x1) / 2, cy = ...; [cx - w/2, cy - h/2, cx + w/2, cy + h/2]
  const float w = (x2 - x1) * 1.05f, h = (y2 - y1) * 1.05f, cx = (x2 + x1) / 2.f, cy = (y2 + y1) / 2.f;
  const int k = c - K;
  out_bbox[4l * r + k] = k == 0 ? cx - w / 2.f : (k == 1 ? cy - h / 2.f : (k == 2 ? cx + w / 2.f : cy + h / 2.f));
}

extern "C" size_t yolat_predict_select_workspace_bytes(int64_t N, int64_t P, int64_t R) {
  if (N <= 0 || P <= 0 || R < 0) return 0;
  return (size_t)(2 * (P + 1) + N + (R + 1) + 64) * sizeof(int32_t) + 1024;
}

extern "C" int yolat_predict_select(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const int64_t* edge,
                                    int64_t stride_e, int64_t stride_c, const int64_t* bbox_idx, int64_t N, int64_t E,
                                    const yolat_predict_tree* tree, int32_t* out, void* workspace, size_t workspace_bytes,
                                    yolat_stream_t stream) {
  if (!logits || !bbox_idx || !tree || !out || !workspace || P <= 0 || K <= 0 || N <= 0 || E < 0 || (E > 0 && !edge) ||
      ld_logits < K)
    return YOLAT_E_INVALID;
  const yolat_predict_tree& t = *tree;
  if (!yl_predict_tree_ok(t, 0)) return YOLAT_E_INVALID;
  if (N >= (1LL << 30) || E >= (1LL << 30) || P >= (1LL << 30) || t.R + t.Ctot >= (1LL << 30)) return YOLAT_E_UNSUPPORTED;
  if (workspace_bytes < yolat_predict_select_workspace_bytes(N, P, t.R)) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  int32_t* seg_ptr = reinterpret_cast<int32_t*>(base);
  int32_t* eptr = seg_ptr + (P + 1);
  int32_t* node_seg = eptr + (P + 1);
  int32_t* sel_off = node_seg + N;
  int32_t* info = sel_off + (t.R + 1);           // [4] locality flags, then [1] status bits of malformed ids
  int32_t* status = info + 4;
  hipLaunchKernelGGL(k_predict_zero, dim3(1), dim3(64), 0, st, info, 8);
  hipLaunchKernelGGL(k_predict_zero, dim3(1), dim3(64), 0, st, out, YL_SEL_HEAD);
  YL_LAUNCH_CHECK();
  int rc = yl_local_prep(edge, stride_e, stride_c, bbox_idx, N, E, P, seg_ptr, node_seg, eptr, status, info, false, st);
  if (rc != 0) return rc;
  if (t.R + t.Ctot > 0) {
    hipLaunchKernelGGL(k_predict_validate, dim3(yl_cdiv(t.R + t.Ctot, 256)), dim3(256), 0, st, t, seg_ptr, eptr, (int)P, info,
                       status, out);
    YL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_predict_select, dim3(1), dim3(1024), 0, st, t, logits, (long)ld_logits, (int)K, (int)P, sel_off, out);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_predict_gather(const float* logits, int64_t ld_logits, int64_t P, int64_t K, const float* bbox,
                                    const int32_t* rows, int64_t total, float* out_cls, float* out_bbox,
                                    yolat_stream_t stream) {
  if (total < 0 || P <= 0 || K <= 0 || ld_logits < K) return YOLAT_E_INVALID;
  if (total == 0) return 0;
  if (!logits || !bbox || !rows || !out_cls || !out_bbox) return YOLAT_E_INVALID;
  if (total * (K + 4) >= (1LL << 40)) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_predict_gather, dim3(yl_cdiv(total * (K + 4), 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     (long)ld_logits, (int)K, bbox, rows, (int)total, (int)P, out_cls, out_bbox);
  YL_LAUNCH_CHECK();
  return 0;
}
