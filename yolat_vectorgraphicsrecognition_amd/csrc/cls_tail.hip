// cls_tail.hip — the last two classifier layers of the fp32 eval forward as ONE launch (arch:92-93,128):
//   c2     = relu(bn(c1 . Wc2^T + bc2))      the 32 x 32 split-K tiles of k_gemm_nt_sk (gemm_sk.hpp), statement for statement
//   logits = c2 . Wc3^T + bc3                folded in: no launch of its own, c2 never reaches memory
// Entry points: yl_cls_tail_eval_impl (forward_eval.hip), yolat_debug_cls_tail_eval (tests, tools).
//
// A 32 x 32 tile of c2 holds 32 of a row's H2 columns, so a workgroup can only form a PARTIAL product with Wc3: its slab
//   S[r][c] = sum_{j < 32} c2[row0 + r][col0 + j] * Wc3[c][col0 + j]        (fp32 fma, j ascending, c < n_classes <= 32)
// The H2 / 32 slabs of a row tile are summed by whichever of its workgroups finishes last (DESIGN.md 3l "The classifier
// tail"):
//   * every thread stores 16 bytes of the slab write-through (buffer store, sc1): a wave instruction covers 8 rows x 128 B;
//   * every wave waits for its stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, then ONE lane adds 1 to the
//     row tile's ticket (relaxed, agent scope);
//   * the workgroup whose add returned H2 / 32 - 1 is the reducer: that lane runs an agent-scope acquire (the kernel shares
//     its CU with other workgroups, of this launch and of other streams' launches, so the acquire stays), the workgroup
//     meets at a barrier and reads the slabs with sc1 buffer loads — never a plain load —, adds them in ascending column-tile
//     order, adds bc3, stores the logits and puts the ticket back to 0.
// No floating-point atomics: the logits do not depend on which workgroup arrives last, nor on the order of arrival.
// The tickets must be zero when the launch starts; every launch leaves them zero.
#include "operands.hpp"
#include "epilogue.hpp"
#include "gemm_sk.hpp"
#include "internal.hpp"
#include <stdlib.h>

namespace {
typedef unsigned ct_u32x4 __attribute__((ext_vector_type(4)));

// LDS of the tail, in floats from the start of the body's staging area; [0, 3072) is the reduction's
constexpr int CT_LD = 33;
constexpr int CT_T = 3072;                       // [32][33] the c2 tile, row-major
constexpr int CT_W = CT_T + 32 * CT_LD;          // [32][33] Wc3[c][col0 + j]; rows c >= n_classes are zero
constexpr int CT_B = CT_W + 32 * CT_LD;          // [32] bc3
constexpr int CT_FLAG = CT_B + 32;               // "this workgroup is the reducer"
static_assert(CT_FLAG < 2 * 32 * 129, "the tail's LDS lies inside the staging area");

struct ClsTail {
  const float* W3; long ldw3; const float* b3; int ncls;
  float* logits; long ld_logits;
  float* slabs; unsigned slab_bytes;             // [row tile][column tile][32][32]
  unsigned* tickets;                             // [row tile]
  float* c2; long ldc2;                          // nullable: the c2 tile is stored too (tests)

  struct Pre { float4 w; float b; };
  // thread -> (class c = tid / 8, columns 4 (tid & 7) ..): issued behind the K loop, in flight under the reduction
  __device__ __forceinline__ Pre prefetch(int col0, int tid) const {
    Pre p;
    const int c = tid >> 3, q = tid & 7;
    p.w = c < ncls ? *reinterpret_cast<const float4*>(W3 + (long)c * ldw3 + col0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    p.b = (b3 != nullptr && tid < ncls) ? b3[tid] : 0.f;
    return p;
  }
  __device__ __forceinline__ void park(const Pre& p, float* smem, int tid) const {
    float* d = smem + CT_W + (tid >> 3) * CT_LD + 4 * (tid & 7);
    d[0] = p.w.x; d[1] = p.w.y; d[2] = p.w.z; d[3] = p.w.w;
    if (tid < 32) smem[CT_B + tid] = p.b;
  }
  // wave 0: wave_epilogue's value (bias, scale-shift, floor, + 0 for the absent accumulate term) into LDS instead of Y
  __device__ __forceinline__ void tile(f32x16 acc, int row_base, int col, int lhi, const Epilogue& ep, int M, int N,
                                       const EpiPre& pre, float* smem) const {
    if (ep.bias != nullptr) {
      const float bv = pre.bias;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += bv;
    }
    const float sc = pre.sc, sh = pre.sh;
    const float floor = ep.relu ? 0.f : -INFINITY;
    const int l31 = threadIdx.x & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float v = fmaxf(fmaf(acc[r], sc, sh), floor) + 0.f;
      smem[CT_T + rl * CT_LD + l31] = v;
      if (c2 != nullptr && col < N && row_base + rl < M) c2[(long)(row_base + rl) * ldc2 + col] = v;
    }
  }
  __device__ __forceinline__ void finish(const Pre& p, int rt, int ct, int nct, int M, float* smem, int tid) const {
    park(p, smem, tid);                                     // (beyond the reduction's [3][16][64]: nobody reads there)
    __syncthreads();                                        // the c2 tile and the Wc3 slice are in LDS
    const int r = tid >> 3, q = tid & 7;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
      const float t = smem[CT_T + r * CT_LD + j];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = fmaf(t, smem[CT_W + (4 * q + i) * CT_LD + j], s[i]);
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(slabs, 0, (int)slab_bytes, 0x00020000);
    const unsigned in_slab = (unsigned)(r * 32 + 4 * q) * 4u;
    ct_u32x4 o;
    o.x = __float_as_uint(s[0]); o.y = __float_as_uint(s[1]); o.z = __float_as_uint(s[2]); o.w = __float_as_uint(s[3]);
    __builtin_amdgcn_raw_buffer_store_b128(o, rs, (unsigned)(rt * nct + ct) * 4096u + in_slab, 0, 16);      // aux 16 = sc1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every storing wave, before the barrier the ticket lane joins
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem + CT_FLAG);
    if (tid == 0) {
      const unsigned old = __hip_atomic_fetch_add(tickets + rt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == (unsigned)(nct - 1);
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      *flag = last;
    }
    __syncthreads();
    if (*flag == 0) return;
    // the reducer: slabs in ascending column-tile order, eight loads in flight
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned base = (unsigned)(rt * nct) * 4096u + in_slab;
    for (int t0 = 0; t0 < nct; t0 += 8) {
      ct_u32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + (unsigned)yl_min(t0 + k, nct - 1) * 4096u, 0, 16);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (t0 + k < nct) {
          sum[0] += __uint_as_float(v[k].x); sum[1] += __uint_as_float(v[k].y);
          sum[2] += __uint_as_float(v[k].z); sum[3] += __uint_as_float(v[k].w);
        }
      }
    }
    const int row = rt * 32 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * q + i;
      if (row < M && c < ncls) logits[(long)row * ld_logits + c] = sum[i] + smem[CT_B + c];
    }
    if (tid == 0) __hip_atomic_store(tickets + rt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

__global__ void __launch_bounds__(256) k_cls_tail(DenseOp A, DenseOp B, Epilogue ep, int M, int N, int K, ClsTail tail) {
  constexpr bool B_NFAST = false;
#define YL_SK_TAIL 1
#include "gemm_sk_tile.inc"
#undef YL_SK_TAIL
}

__global__ void k_cls_tail_zero(unsigned* tickets, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tickets[i] = 0u;
}
}  // namespace

// YOLAT_CLS_TAIL_FOLD=0: the two launches (read once)
bool yl_cls_tail_on() {
  static const bool on = []() { const char* v = getenv("YOLAT_CLS_TAIL_FOLD"); return !(v && v[0] == '0'); }();
  return on;
}

// the shapes the fold takes: layer 2 is the split-K launch of launch_gemm_nt (dense.hip), whole 32-column tiles, at most 32 classes
bool yl_cls_tail_shape_ok(int64_t P, int64_t H1, int64_t H2, int64_t n_classes) {
  if (P <= 0 || H1 < 256 || H2 <= 0 || H2 % 32 != 0 || n_classes < 1 || n_classes > 32) return false;
  if ((long)yl_cdiv(P, 64) * yl_cdiv(H2, 64) >= 160) return false;
  return (long)yl_cdiv(P, 32) * (H2 / 32) * 4096L < (1L << 31);
}
size_t yl_cls_tail_ticket_elems(int64_t P) { return (size_t)((yl_cdiv(P, 32) + 63) / 64 * 64); }
size_t yl_cls_tail_slab_elems(int64_t P, int64_t H2) { return (size_t)yl_cdiv(P, 32) * (size_t)yl_cdiv(H2, 32) * 1024; }

int yl_cls_tail_eval_impl(const float* c1, int64_t ldc1, int64_t P, int64_t H1, const float* W2, int64_t ldw2, const float* b2,
                          const float* s2, const float* t2, int64_t H2, const float* W3, int64_t ldw3, const float* b3,
                          int64_t n_classes, float* logits, int64_t ld_logits, uint32_t* tickets, float* slabs, bool primed,
                          float* c2_dbg, int64_t ld_dbg, yolat_stream_t stream) {
  if (!c1 || !W2 || !W3 || !logits || !tickets || !slabs) return YOLAT_E_INVALID;
  if (!yl_cls_tail_shape_ok(P, H1, H2, n_classes)) return YOLAT_E_UNSUPPORTED;
  if (ldc1 < H1 || ldw2 < H1 || ldw3 < H2 || ld_logits < n_classes || (s2 == nullptr) != (t2 == nullptr)) return YOLAT_E_INVALID;
  if (c2_dbg != nullptr && ld_dbg < H2) return YOLAT_E_INVALID;
  if (ldw3 % 4 != 0 || !yl_aligned16(W3) || !yl_aligned16(slabs)) return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int rts = yl_cdiv(P, 32), cts = (int)(H2 / 32);
  if (!primed) {
    hipLaunchKernelGGL(k_cls_tail_zero, dim3(yl_cdiv(rts, 256)), dim3(256), 0, st, tickets, rts);
    YL_LAUNCH_CHECK();
  }
  DenseOp a = yl_dense(c1, ldc1, P, H1), b = yl_dense(W2, ldw2, H2, H1);
  Epilogue ep;
  ep.bias = b2; ep.scale = s2; ep.shift = t2; ep.relu = 1;
  ep.Y = nullptr; ep.ldy = 0; ep.accumulate = 0; ep.stats = nullptr; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  ClsTail t;
  t.W3 = W3; t.ldw3 = ldw3; t.b3 = b3; t.ncls = (int)n_classes; t.logits = logits; t.ld_logits = ld_logits;
  t.slabs = slabs; t.slab_bytes = (unsigned)(yl_cls_tail_slab_elems(P, H2) * 4); t.tickets = tickets;
  t.c2 = c2_dbg; t.ldc2 = ld_dbg;
  hipLaunchKernelGGL(k_cls_tail, dim3(rts, cts), dim3(256), 0, st, a, b, ep, (int)P, (int)H2, (int)H1, t);
  YL_LAUNCH_CHECK();
  return 0;
}

// Classifier layers 2 + 3 (BatchNorm + ReLU behind layer 2) as an op routed the way the eval forward routes them, for tests
// and tools (not part of the C ABI header): the folded launch where it applies (*folded = 1), yolat_linear_fwd twice
// otherwise.  work: yolat_debug_cls_tail_work_bytes bytes, 256-byte aligned — tickets, slabs, c2.  primed != 0: the previous
// use of `work` was this op at the same P and H2 and has been enqueued on the same stream, so the tickets are zero.
// c2_dbg != nullptr receives c2 [P, H2] either way.
extern "C" size_t yolat_debug_cls_tail_work_bytes(int64_t P, int64_t H2) {
  if (P <= 0 || H2 <= 0) return 0;
  return 4 * (yl_cls_tail_ticket_elems(P) + yl_cls_tail_slab_elems(P, H2) + (size_t)(P * H2));
}
extern "C" int yolat_debug_cls_tail_eval(const float* c1, int64_t ldc1, int64_t P, int64_t H1, const float* W2, int64_t ldw2,
                                         const float* b2, const float* s2, const float* t2, int64_t H2, const float* W3,
                                         int64_t ldw3, const float* b3, int64_t n_classes, float* logits, int64_t ld_logits,
                                         void* work, int primed, float* c2_dbg, int64_t ld_dbg, int* folded,
                                         yolat_stream_t stream) {
  if (!work || P <= 0 || H2 <= 0 || (((uintptr_t)work) & 255) != 0) return YOLAT_E_INVALID;
  uint32_t* tickets = reinterpret_cast<uint32_t*>(work);
  float* slabs = reinterpret_cast<float*>(work) + yl_cls_tail_ticket_elems(P);
  float* c2 = c2_dbg ? c2_dbg : slabs + yl_cls_tail_slab_elems(P, H2);
  const int64_t ldc2 = c2_dbg ? ld_dbg : H2;
  const bool fold = yl_cls_tail_on() && !yl_strict_fp32() && yl_cls_tail_shape_ok(P, H1, H2, n_classes) && ldw3 % 4 == 0 &&
                    yl_aligned16(W3);
  if (folded) *folded = fold ? 1 : 0;
  if (fold)
    return yl_cls_tail_eval_impl(c1, ldc1, P, H1, W2, ldw2, b2, s2, t2, H2, W3, ldw3, b3, n_classes, logits, ld_logits, tickets,
                                 slabs, primed != 0, c2_dbg, ld_dbg, stream);
  YL_TRY(yolat_linear_fwd(c1, ldc1, P, H1, nullptr, nullptr, 0, W2, ldw2, b2, H2, s2, t2, 1, c2, ldc2, 0, nullptr, stream));
  return yolat_linear_fwd(c2, ldc2, P, H2, nullptr, nullptr, 0, W3, ldw3, b3, n_classes, nullptr, nullptr, 0, logits, ld_logits,
                          0, nullptr, stream);
}
