// base.hpp — shared device helpers for libyolat_hip.so (gfx950 / CDNA4 only).
//
// Hardware model used throughout (MI355X): 64-lane wavefronts, 256-thread workgroups = 4 waves =
// one wave per SIMD, fp32-input MFMA v_mfma_f32_32x32x2_f32 (exact fp32 fma chain, 64 cycles per
// instruction per SIMD), LDS tiles padded by one dword so that the per-lane column reads of the
// MFMA A/B fragments (ds_read_b32, 2 x 32-lane groups) are bank-conflict free.
//
// Loader rule (learned from the ISA): every global load in a staging routine must be UNCONDITIONAL.
// A per-lane "load or zero" branch makes hipcc wrap each load in its own exec-mask region followed
// by s_waitcnt vmcnt(0), i.e. one dependent L2 round trip per element.  So out-of-range rows /
// columns are handled by clamping the address (the loaded value is then discarded by a select, or
// lands in output rows/columns that the epilogue masks) and the aligned interior case is a
// compile-time FAST path with plain 16-byte loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yolat_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define YL_LAUNCH_CHECK()                          \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) return (int)e__;        \
  } while (0)

#define YL_TRY(call)            \
  do {                          \
    int rc__ = (call);          \
    if (rc__ != 0) return rc__; \
  } while (0)

static inline int yl_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline bool yl_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Bump allocation of a whole-forward workspace in 256-byte aligned pieces.  base == nullptr: sizing only (off is the size).
struct Carver {
  char* base; size_t off;
  template <class T> T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};

// A prepared device graph (yolat_graph_csr; collate.hip): YOLAT_E_INVALID unless it holds every array a forward over E edges
// reads.  With a plan, the plan's graph members are pointed at the caller's arrays (the kernels read them, never write).
template <class PlanT>
static inline int yl_adopt_graph(const yolat_graph_csr* g, int64_t E, PlanT* p) {
  if (!g || !g->row_ptr || !g->seg_ptr || !g->node_seg || (E > 0 && (!g->src || !g->dst || !g->attr)))
    return YOLAT_E_INVALID;
  if (p != nullptr) {
    p->row_ptr = const_cast<int*>(g->row_ptr); p->src = const_cast<int*>(g->src); p->dst = const_cast<int*>(g->dst);
    p->attr = const_cast<float*>(g->attr); p->seg_ptr = const_cast<int*>(g->seg_ptr);
    p->node_seg = const_cast<int*>(g->node_seg);
  }
  return 0;
}
// YOLAT_STRICT_FP32=1: every GEMM of the fp32 mode runs on the fp32-input MFMA kernels (v_mfma_f32_32x32x2_f32) instead
// of the bf16x6 emulation (x6.hpp) — the one switch for strict-parity runs (IEEE Inf / NaN propagation, fp32 MFMA
// summation order); the Python side (plan.py, ops.py) reads the same variable.
static inline bool yl_strict_fp32() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("YOLAT_STRICT_FP32"); v = (e && e[0] == '1') ? 1 : 0; }
  return v != 0;
}

// A launch that is the fall-back of another one (conv_local.hip's one-launch conv stack): it runs only when the word at p
// holds val — the epoch the forward raised the flag with — and is a dead launch otherwise.  p == nullptr: always runs.
struct YlGate { const int* p; int val; };
__device__ __forceinline__ bool yl_gate_dead(const YlGate& g) { return g.p != nullptr && *g.p != g.val; }

__device__ __forceinline__ int yl_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int yl_max(int a, int b) { return a > b ? a : b; }
// a*b rounded on its own: the empty asm keeps the compiler from contracting it with a following add into an
// fma (-ffp-contract=fast does that even through __fmul_rn/__fadd_rn), so two kernels that must agree bit
// for bit can pin the same two roundings
__device__ __forceinline__ float yl_mul_rn(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// two floats -> packed bfloat16 pair (a in the low half), round-to-nearest-even: v_cvt_pk_bf16_f32
typedef __bf16 yl_bf16x2 __attribute__((ext_vector_type(2)));
typedef float yl_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned yl_pack_bf16(float a, float b) {
  yl_f32x2 v; v.x = a; v.y = b;
  yl_bf16x2 h = __builtin_convertvector(v, yl_bf16x2);
  return *reinterpret_cast<unsigned*>(&h);
}
__device__ __forceinline__ float yl_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float yl_bf16_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
