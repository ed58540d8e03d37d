// operands.hpp — the operand loaders of the GEMM kernels, their host-side constructors and the XCD tile map.
#pragma once
#include "base.hpp"

// ------------------------------------------------------------------------------------------------
// Operand loaders.  load4<FAST>(r, k, v): 4 consecutive k-elements of logical row r (k % 4 == 0).
//   FAST  : caller guarantees `vec` (16-byte loads legal) and k + 3 < cols.
//   !FAST : any alignment / K tail; columns >= cols read as exactly 0.
// Rows >= rows return the (finite or not) contents of the last valid row: every consumer masks
// them (NT GEMM: epilogue row/column masks; TN GEMM: explicit select).
// ------------------------------------------------------------------------------------------------

// Row-major dense operand; PRO adds the per-column affine + ReLU prologue (BatchNorm1d+ReLU of the
// producer applied on the fly):  v = max(v*scale[k] + shift[k], floor),  floor = 0 or -inf.
template <bool PRO>
struct DenseOpT {
  const float* p;
  long ld;
  int rows, cols;
  const float* scale;
  const float* shift;
  float floor;
  int vec;  // ld % 4 == 0, base (and scale/shift) 16-byte aligned

  template <bool FAST>
  __device__ __forceinline__ void load4(int r, int k, float v[4]) const {
    const float* q = p + (long)yl_min(r, rows - 1) * ld;
    if (FAST) {
      const float4 t = *reinterpret_cast<const float4*>(q + k);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      if (PRO) {
        const float4 s = *reinterpret_cast<const float4*>(scale + k);
        const float4 h = *reinterpret_cast<const float4*>(shift + k);
        v[0] = fmaxf(fmaf(v[0], s.x, h.x), floor);
        v[1] = fmaxf(fmaf(v[1], s.y, h.y), floor);
        v[2] = fmaxf(fmaf(v[2], s.z, h.z), floor);
        v[3] = fmaxf(fmaf(v[3], s.w, h.w), floor);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kc = yl_min(k + j, cols - 1);
        float t = q[kc];
        if (PRO) t = fmaxf(fmaf(t, scale[kc], shift[kc]), floor);
        v[j] = (k + j < cols) ? t : 0.f;
      }
    }
  }
};
typedef DenseOpT<false> DenseOp;
typedef DenseOpT<true> DenseProOp;

// bfloat16-STORED dense operand (training with bf16 storage of the [E,*] tensors, train_bf16.hip): the same loader
// contract, elements converted to fp32 while loading (bf16 -> fp32 is a 16-bit shift: exact), prologue in fp32.
typedef unsigned short yl_bf16_t;
__device__ __forceinline__ float4 yl_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 yl_ld4(const yl_bf16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(yl_bf16_lo(u.x), yl_bf16_hi(u.x), yl_bf16_lo(u.y), yl_bf16_hi(u.y));
}
__device__ __forceinline__ void yl_st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void yl_st4(yl_bf16_t* p, const float4& v) {       // round-to-nearest-even
  uint2 u;
  u.x = yl_pack_bf16(v.x, v.y); u.y = yl_pack_bf16(v.z, v.w);
  *reinterpret_cast<uint2*>(p) = u;
}
__device__ __forceinline__ float yl_ld1(const float* p) { return *p; }
__device__ __forceinline__ float yl_ld1(const yl_bf16_t* p) { return __uint_as_float(((unsigned)*p) << 16); }

template <bool PRO>
struct HalfOpT {
  const yl_bf16_t* p;
  long ld;
  int rows, cols;
  const float* scale;
  const float* shift;
  float floor;
  int vec;  // ld % 4 == 0, base 8-byte aligned (and scale/shift 16-byte aligned)

  template <bool FAST>
  __device__ __forceinline__ void load4(int r, int k, float v[4]) const {
    const yl_bf16_t* q = p + (long)yl_min(r, rows - 1) * ld;
    if (FAST) {
      const float4 t = yl_ld4(q + k);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      if (PRO) {
        const float4 s = *reinterpret_cast<const float4*>(scale + k);
        const float4 h = *reinterpret_cast<const float4*>(shift + k);
        v[0] = fmaxf(fmaf(v[0], s.x, h.x), floor);
        v[1] = fmaxf(fmaf(v[1], s.y, h.y), floor);
        v[2] = fmaxf(fmaf(v[2], s.z, h.z), floor);
        v[3] = fmaxf(fmaf(v[3], s.w, h.w), floor);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kc = yl_min(k + j, cols - 1);
        float t = yl_ld1(q + kc);
        if (PRO) t = fmaxf(fmaf(t, scale[kc], shift[kc]), floor);
        v[j] = (k + j < cols) ? t : 0.f;
      }
    }
  }
};
typedef HalfOpT<false> HalfOp;
typedef HalfOpT<true> HalfProOp;

// Dense operand used transposed: logical element (r, k) = p[k*ld + r]  (r fast in memory).
struct TransOp {
  const float* p;
  long ld;
  int rows, cols;
  int vec;  // 1: the element path is already coalesced along r; FAST only skips the K-tail select
  template <bool FAST>
  __device__ __forceinline__ void load4(int r, int k, float v[4]) const {
    const int rc = yl_min(r, rows - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kc = yl_min(k + j, cols - 1);
      const float t = p[(long)kc * ld + rc];
      v[j] = (FAST || k + j < cols) ? t : 0.f;
    }
  }
};

// Edge feature rows of AttrRelativeEdgeConvGlobalPool2.message (torch_vertex.py:331), gathered on
// the fly:  row q (CSR slot) = [ x[dst_q] | x[src_q] - x[dst_q] | attr_q ],  K = 2*Cin + 4.
// Branch-free: two unconditional loads (pa, pb) and a select per segment.
struct EdgeOp {
  const float* x;
  long ldx;
  int Cin;
  const int* src;
  const int* dst;
  const float* attr;  // [E,4] contiguous
  int rows;           // E
  int cols;           // 2*Cin + 4
  int vec;            // Cin % 4 == 0, ldx % 4 == 0, x and attr 16-byte aligned

  template <bool FAST>
  __device__ __forceinline__ void load4(int q, int k, float v[4]) const {
    const int qc = yl_min(q, rows - 1);
    const long s = src[qc], d = dst[qc];
    if (FAST) {
      // a float4 never straddles a segment because Cin % 4 == 0
      const bool seg0 = k < Cin, seg1 = !seg0 && (k < 2 * Cin);
      const int kx = seg0 ? k : (seg1 ? k - Cin : 0);
      const float* pa = seg0 ? x + d * ldx + kx : (seg1 ? x + s * ldx + kx : attr + (long)qc * 4);
      const float* pb = x + d * ldx + kx;
      const float4 a = *reinterpret_cast<const float4*>(pa);
      const float4 b = *reinterpret_cast<const float4*>(pb);
      v[0] = seg1 ? a.x - b.x : a.x;
      v[1] = seg1 ? a.y - b.y : a.y;
      v[2] = seg1 ? a.z - b.z : a.z;
      v[3] = seg1 ? a.w - b.w : a.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        const bool seg0 = kk < Cin, seg1 = !seg0 && (kk < 2 * Cin);
        const bool seg2 = !seg0 && !seg1 && (kk < cols);
        const int kx = seg0 ? kk : (seg1 ? kk - Cin : 0);
        const int ka = seg2 ? kk - 2 * Cin : 0;
        const float xd = x[d * ldx + kx];
        const float xs = x[s * ldx + kx];
        const float at = attr[(long)qc * 4 + ka];
        v[j] = seg0 ? xd : (seg1 ? xs - xd : (seg2 ? at : 0.f));
      }
    }
  }
};

// Combined weight of the edge-MLP input gradient (yolat_edge_lin1_bwd_x): logical (n, k) with
// n in [0, 2*Cin) the input column and k in [0, C) the hidden channel:
//   n <  Cin : W1[k][n] - W1[k][Cin + n]     (gradient reaching x[dst])
//   n >= Cin : W1[k][n]                      (gradient reaching x[src])
struct EdgeWcOp {
  const float* W1;
  long ldw;
  int Cin, C;
  int vec;
  template <bool FAST>
  __device__ __forceinline__ void load4(int n, int k, float v[4]) const {
    const int nc = yl_min(n, 2 * Cin - 1);
    const bool lo = nc < Cin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kc = yl_min(k + j, C - 1);
      const float* row = W1 + (long)kc * ldw;
      const float a = row[nc];
      const float b = row[lo ? Cin + nc : nc];
      const float t = lo ? a - b : a;
      v[j] = (FAST || k + j < C) ? t : 0.f;
    }
  }
};

// XCD-aware workgroup -> tile map.  The dispatcher places linear workgroup id b on XCD b % 8 (observed,
// MI355X_MICROARCH.md "Workgroup dispatch"); each XCD has a private 4 MiB L2.  With the plain (x, y) map
// the gridDim.y workgroups that share one A row-tile land on 8 different XCDs, and every one of them
// pulls the tile over the fabric (PMC: 79 MB fetched for the 5.6 MB fusion GEMM at cfg 2).  Here XCD x
// owns a contiguous range of row-major (row-tile, col-tile) pairs, column tile fastest, so the sharers of
// an A tile run back-to-back on one XCD and hit its L2.  A speed choice only: any placement is correct.
__device__ __forceinline__ int l31_of_lane() { return (int)(threadIdx.x & 31); }

__device__ __forceinline__ void yl_xcd_tile(int& rt, int& ct) {
  const int tm = gridDim.x, tn = gridDim.y;
  const int total = tm * tn, id = blockIdx.x + tm * blockIdx.y;
  const int chunk = total >> 3, rem = total & 7;
  const int xcd = id & 7, slot = id >> 3;
  const int logical = xcd * chunk + (xcd < rem ? xcd : rem) + slot;
  rt = logical / tn;
  ct = logical - rt * tn;
}

// ---- host-side operand constructors --------------------------------------------------------------
static inline DenseOp yl_dense(const float* p, long ld, long rows, long cols) {
  DenseOp d;
  d.p = p; d.ld = ld; d.rows = (int)rows; d.cols = (int)cols;
  d.scale = nullptr; d.shift = nullptr; d.floor = -INFINITY;
  d.vec = (ld % 4 == 0) && yl_aligned16(p);
  return d;
}
static inline DenseProOp yl_dense_pro(const float* p, long ld, long rows, long cols,
                                      const float* scale, const float* shift, int relu) {
  DenseProOp d;
  d.p = p; d.ld = ld; d.rows = (int)rows; d.cols = (int)cols;
  d.scale = scale; d.shift = shift; d.floor = relu ? 0.f : -INFINITY;
  d.vec = (ld % 4 == 0) && yl_aligned16(p) && yl_aligned16(scale) && yl_aligned16(shift);
  return d;
}
static inline HalfOp yl_half(const yl_bf16_t* p, long ld, long rows, long cols) {
  HalfOp d;
  d.p = p; d.ld = ld; d.rows = (int)rows; d.cols = (int)cols;
  d.scale = nullptr; d.shift = nullptr; d.floor = -INFINITY;
  d.vec = (ld % 4 == 0) && ((((uintptr_t)p) & 7) == 0);
  return d;
}
static inline HalfProOp yl_half_pro(const yl_bf16_t* p, long ld, long rows, long cols, const float* scale,
                                    const float* shift, int relu) {
  HalfProOp d;
  d.p = p; d.ld = ld; d.rows = (int)rows; d.cols = (int)cols;
  d.scale = scale; d.shift = shift; d.floor = relu ? 0.f : -INFINITY;
  d.vec = (ld % 4 == 0) && ((((uintptr_t)p) & 7) == 0) && yl_aligned16(scale) && yl_aligned16(shift);
  return d;
}
static inline EdgeOp yl_edge(const float* x, long ldx, long Cin, const int* src, const int* dst,
                             const float* attr, long E) {
  EdgeOp a;
  a.x = x; a.ldx = ldx; a.Cin = (int)Cin; a.src = src; a.dst = dst; a.attr = attr;
  a.rows = (int)E; a.cols = (int)(2 * Cin + 4);
  a.vec = (Cin % 4 == 0) && (ldx % 4 == 0) && yl_aligned16(x) && yl_aligned16(attr);
  return a;
}
