// edge_ops.hip — the single-op edge kernels of AttrRelativeEdgeConvGlobalPool2 (gcn_lib/sparse/torch_vertex.py:288-341)
// on gfx950, used by training and by the eval fall-back: the gathered and the factorised first edge Linear, CSR mean
// aggregation, and their backward (scatter, per-node sums, attr weight gradient, BatchNorm apply + sums, dW1 merge).
// All [E,*] tensors are in destination-sorted (CSR) order, so aggregation reads contiguous rows and needs no atomics.
// The fused eval kernels are in edge.hip.
//
// Ops with a bfloat16-storage twin (`_h`: the [E,64] operand stored as bf16) have ONE host wrapper, a template on the
// operand's element type T = float / yl_bf16_t; where the twins differ, an `if constexpr` names the difference.
#include "operands.hpp"
#include "epilogue.hpp"
#include "gemm_nt.hpp"
#include "gemm_tn.hpp"
#include <type_traits>

// rows of T that the kernels read or write four elements at a time: 16 bytes of float, 8 of bfloat16
template <class T> static inline bool yl_row_aligned(const void* p) { return (((uintptr_t)p) % (4 * sizeof(T))) == 0; }

extern "C" int yolat_edge_lin1_fwd(const float* x, int64_t ldx, int64_t N, int64_t Cin,
                                   const int32_t* src_csr, const int32_t* dst_csr,
                                   const float* attr_csr, int64_t E, const float* W1, int64_t ldw,
                                   const float* b1, int64_t C, const float* o_scale,
                                   const float* o_shift, int o_relu, float* H1, int64_t ldh,
                                   float* stats, yolat_stream_t stream) {
  if (E < 0 || N <= 0 || Cin <= 0 || C <= 0 || !x || !W1) return YOLAT_E_INVALID;
  if (E == 0) return 0;
  if (!src_csr || !dst_csr || !attr_csr || !H1 || E >= (1LL << 31)) return YOLAT_E_INVALID;
  const long K = 2 * Cin + 4;
  if (ldw < K || ldh < C || ldx < Cin) return YOLAT_E_INVALID;
  if ((o_scale == nullptr) != (o_shift == nullptr)) return YOLAT_E_INVALID;
  EdgeOp a = yl_edge(x, ldx, Cin, src_csr, dst_csr, attr_csr, E);
  DenseOp b = yl_dense(W1, ldw, C, K);
  Epilogue ep;
  ep.bias = b1; ep.scale = o_scale; ep.shift = o_shift; ep.relu = o_relu;
  ep.Y = H1; ep.ldy = ldh; ep.accumulate = 0; ep.stats = stats; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(yl_cdiv(E, 64), yl_cdiv(C, 64));
  if (K <= 16)
    hipLaunchKernelGGL((k_gemm_nt<64, 64, 16, EdgeOp, DenseOp, false>), grid, dim3(256), 0, st, a,
                       b, ep, (int)E, (int)C, (int)K);
  else
    hipLaunchKernelGGL((k_gemm_nt<64, 64, 32, EdgeOp, DenseOp, false>), grid, dim3(256), 0, st, a,
                       b, ep, (int)E, (int)C, (int)K);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Factorised FIRST edge Linear for the training forward:  H1[q] = U[dst_q] + V[src_q] + W1c.attr_q + b1
// (UV = x.[W1a-W1b | W1b]^T computed once per node by a dense GEMM), plus the BatchNorm partial statistics in the
// GEMM epilogue's format (float2 (sum, M2 about the group mean) per 32-row group and column).  Replaces the
// gathered K = 2 Cin + 4 GEMM when E >> N: at E = 1.2 M / N = 200 k that GEMM ran at 17 TFLOP/s (1.19 ms) because
// its A operand is two random 256-B row gathers per edge.  One workgroup = 64 edges: thread (row rb + 16 t,
// columns 4q..) writes its 16 bytes of H1 and parks them in LDS; 128 threads then reduce the two 32-row groups.
// ------------------------------------------------------------------------------------------------
template <class TO>
__global__ void __launch_bounds__(256) k_edge_uv_lin1(const float* __restrict__ UV, long ld_uv,
                                                      const int* __restrict__ src, const int* __restrict__ dst,
                                                      const float* __restrict__ attr, int E,
                                                      const float* __restrict__ Wc4, const float* __restrict__ b1,
                                                      TO* __restrict__ H1, long ldh, float2* __restrict__ stats) {
  constexpr int LDT = 65;
  __shared__ float T[64 * LDT];
  const int tid = threadIdx.x, q = tid & 15, rb = tid >> 4;
  const int row0 = blockIdx.x * 64;
  float4 wc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wc[j] = *reinterpret_cast<const float4*>(Wc4 + (4 * q + j) * 4);
  float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b1) bb = *reinterpret_cast<const float4*>(b1 + 4 * q);
  int di[4], si[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = yl_min(row0 + rb + 16 * t, E - 1);
    di[t] = dst[e]; si[t] = src[e];
  }
  float4 u[4], v[4], a[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = yl_min(row0 + rb + 16 * t, E - 1);
    u[t] = *reinterpret_cast<const float4*>(UV + (long)di[t] * ld_uv + 4 * q);
    v[t] = *reinterpret_cast<const float4*>(UV + (long)si[t] * ld_uv + 64 + 4 * q);
    a[t] = *reinterpret_cast<const float4*>(attr + (long)e * 4);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    auto one = [&](float uu, float vv, const float4& w, float b) {
      float z = uu + vv;
      z = fmaf(a[t].x, w.x, z); z = fmaf(a[t].y, w.y, z); z = fmaf(a[t].z, w.z, z); z = fmaf(a[t].w, w.w, z);
      return z + b;
    };
    const float4 h = make_float4(one(u[t].x, v[t].x, wc[0], bb.x), one(u[t].y, v[t].y, wc[1], bb.y),
                                 one(u[t].z, v[t].z, wc[2], bb.z), one(u[t].w, v[t].w, wc[3], bb.w));
    const int r = rb + 16 * t;
    if (row0 + r < E) yl_st4(H1 + (long)(row0 + r) * ldh + 4 * q, h);
    float* tr = T + r * LDT + 4 * q;
    tr[0] = h.x; tr[1] = h.y; tr[2] = h.z; tr[3] = h.w;
  }
  if (stats == nullptr) return;
  __syncthreads();
  if (tid < 128) {
    const int c = tid & 63, grp = tid >> 6;
    const int base = row0 + 32 * grp;
    int cnt = E - base;
    cnt = cnt > 32 ? 32 : cnt;
    if (cnt == 32) {
      // full group: the 32 values in registers (reads in flight together; the rolled loops below were 2 x 32 dependent
      // LDS round trips per workgroup), same order of additions
      float v[32];
#pragma unroll
      for (int r = 0; r < 32; ++r) v[r] = T[(32 * grp + r) * LDT + c];
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 32; ++r) sum += v[r];
      const float mu = sum / 32.f;
      float m2 = 0.f;
#pragma unroll
      for (int r = 0; r < 32; ++r) { const float d = v[r] - mu; m2 += d * d; }
      stats[(long)(base >> 5) * 64 + c] = make_float2(sum, m2);
    } else if (cnt > 0) {
      float sum = 0.f;
      for (int r = 0; r < cnt; ++r) sum += T[(32 * grp + r) * LDT + c];
      const float mu = sum / (float)cnt;
      float m2 = 0.f;
      for (int r = 0; r < cnt; ++r) { const float d = T[(32 * grp + r) * LDT + c] - mu; m2 += d * d; }
      stats[(long)(base >> 5) * 64 + c] = make_float2(sum, m2);
    }
  }
}

// T = float, or yl_bf16_t: H1 stored as bfloat16 (round-to-nearest-even); the BatchNorm partial statistics are those of
// the fp32 values before rounding.
template <class T>
static int edge_uv_lin1_fwd_impl(const float* UV, int64_t ld_uv, const int32_t* src_csr, const int32_t* dst_csr,
                                 const float* attr_csr, int64_t E, const float* Wc4, const float* b1, int64_t C, T* H1,
                                 int64_t ldh, float* stats, yolat_stream_t stream) {
  if (E < 0 || !UV || !Wc4) return YOLAT_E_INVALID;
  if (C != 64) return YOLAT_E_UNSUPPORTED;
  if (E == 0) return 0;
  if (!src_csr || !dst_csr || !attr_csr || !H1 || E >= (1LL << 31) || ldh < C || ld_uv < 2 * C) return YOLAT_E_INVALID;
  if (ld_uv % 4 != 0 || ldh % 4 != 0 || !yl_aligned16(UV) || !yl_aligned16(attr_csr) || !yl_aligned16(Wc4) ||
      !yl_row_aligned<T>(H1) || (b1 && !yl_aligned16(b1)) || (stats && (((uintptr_t)stats) & 7) != 0))
    return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_edge_uv_lin1<T>, dim3(yl_cdiv(E, 64)), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv, src_csr,
                     dst_csr, attr_csr, (int)E, Wc4, b1, H1, (long)ldh, reinterpret_cast<float2*>(stats));
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_edge_uv_lin1_fwd(const float* UV, int64_t ld_uv, const int32_t* src_csr, const int32_t* dst_csr,
                                      const float* attr_csr, int64_t E, const float* Wc4, const float* b1, int64_t C,
                                      float* H1, int64_t ldh, float* stats, yolat_stream_t stream) {
  return edge_uv_lin1_fwd_impl<float>(UV, ld_uv, src_csr, dst_csr, attr_csr, E, Wc4, b1, C, H1, ldh, stats, stream);
}

extern "C" int yolat_edge_uv_lin1_fwd_h(const float* UV, int64_t ld_uv, const int32_t* src_csr, const int32_t* dst_csr,
                                        const float* attr_csr, int64_t E, const float* Wc4, const float* b1, int64_t C,
                                        uint16_t* H1, int64_t ldh, float* stats, yolat_stream_t stream) {
  return edge_uv_lin1_fwd_impl<yl_bf16_t>(UV, ld_uv, src_csr, dst_csr, attr_csr, E, Wc4, b1, C, H1, ldh, stats, stream);
}

extern "C" int yolat_edge_lin1_bwd_w(const float* dH1, int64_t lddh, int64_t E, int64_t C,
                                     const float* x, int64_t ldx, int64_t N, int64_t Cin,
                                     const int32_t* src_csr, const int32_t* dst_csr,
                                     const float* attr_csr, float* dW1, int64_t lddw, float* db1,
                                     int accumulate, float* partial, yolat_stream_t stream) {
  if (E < 0 || N <= 0 || Cin <= 0 || C <= 0 || !x || !dW1 || !partial) return YOLAT_E_INVALID;
  if (E > 0 && (!dH1 || !src_csr || !dst_csr || !attr_csr)) return YOLAT_E_INVALID;
  const long K = 2 * Cin + 4;
  if (lddw < K || lddh < C || E >= (1LL << 31)) return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  TnPlan p = yl_tn_plan(E, C, K);
  DenseOp y = yl_dense(dH1, lddh, E, C);
  EdgeOp a = yl_edge(x, ldx, Cin, src_csr, dst_csr, attr_csr, E);
  float* dbpart = db1 ? partial + (size_t)p.S * C * K : nullptr;
  dim3 grid(yl_cdiv(C, 64), yl_cdiv(K, 64), p.S);
  hipLaunchKernelGGL((k_gemm_tn<DenseOp, EdgeOp>), grid, dim3(256), 0, st, y, a, partial, dbpart,
                     (int)E, (int)C, (int)K, p.rows_per_split);
  YL_LAUNCH_CHECK();
  const long elems = C * K;
  yl_reduce_dw_db(st, partial, elems, p.S, dW1, (long)lddw, (int)K, dbpart, db1, (long)C, accumulate);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_edge_lin1_bwd_x(const float* dH1, int64_t lddh, int64_t E, int64_t C,
                                     const float* W1, int64_t ldw, int64_t Cin, float* dG,
                                     int64_t lddg, yolat_stream_t stream) {
  if (E < 0 || C <= 0 || Cin <= 0 || !W1) return YOLAT_E_INVALID;
  if (E == 0) return 0;
  if (!dH1 || !dG || lddh < C || lddg < 2 * Cin || ldw < 2 * Cin + 4 || E >= (1LL << 31))
    return YOLAT_E_INVALID;
  DenseOp a = yl_dense(dH1, lddh, E, C);
  EdgeWcOp b;
  b.W1 = W1; b.ldw = ldw; b.Cin = (int)Cin; b.C = (int)C; b.vec = 1;
  Epilogue ep;
  ep.bias = nullptr; ep.scale = nullptr; ep.shift = nullptr; ep.relu = 0;
  ep.Y = dG; ep.ldy = lddg; ep.accumulate = 0; ep.stats = nullptr; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  const long Nn = 2 * Cin;
  dim3 grid(yl_cdiv(E, 64), yl_cdiv(Nn, 64));
  hipLaunchKernelGGL((k_gemm_nt<64, 64, 32, DenseOp, EdgeWcOp, true>), grid, dim3(256), 0,
                     (hipStream_t)stream, a, b, ep, (int)E, (int)Nn, (int)C);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// CSR mean aggregation.  One wave per destination node, lanes across channels (256-B rows are
// read fully coalesced); rows of a node are consecutive CSR slots, summed in ascending edge order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_csr_mean_fwd(const float* H, long ldh, int C,
                                                      const float* hs, const float* hb, int relu,
                                                      const int* row_ptr, int N, float* out,
                                                      long ldo, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int q0 = row_ptr[n], q1 = row_ptr[n + 1];
  const float inv = 1.f / (float)((q1 - q0) > 1 ? (q1 - q0) : 1);
  for (int c = lane; c < C; c += 64) {
    const float sc = hs ? hs[c] : 1.f, sh = hs ? hb[c] : 0.f;
    const float floor = relu ? 0.f : -INFINITY;
    float s = 0.f;
    int q = q0;
    for (; q + 4 <= q1; q += 4) {      // 4 independent row loads in flight; summation stays in edge order
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = H[(long)(q + j) * ldh + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) s += fmaxf(fmaf(v[j], sc, sh), floor);
    }
    for (; q < q1; ++q) s += fmaxf(fmaf(H[(long)q * ldh + c], sc, sh), floor);
    s = yl_mul_rn(s, inv);
    float* o = out + (long)n * ldo + c;
    if (accumulate) s += *o;
    *o = s;
  }
}

// C == 4*LPN, 16-byte aligned rows: LPN lanes own one node (one float4 of columns each), 64/LPN nodes per
// wave, up to 8 rows (8 x 16 B per lane) in flight per lane.  Per-column summation order is unchanged
// (ascending CSR slot), so results are bit-identical to the scalar kernel above.
template <int LPN, class T = float>
__global__ void __launch_bounds__(256) k_csr_mean_fwd_v4(const T* __restrict__ H, long ldh,
                                                         const float* hs, const float* hb, int relu,
                                                         const int* __restrict__ row_ptr, int N,
                                                         float* out, long ldo, int accumulate) {
  const int sub = threadIdx.x % LPN;
  const int n = blockIdx.x * (256 / LPN) + threadIdx.x / LPN;
  if (n >= N) return;
  const int q0 = row_ptr[n], q1 = row_ptr[n + 1];
  const float inv = 1.f / (float)((q1 - q0) > 1 ? (q1 - q0) : 1);
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (hs) {
    sc = *reinterpret_cast<const float4*>(hs + 4 * sub);
    sh = *reinterpret_cast<const float4*>(hb + 4 * sub);
  }
  const float floor = relu ? 0.f : -INFINITY;
  const T* hp = H + 4 * sub;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add = [&](const float4& v) {
    s.x += fmaxf(fmaf(v.x, sc.x, sh.x), floor);
    s.y += fmaxf(fmaf(v.y, sc.y, sh.y), floor);
    s.z += fmaxf(fmaf(v.z, sc.z, sh.z), floor);
    s.w += fmaxf(fmaf(v.w, sc.w, sh.w), floor);
  };
  int q = q0;
  for (; q + 8 <= q1; q += 8) {
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = yl_ld4(hp + (long)(q + j) * ldh);
#pragma unroll
    for (int j = 0; j < 8; ++j) add(v[j]);
  }
  if (q < q1) {   // 1..7 remaining rows: clamped (re-read) addresses keep the loads unconditional
    float4 v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = yl_ld4(hp + (long)yl_min(q + j, q1 - 1) * ldh);
#pragma unroll
    for (int j = 0; j < 7; ++j)
      if (q + j < q1) add(v[j]);
  }
  s.x = yl_mul_rn(s.x, inv); s.y = yl_mul_rn(s.y, inv); s.z = yl_mul_rn(s.z, inv); s.w = yl_mul_rn(s.w, inv);
  float4* o = reinterpret_cast<float4*>(out + (long)n * ldo + 4 * sub);
  if (accumulate) {
    const float4 p = *o;
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  *o = s;
}

// T = float: any C and any row layout (the scalar kernel where the rows are not 64 aligned columns); H may be null and
// ldh is not checked (a graph without edges reads no row).  T = yl_bf16_t (training with bf16 storage): C = 64 and
// 8-byte aligned rows only.
template <class T>
static int csr_mean_fwd_impl(const T* H, int64_t ldh, int64_t C, const float* h_scale, const float* h_shift, int h_relu,
                             const int32_t* row_ptr, int64_t N, float* out, int64_t ldo, int accumulate,
                             yolat_stream_t stream) {
  constexpr bool f32 = std::is_same<T, float>::value;
  if (N <= 0 || !row_ptr || !out || ldo < C) return YOLAT_E_INVALID;
  if constexpr (f32) {              // twins differ: fp32 rejects C <= 0 here; bf16 rejects a null H and ldh < C
    if (C <= 0) return YOLAT_E_INVALID;
  } else {
    if (!H || ldh < C) return YOLAT_E_INVALID;
  }
  if ((h_scale == nullptr) != (h_shift == nullptr)) return YOLAT_E_INVALID;
  if (C == 64 && ldh % 4 == 0 && ldo % 4 == 0 && yl_row_aligned<T>(H) && yl_aligned16(out) &&
      (!h_scale || (yl_aligned16(h_scale) && yl_aligned16(h_shift)))) {
    hipLaunchKernelGGL((k_csr_mean_fwd_v4<16, T>), dim3(yl_cdiv(N, 16)), dim3(256), 0, (hipStream_t)stream, H, (long)ldh,
                       h_scale, h_shift, h_relu, row_ptr, (int)N, out, (long)ldo, accumulate);
    YL_LAUNCH_CHECK();
    return 0;
  }
  if constexpr (f32) {              // twins differ: only fp32 has the scalar kernel for the other layouts
    hipLaunchKernelGGL(k_csr_mean_fwd, dim3(yl_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, H, (long)ldh, (int)C, h_scale,
                       h_shift, h_relu, row_ptr, (int)N, out, (long)ldo, accumulate);
    YL_LAUNCH_CHECK();
    return 0;
  } else {
    return YOLAT_E_UNSUPPORTED;
  }
}

extern "C" int yolat_csr_mean_fwd(const float* H, int64_t ldh, int64_t C, const float* h_scale,
                                  const float* h_shift, int h_relu, const int32_t* row_ptr,
                                  int64_t N, float* out, int64_t ldo, int accumulate,
                                  yolat_stream_t stream) {
  return csr_mean_fwd_impl<float>(H, ldh, C, h_scale, h_shift, h_relu, row_ptr, N, out, ldo, accumulate, stream);
}

extern "C" int yolat_csr_mean_fwd_h(const uint16_t* H, int64_t ldh, int64_t C, const float* h_scale,
                                    const float* h_shift, int h_relu, const int32_t* row_ptr, int64_t N, float* out,
                                    int64_t ldo, int accumulate, yolat_stream_t stream) {
  return csr_mean_fwd_impl<yl_bf16_t>(H, ldh, C, h_scale, h_shift, h_relu, row_ptr, N, out, ldo, accumulate, stream);
}

__global__ void __launch_bounds__(256) k_csr_mean_bwd(const float* dOut, long lddo, int C,
                                                      const int* row_ptr, const int* dst, int E,
                                                      float* dM, long lddm) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= E) return;
  const int n = dst[q];
  const int deg = row_ptr[n + 1] - row_ptr[n];
  const float inv = 1.f / (float)(deg > 1 ? deg : 1);
  for (int c = lane; c < C; c += 64) dM[(long)q * lddm + c] = dOut[(long)n * lddo + c] * inv;
}

// C == 64, aligned rows: 16 lanes x float4 per edge, a wave writes 4 rows (1 KiB) per store instead of 256 B
template <class T>
__global__ void __launch_bounds__(256) k_csr_mean_bwd_v4(const float* __restrict__ dOut, long lddo,
                                                         const int* __restrict__ row_ptr, const int* __restrict__ dst,
                                                         int E, T* __restrict__ dM, long lddm) {
  const int l16 = threadIdx.x & 15;
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (q >= E) return;
  const int n = dst[q];
  const int deg = row_ptr[n + 1] - row_ptr[n];
  const float inv = 1.f / (float)(deg > 1 ? deg : 1);
  const float4 g = *reinterpret_cast<const float4*>(dOut + (long)n * lddo + 4 * l16);
  yl_st4(dM + (long)q * lddm + 4 * l16, make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv));
}

// T = float: any C and any row layout (scalar kernel); T = yl_bf16_t (dM stored as bfloat16): C = 64, aligned rows only.
template <class T>
static int csr_mean_bwd_impl(const float* dOut, int64_t lddo, int64_t C, const int32_t* row_ptr, const int32_t* dst_csr,
                             int64_t E, T* dM, int64_t lddm, yolat_stream_t stream) {
  constexpr bool f32 = std::is_same<T, float>::value;
  if (E < 0 || !dOut || !row_ptr) return YOLAT_E_INVALID;
  if constexpr (f32) {              // twins differ: only fp32 rejects C <= 0 as invalid (bf16: unsupported, below)
    if (C <= 0) return YOLAT_E_INVALID;
  }
  if (E == 0) return 0;
  if (!dst_csr || !dM || lddm < C) return YOLAT_E_INVALID;
  if (C == 64 && lddo % 4 == 0 && lddm % 4 == 0 && yl_aligned16(dOut) && yl_row_aligned<T>(dM)) {
    hipLaunchKernelGGL(k_csr_mean_bwd_v4<T>, dim3(yl_cdiv(E, 16)), dim3(256), 0, (hipStream_t)stream, dOut, (long)lddo,
                       row_ptr, dst_csr, (int)E, dM, (long)lddm);
  } else if constexpr (f32) {       // twins differ: only fp32 has the scalar kernel for the other layouts
    hipLaunchKernelGGL(k_csr_mean_bwd, dim3(yl_cdiv(E, 4)), dim3(256), 0, (hipStream_t)stream, dOut, (long)lddo, (int)C,
                       row_ptr, dst_csr, (int)E, dM, (long)lddm);
  } else {
    return YOLAT_E_UNSUPPORTED;
  }
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_csr_mean_bwd(const float* dOut, int64_t lddo, int64_t C,
                                  const int32_t* row_ptr, const int32_t* dst_csr, int64_t E,
                                  float* dM, int64_t lddm, yolat_stream_t stream) {
  return csr_mean_bwd_impl<float>(dOut, lddo, C, row_ptr, dst_csr, E, dM, lddm, stream);
}

extern "C" int yolat_csr_mean_bwd_h(const float* dOut, int64_t lddo, int64_t C, const int32_t* row_ptr,
                                    const int32_t* dst_csr, int64_t E, uint16_t* dM, int64_t lddm,
                                    yolat_stream_t stream) {
  return csr_mean_bwd_impl<yl_bf16_t>(dOut, lddo, C, row_ptr, dst_csr, E, dM, lddm, stream);
}

// ------------------------------------------------------------------------------------------------
// Backward of the two gathers: dX[n] (+)= sum_{q in CSR row n} dG[q, 0:Cin]
//                                       + sum_{q in CSC col n} dG[q, Cin:2Cin]   (ascending slots)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_edge_scatter_bwd(const float* dG, long lddg, int Cin,
                                                          const int* row_ptr, const int* col_ptr,
                                                          const int* slots, int N, float* dX,
                                                          long lddx, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int q0 = row_ptr[n], q1 = row_ptr[n + 1];
  const int t0 = col_ptr[n], t1 = col_ptr[n + 1];
  for (int c = lane; c < Cin; c += 64) {
    float s = 0.f;
    for (int q = q0; q < q1; ++q) s += dG[(long)q * lddg + c];
    for (int t = t0; t < t1; ++t) s += dG[(long)slots[t] * lddg + Cin + c];
    float* o = dX + (long)n * lddx + c;
    if (accumulate) s += *o;
    *o = s;
  }
}

// Cin == 64, aligned rows: 16 lanes x float4 per node (a wave covers 4 nodes), 4 row loads in flight per thread;
// same summation order as the scalar kernel (CSR slots ascending, then CSC slots ascending)
__global__ void __launch_bounds__(256) k_edge_scatter_bwd_v4(const float* __restrict__ dG, long lddg,
                                                             const int* __restrict__ row_ptr,
                                                             const int* __restrict__ col_ptr,
                                                             const int* __restrict__ slots, int N, float* dX,
                                                             long lddx, int accumulate) {
  const int l16 = threadIdx.x & 15;
  const int n = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (n >= N) return;
  const int q0 = row_ptr[n], q1 = row_ptr[n + 1];
  const int t0 = col_ptr[n], t1 = col_ptr[n + 1];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* gd = dG + 4 * l16;
  for (int q = q0; q < q1; q += 4) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(gd + (long)yl_min(q + k, q1 - 1) * lddg);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (q + k < q1) { s.x += v[k].x; s.y += v[k].y; s.z += v[k].z; s.w += v[k].w; }
  }
  const float* gs = dG + 64 + 4 * l16;
  for (int t = t0; t < t1; t += 4) {
    int sl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sl[k] = slots[yl_min(t + k, t1 - 1)];
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(gs + (long)sl[k] * lddg);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t + k < t1) { s.x += v[k].x; s.y += v[k].y; s.z += v[k].z; s.w += v[k].w; }
  }
  float4* o = reinterpret_cast<float4*>(dX + (long)n * lddx + 4 * l16);
  if (accumulate) { const float4 d = *o; s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w; }
  *o = s;
}

// ------------------------------------------------------------------------------------------------
// Backward of the FACTORISED first edge Linear (training, E >> N).  Forward:  H1[q] = U[dst_q] + V[src_q] + W1c.attr_q + b1
// with UV = x.[W1a - W1b | W1b]^T, so the gradients w.r.t. the per-node products are two per-node sums of dH1 rows,
//   dU[n] = sum_{q in CSR row n} dH1[q]   (contiguous rows)      dV[n] = sum_{t in CSC col n} dH1[slots[t]]   (gathered)
// and everything else is N-row dense algebra (dWuv = dUV^T.x, dx += dUV.Wuv) plus dW1c = dH1^T.attr, db1 = colsum(dH1).
// Replaces the gathered K = 2Cin+4 TN GEMM (dW1), the E x 64 -> E x 2Cin NT GEMM (dG) and the gather-scatter of dG:
// at cfg 5 (E = 1.2 M, N = 200 k) 595 + 347 + 145 us per block layer.  One 16-lane group per node, one float4 of
// columns per lane, 8 rows in flight; ascending slot order -> deterministic.  C = 64.
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_edge_uv_sums(const T* __restrict__ dH, long ldh,
                                                      const int* __restrict__ row_ptr, const int* __restrict__ col_ptr,
                                                      const int* __restrict__ slots, int N, float* __restrict__ dUV,
                                                      long ldo, int with_u) {
  const int sub = threadIdx.x & 15;
  const int n = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (n >= N) return;
  const T* hp = dH + 4 * sub;
  auto acc = [](float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; };
  // ---- dU: the node's own CSR rows (with_u == 0: written by yolat_bn_apply_edge_sums)
  int q0 = 0, q1 = 0;
  if (with_u) { q0 = row_ptr[n]; q1 = row_ptr[n + 1]; }
  float4 su = make_float4(0.f, 0.f, 0.f, 0.f);
  int q = q0;
  for (; q + 8 <= q1; q += 8) {
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = yl_ld4(hp + (long)(q + j) * ldh);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc(su, v[j]);
  }
  if (q < q1) {
    float4 v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = yl_ld4(hp + (long)yl_min(q + j, q1 - 1) * ldh);
#pragma unroll
    for (int j = 0; j < 7; ++j)
      if (q + j < q1) acc(su, v[j]);
  }
  // ---- dV: rows of the edges that leave this node (CSC by source; slot list ascending)
  const int t0 = col_ptr[n], t1 = col_ptr[n + 1];
  float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = t0; t < t1; t += 8) {
    int sl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sl[j] = slots[yl_min(t + j, t1 - 1)];
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = yl_ld4(hp + (long)sl[j] * ldh);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (t + j < t1) acc(sv, v[j]);
  }
  float* o = dUV + (long)n * ldo + 4 * sub;
  if (with_u) *reinterpret_cast<float4*>(o) = su;
  *reinterpret_cast<float4*>(o + 64) = sv;
}

// with_u = 1: both halves of dUV, from the CSR rows (row_ptr) and the CSC columns.  with_u = 0 (yolat_edge_uv_sums_v): the
// dV half alone, row_ptr unused — the kernel is handed col_ptr in its place and never reads it.
template <class T>
static int edge_uv_sums_impl(const T* dH1, int64_t ldh, const int32_t* row_ptr, const int32_t* col_ptr, const int32_t* slots,
                             int64_t N, int64_t C, float* dUV, int64_t ld_uv, int with_u, yolat_stream_t stream) {
  if (N <= 0 || !dH1 || (with_u && !row_ptr) || !col_ptr || !slots || !dUV || ldh < C || ld_uv < 2 * C)
    return YOLAT_E_INVALID;
  if (C != 64 || ldh % 4 != 0 || ld_uv % 4 != 0 || !yl_row_aligned<T>(dH1) || !yl_aligned16(dUV)) return YOLAT_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_edge_uv_sums<T>, dim3(yl_cdiv(N, 16)), dim3(256), 0, (hipStream_t)stream, dH1, (long)ldh,
                     with_u ? row_ptr : col_ptr, col_ptr, slots, (int)N, dUV, (long)ld_uv, with_u);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_edge_uv_sums(const float* dH1, int64_t ldh, const int32_t* row_ptr, const int32_t* col_ptr,
                                  const int32_t* slots, int64_t N, int64_t C, float* dUV, int64_t ld_uv,
                                  yolat_stream_t stream) {
  return edge_uv_sums_impl<float>(dH1, ldh, row_ptr, col_ptr, slots, N, C, dUV, ld_uv, 1, stream);
}

extern "C" int yolat_edge_uv_sums_h(const uint16_t* dH1, int64_t ldh, const int32_t* row_ptr, const int32_t* col_ptr,
                                    const int32_t* slots, int64_t N, int64_t C, float* dUV, int64_t ld_uv,
                                    yolat_stream_t stream) {
  return edge_uv_sums_impl<yl_bf16_t>(dH1, ldh, row_ptr, col_ptr, slots, N, C, dUV, ld_uv, 1, stream);
}

// The dV half alone (dUV columns [64, 128): sums over the CSC column of every node, gathered by slot), for callers that
// got the dU half from yolat_bn_apply_edge_sums.  dH1 fp32 (half = 0) or bfloat16.
extern "C" int yolat_edge_uv_sums_v(const void* dH1, int64_t ldh, int half, const int32_t* col_ptr, const int32_t* slots,
                                    int64_t N, int64_t C, float* dUV, int64_t ld_uv, yolat_stream_t stream) {
  if (half)
    return edge_uv_sums_impl<yl_bf16_t>(reinterpret_cast<const yl_bf16_t*>(dH1), ldh, nullptr, col_ptr, slots, N, C, dUV,
                                        ld_uv, 0, stream);
  return edge_uv_sums_impl<float>(reinterpret_cast<const float*>(dH1), ldh, nullptr, col_ptr, slots, N, C, dUV, ld_uv, 0,
                                  stream);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the attr columns of the factorised first edge Linear + its bias gradient (training backward,
// torch_vertex.py:331 nn.0 restricted to the 4 edge-attribute inputs):
//   dWc4[c][j] = sum_e dH1[e][c] * attr[e][j]      (64 x 4)        db1[c] = sum_e dH1[e][c]
// A pure streaming reduction over the [E, 64] gradient (307 MB fp32 / 154 MB bf16 at E = 1.2 M).  It used to run on the
// general TN GEMM (k_gemm_tn split-row: 64 x 64 tiles for a [64 x 4] result): 279 us fp32 / 319 us bf16 per call = 0.15 /
// 0.13 of HBM, 14 - 18 % of the cfg-5 train step.  Here: one pass, 16 bytes (fp32) / 8 bytes (bf16) per
// lane, a 16-lane group per row (the row's attr quad is one broadcast 16-byte load), 64 rows per workgroup and step with
// all loads of the step in flight, 16 + 4 register accumulators per lane; the 16 row groups of a workgroup are summed
// through LDS in fixed order, the workgroups' partials by a second small launch in fixed order: deterministic.
// ------------------------------------------------------------------------------------------------
constexpr int ADW_WG_MAX = 2048;
template <class T>
__global__ void __launch_bounds__(256) k_attr_dw(const T* __restrict__ dH, long ldh, const float4* __restrict__ attr, int E,
                                                 int rows_wg, float* __restrict__ part) {
  __shared__ float red[16][16 * 20 + 4];
  const int tid = threadIdx.x, sub = tid & 15, rg = tid >> 4;
  const int b0 = blockIdx.x * rows_wg, b1 = yl_min(b0 + rows_wg, E);
  float w[4][4], sb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sb[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[c][j] = 0.f;
  }
  const T* hp = dH + 4 * sub;
  for (int r0 = b0; r0 < b1; r0 += 64) {
    float4 h[4], a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = yl_min(r0 + 16 * t + rg, E - 1);
      h[t] = yl_ld4(hp + (long)r * ldh);
      a[t] = attr[r];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (r0 + 16 * t + rg < b1) {
        const float hv[4] = {h[t].x, h[t].y, h[t].z, h[t].w}, av[4] = {a[t].x, a[t].y, a[t].z, a[t].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sb[c] += hv[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) w[c][j] = fmaf(hv[c], av[j], w[c][j]);
        }
      }
    }
  }
  // this lane's 20 sums: columns 4 sub + c -> [c][j] at (4 sub + c) * 4 + j, bias at 256 + 4 sub + c
  float* mine = red[rg];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) mine[(4 * sub + c) * 4 + j] = w[c][j];
    mine[256 + 4 * sub + c] = sb[c];
  }
  __syncthreads();
  for (int i = tid; i < 320; i += 256) {
    float s = red[0][i];
#pragma unroll
    for (int g2 = 1; g2 < 16; ++g2) s += red[g2][i];
    part[(long)blockIdx.x * 320 + i] = s;
  }
}
// Sum of the workgroups' partials: ONE 256-thread workgroup per output (320 of them), thread t takes partial rows t, t + 256,
// ... (eight loads in flight), the 256 thread sums meet in a fixed tree (shuffles inside a wave, then the four wave sums
// in order) -> deterministic.  (32 lanes per output in 40 workgroups walked 64 partials per lane: 15 us per call for 2.6 MB,
// four calls per cfg-5 step; one workgroup walking all 2048 partials per output was 57 us.)
static __global__ void __launch_bounds__(256) k_attr_dw_reduce(const float* __restrict__ part, int nwg, float* __restrict__ dWc4,
                                                             float* __restrict__ db) {
  __shared__ float ws[4];
  const int o = blockIdx.x, t = threadIdx.x;                     // o < 320 by the launch
  float s = 0.f;
  for (int g0 = t; g0 < nwg; g0 += 8 * 256) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(long)yl_min(g0 + 256 * j, nwg - 1) * 320 + o];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (g0 + 256 * j < nwg) s += v[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if ((t & 63) == 0) ws[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    if (o < 256) dWc4[o] = s;
    else if (db != nullptr) db[o - 256] = s;
  }
}

extern "C" size_t yolat_edge_attr_dw_work_elems(int64_t E) { (void)E; return (size_t)ADW_WG_MAX * 320; }

extern "C" int yolat_edge_attr_dw(const void* dH1, int64_t ldh, int half, const float* attr_csr, int64_t E, int64_t C,
                                  float* dWc4, float* db1, float* work, yolat_stream_t stream) {
  if (E <= 0 || !dH1 || !attr_csr || !dWc4 || !work || ldh < C) return YOLAT_E_INVALID;
  if (C != 64 || ldh % 4 != 0 || !yl_aligned16(attr_csr) || E >= (1LL << 31) - 64 ||
      (((uintptr_t)dH1) & (half ? 7 : 15)) != 0)
    return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  long rows_wg = (yl_cdiv(E, ADW_WG_MAX) + 63) / 64 * 64;
  if (rows_wg < 256) rows_wg = 256;
  const int nwg = yl_cdiv(E, rows_wg);
  if (half)
    hipLaunchKernelGGL(k_attr_dw<yl_bf16_t>, dim3(nwg), dim3(256), 0, st, reinterpret_cast<const yl_bf16_t*>(dH1), (long)ldh,
                       reinterpret_cast<const float4*>(attr_csr), (int)E, (int)rows_wg, work);
  else
    hipLaunchKernelGGL(k_attr_dw<float>, dim3(nwg), dim3(256), 0, st, reinterpret_cast<const float*>(dH1), (long)ldh,
                       reinterpret_cast<const float4*>(attr_csr), (int)E, (int)rows_wg, work);
  YL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_attr_dw_reduce, dim3(320), dim3(256), 0, st, work, nwg, dWc4, db1);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm-1 backward apply + the CONTIGUOUS consumers of its result in one pass (round 4; training backward of the
// factorised conv layer, torch_vertex.py:331-332 nn.1/nn.2 backward feeding nn.0's):
//   dH1[q] = scale * (relu'(.) dA1[q] - c1 - xhat[q] c2)                        (k_bn_bwd_apply_v4's arithmetic, stored)
//   dU[n]  = sum_{q in CSR row n} dH1[q]                                        (k_edge_uv_sums' first half, ascending q)
//   dWc4   = dH1^T . attr,  db1 = column sums of dH1                            (k_attr_dw)
// dH1 used to be written by the apply pass and read three times (dU rows, dV gather, attr gradient): 921 + 614 + 307 MB
// per layer at E = 1.2 M.  Here the rows of a node are formed, stored (the dV gather of yolat_edge_uv_sums_v still
// needs them) and summed while they are in registers: 921 MB + the gather.  One 16-lane group per node (a float4 of
// columns per lane), 4 rows in flight, a workgroup owns a contiguous range of nodes = a contiguous range of rows;
// 16 + 4 attr accumulators per lane over all the nodes of the group, reduced like k_attr_dw (LDS in fixed order, then
// k_attr_dw_reduce over the workgroups): deterministic.  bf16 storage: the sums take the ROUNDED values, i.e. what the
// gather reads back.
// ------------------------------------------------------------------------------------------------
constexpr int BA_NODES_MAX = 1024;
__device__ __forceinline__ float ba_round(float v, float) { return v; }
__device__ __forceinline__ float ba_round(float v, yl_bf16_t) { return __uint_as_float((yl_pack_bf16(v, 0.f) & 0xffffu) << 16); }
__device__ __forceinline__ float ba_ld1(const float* p) { return *p; }
__device__ __forceinline__ float ba_ld1(const yl_bf16_t* p) { return __uint_as_float((unsigned)(*p) << 16); }
__device__ __forceinline__ void ba_st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void ba_st1(yl_bf16_t* p, float v) { *p = (yl_bf16_t)(__float_as_uint(v) >> 16); }   // v is rounded already
// Mapping: one WAVE per row, lane = column.  (The first version used a 16-lane group per node with a float4 of columns
// per lane, like k_edge_uv_sums: 16 attr accumulators + 24 constants + the rows in flight = 124 VGPRs = 4 waves per SIMD,
// and it ran at 184 us per call at E = 1.2 M against 144 for the apply pass alone.)  With the row wave-uniform the
// attr quad is a scalar load, a lane holds 4 + 1 accumulators and 6 constants, eight rows are in flight with 16
// registers, and the node boundaries are scalar branches.
template <class T>
__global__ void __launch_bounds__(256) k_bn_apply_edge_sums(const T* __restrict__ dZ, long lddz, const T* __restrict__ Y,
                                                            long ldy, T* dY, long lddy,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            int relu, const float* __restrict__ coef,
                                                            const int* __restrict__ row_ptr, const float4* __restrict__ attr,
                                                            int N, int nodes_wg, float* __restrict__ dU, long ldo,
                                                            float* __restrict__ part) {
  __shared__ float red[4][320];
  __shared__ int rp[BA_NODES_MAX + 1];
  const int tid = threadIdx.x, c = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float mu = mean[c], is = invstd[c], sc = scale[c], sh = shift[c], k1 = coef[c], k2 = coef[64 + c];
  auto one = [&](float y, float g) {
    if (relu && !(fmaf(y, sc, sh) > 0.f)) g = 0.f;
    // the product is a stored value: the sums below must add exactly what the gather reads back — the empty asm keeps
    // the compiler from contracting "sum + a * (...)" into an fma of its factors
    float p = sc * (g - k1 - ((y - mu) * is) * k2);
    asm volatile("" : "+v"(p));
    return ba_round(p, T());
  };
  float w[4] = {0.f, 0.f, 0.f, 0.f}, sb = 0.f;
  // The workgroup's nodes [n0, n1) are dealt to its 4 waves as 4 contiguous node ranges of (nearly) equal ROW counts:
  // wave k owns the nodes whose first row lies in the k-th quarter of the workgroup's row range (the last wave also the
  // trailing nodes without rows).  A function of the graph alone, so the order of every sum is fixed.
  const int n0 = blockIdx.x * nodes_wg, n1 = yl_min(n0 + nodes_wg, N);
  const int cnt = n1 - n0;                                  // <= BA_NODES_MAX by the launch
  for (int i = tid; i <= cnt; i += 256) rp[i] = row_ptr[n0 + i];
  __syncthreads();
  const long Q0 = rp[0], QR = (long)rp[cnt] - Q0;
  auto first_at_or_after = [&](long v) {                    // lowest i in [0, cnt] with rp[i] >= v
    int lo = 0, hi = cnt;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rp[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  int i = __builtin_amdgcn_readfirstlane(first_at_or_after(Q0 + QR * wave / 4));
  const int iend = wave == 3 ? cnt : __builtin_amdgcn_readfirstlane(first_at_or_after(Q0 + QR * (wave + 1) / 4));
  // the wave's nodes [i, iend) own the contiguous rows [rp[i], rp[iend]): streamed eight at a time whatever the node
  // boundaries are; a row that starts a new node first flushes the finished nodes' sums (nodes without rows: zeros)
  if (i < iend) {
    const int qa = __builtin_amdgcn_readfirstlane(rp[i]), qb = __builtin_amdgcn_readfirstlane(rp[iend]);
    int qn = __builtin_amdgcn_readfirstlane(rp[i + 1]);     // first row that is NOT node i's
    float su = 0.f;
    for (int q = qa; q < qb; q += 8) {
      float y[8], g[8];
      float4 av[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const long r = yl_min(q + k, qb - 1);               // wave-uniform
        y[k] = ba_ld1(Y + r * ldy + c);
        g[k] = ba_ld1(dZ + r * lddz + c);
        av[k] = attr[r];                                    // scalar load
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (q + k < qb) {
          while (q + k >= qn) {
            dU[(long)(n0 + i) * ldo + c] = su;
            su = 0.f;
            ++i;
            qn = __builtin_amdgcn_readfirstlane(rp[i + 1]);
          }
          const float hv = one(y[k], g[k]);
          ba_st1(dY + (long)(q + k) * lddy + c, hv);
          su += hv;
          sb += hv;
          w[0] = fmaf(hv, av[k].x, w[0]); w[1] = fmaf(hv, av[k].y, w[1]);
          w[2] = fmaf(hv, av[k].z, w[2]); w[3] = fmaf(hv, av[k].w, w[3]);
        }
      }
    }
    for (; i < iend; ++i) {                                 // the last node with rows + trailing nodes without
      dU[(long)(n0 + i) * ldo + c] = su;
      su = 0.f;
    }
  }
  float* mine = red[wave];
#pragma unroll
  for (int j = 0; j < 4; ++j) mine[c * 4 + j] = w[j];
  mine[256 + c] = sb;
  __syncthreads();
  for (int e = tid; e < 320; e += 256) part[(long)blockIdx.x * 320 + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

static long ba_nodes_wg(int64_t N) {
  // ~ADW_WG_MAX workgroups: 124 VGPRs = 4 workgroups per CU = 1024 resident on 256 CUs, so 2048 is two full rounds (the
  // first version rounded the node count up to a multiple of 16: 1786 workgroups at cfg 5 = 1.74 rounds)
  long nodes_wg = yl_cdiv(N, ADW_WG_MAX);
  if (nodes_wg < 16) nodes_wg = 16;
  if (nodes_wg > BA_NODES_MAX) nodes_wg = BA_NODES_MAX;      // N > 2 M nodes: more than ADW_WG_MAX workgroups
  return nodes_wg;
}
extern "C" size_t yolat_bn_apply_edge_sums_work_elems(int64_t N) {
  return (size_t)(N > 0 ? yl_cdiv(N, ba_nodes_wg(N)) : 1) * 320;
}

// dA1 / H1 / dH1 [E, 64] fp32 (half = 0) or bfloat16 (half != 0), rows in CSR order (dH1 may alias dA1); coef [128] =
// (c1 | c2) of the BatchNorm backward (yolat_bn_csr_l2_bwd's next_coef); dUV [N, ld_uv]: columns [0, 64) are written
// (the dV half: yolat_edge_uv_sums_v); dWc4 [64, 4], db1 [64] (nullable).  work: yolat_bn_apply_edge_sums_work_elems(N).
extern "C" int yolat_bn_apply_edge_sums(const void* dA1, int64_t ldda, const void* H1, int64_t ldh, void* dH1, int64_t lddh,
                                        int half, int64_t E, const float* save_mean, const float* save_invstd,
                                        const float* scale, const float* shift, int relu, const float* coef,
                                        const int32_t* row_ptr, const float* attr_csr, int64_t N, float* dUV, int64_t ld_uv,
                                        float* dWc4, float* db1, float* work, yolat_stream_t stream) {
  if (E <= 0 || N <= 0 || !dA1 || !H1 || !dH1 || !save_mean || !save_invstd || !scale || !shift || !coef || !row_ptr ||
      !attr_csr || !dUV || !dWc4 || !work || ldda < 64 || ldh < 64 || lddh < 64 || ld_uv < 64)
    return YOLAT_E_INVALID;
  const uintptr_t al = half ? 7 : 15;
  if (ldda % 4 != 0 || ldh % 4 != 0 || lddh % 4 != 0 || ld_uv % 4 != 0 || E >= (1LL << 31) - 64 || N >= (1LL << 31) - 64 ||
      (((uintptr_t)dA1 | (uintptr_t)H1 | (uintptr_t)dH1) & al) || !yl_aligned16(save_mean) || !yl_aligned16(save_invstd) ||
      !yl_aligned16(scale) || !yl_aligned16(shift) || !yl_aligned16(coef) || !yl_aligned16(attr_csr) || !yl_aligned16(dUV))
    return YOLAT_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long nodes_wg = ba_nodes_wg(N);
  const int nwg = yl_cdiv(N, nodes_wg);
  if (half)
    hipLaunchKernelGGL(k_bn_apply_edge_sums<yl_bf16_t>, dim3(nwg), dim3(256), 0, st, reinterpret_cast<const yl_bf16_t*>(dA1),
                       (long)ldda, reinterpret_cast<const yl_bf16_t*>(H1), (long)ldh, reinterpret_cast<yl_bf16_t*>(dH1),
                       (long)lddh, save_mean, save_invstd, scale, shift, relu, coef, row_ptr,
                       reinterpret_cast<const float4*>(attr_csr), (int)N, (int)nodes_wg, dUV, (long)ld_uv, work);
  else
    hipLaunchKernelGGL(k_bn_apply_edge_sums<float>, dim3(nwg), dim3(256), 0, st, reinterpret_cast<const float*>(dA1),
                       (long)ldda, reinterpret_cast<const float*>(H1), (long)ldh, reinterpret_cast<float*>(dH1), (long)lddh,
                       save_mean, save_invstd, scale, shift, relu, coef, row_ptr, reinterpret_cast<const float4*>(attr_csr),
                       (int)N, (int)nodes_wg, dUV, (long)ld_uv, work);
  YL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_attr_dw_reduce, dim3(320), dim3(256), 0, st, work, nwg, dWc4, db1);
  YL_LAUNCH_CHECK();
  return 0;
}

// dW1 [C, 2Cin+4] from the gradients of the split weights (inverse of yolat_conv_split_w1):
//   dW1[:, 0:Cin] = dWuv[0:C],  dW1[:, Cin:2Cin] = dWuv[C:2C] - dWuv[0:C],  dW1[:, 2Cin:] = dWc4
static __global__ void k_conv_merge_dw1(const float* __restrict__ dWuv, const float* __restrict__ dWc4, int Cin, int C,
                                        float* dW1, long ld, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C * Cin) {
    const int c = i / Cin, k = i % Cin;
    const float a = dWuv[(long)c * Cin + k], b = dWuv[(long)(C + c) * Cin + k] - a;
    float* row = dW1 + (long)c * ld;
    row[k] = accumulate ? row[k] + a : a;
    row[Cin + k] = accumulate ? row[Cin + k] + b : b;
  }
  if (i < C * 4) {
    float* d = dW1 + (long)(i / 4) * ld + 2 * Cin + (i % 4);
    *d = accumulate ? *d + dWc4[i] : dWc4[i];
  }
}

extern "C" int yolat_conv_merge_dw1(const float* dWuv, const float* dWc4, int64_t Cin, int64_t C, float* dW1,
                                    int64_t lddw, int accumulate, yolat_stream_t stream) {
  if (!dWuv || !dWc4 || !dW1 || Cin <= 0 || C <= 0 || lddw < 2 * Cin + 4) return YOLAT_E_INVALID;
  const long n = C * (Cin > 4 ? Cin : 4);
  hipLaunchKernelGGL(k_conv_merge_dw1, dim3(yl_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dWuv, dWc4, (int)Cin,
                     (int)C, dW1, (long)lddw, accumulate);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_edge_scatter_bwd(const float* dG, int64_t lddg, int64_t Cin,
                                      const int32_t* row_ptr, const int32_t* col_ptr,
                                      const int32_t* slots, int64_t N, float* dX, int64_t lddx,
                                      int accumulate, yolat_stream_t stream) {
  if (N <= 0 || Cin <= 0 || !row_ptr || !col_ptr || !dX || lddx < Cin) return YOLAT_E_INVALID;
  if (Cin == 64 && lddg % 4 == 0 && lddx % 4 == 0 && yl_aligned16(dG) && yl_aligned16(dX))
    hipLaunchKernelGGL(k_edge_scatter_bwd_v4, dim3(yl_cdiv(N, 16)), dim3(256), 0, (hipStream_t)stream, dG, (long)lddg,
                       row_ptr, col_ptr, slots, (int)N, dX, (long)lddx, accumulate);
  else
  hipLaunchKernelGGL(k_edge_scatter_bwd, dim3(yl_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream,
                     dG, (long)lddg, (int)Cin, row_ptr, col_ptr, slots, (int)N, dX, (long)lddx,
                     accumulate);
  YL_LAUNCH_CHECK();
  return 0;
}
