// edge.hip — the fused EVAL message passing of AttrRelativeEdgeConvGlobalPool2 (gcn_lib/sparse/torch_vertex.py:288-341)
// on gfx950: the two-layer edge MLP in one kernel (k_edge_mlp2, k_edge_uv_mlp2) and the factorised edge MLP fused with
// the CSR mean (k_edge_uv_mlp2_mean, its several-tiles-per-workgroup and wave-specialised forms), with their extern "C"
// entries.  All [E,*] tensors are in destination-sorted (CSR) order, so aggregation reads contiguous rows and needs no
// atomics.  The single-op edge kernels of training and of the eval fall-back (first edge Linear, CSR mean, scatter,
// per-node sums and their backward) live in edge_ops.hip.
#include "operands.hpp"
#include "epilogue.hpp"
#include "gemm_nt_two.hpp"   // not launched here: see the header
#include "internal.hpp"
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------
// Eval-mode edge MLP, both layers in one kernel (torch_vertex.py:311,331-335 `self.nn`, BN folded):
//   H2[q] = relu(s2*(W2 . relu(s1*(W1 . [x[dst] | x[src]-x[dst] | attr](q) + b1) + t1) + b2) + t2)
// One 64-edge tile per workgroup.  GEMM1 is the k_gemm_nt<64,64,*> loop on the gathered operand; its
// activated accumulators go to LDS (never to HBM: saves the E x 64 write + read and one launch), GEMM2
// reads them back as MFMA A-fragments with W2 staged in LDS during GEMM1.  Same k order and the same
// epilogue arithmetic as the two-kernel path -> bit-identical H2.
//   BLOCK = true : Cin % 32 == 0, vector loads; the 4 attr columns are a final 2-MFMA step instead of a
//                  mostly-zero 32-wide k-step (K = 132 costs 66 MFMAs per wave, not 80)
//   BLOCK = false: any Cin (the Cin = 5 head layer), 16-wide generic k-steps
// ------------------------------------------------------------------------------------------------
template <bool BLOCK>
__global__ void __launch_bounds__(256) k_edge_mlp2(EdgeOp A, DenseOp W1, const float* __restrict__ b1,
                                                   const float* __restrict__ s1, const float* __restrict__ t1,
                                                   DenseOp W2, Epilogue ep2, int E) {
  constexpr int BK = BLOCK ? 32 : 16, LD = BK + 1, KQ = BK / 4, NL = (64 * KQ) / 256, LDH = 65;
  __shared__ float As[64 * LD];
  __shared__ float Bs[64 * LD];
  __shared__ float Hs[64 * LDH];
  __shared__ float W2s[64 * LDH];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = blockIdx.x * 64;
  const int col = wn * 32 + l31;
  const int K1 = A.cols, KX = BLOCK ? 2 * A.Cin : K1;     // KX: extent covered by the BK-wide steps

  // epilogue constants + W2 (64x64) prefetched now, consumed after GEMM1
  const float bias1 = b1[col], sc1 = s1 ? s1[col] : 1.f, sh1 = s1 ? t1[col] : 0.f;
  const EpiPre pre2 = epi_prefetch(ep2, row0 + wm * 32, col, E, 64);
  float rw2[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    W2.template load4<false>(i >> 4, 4 * (i & 15), rw2[t]);
  }

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float ra[NL][4], rb[NL][4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int i = tid + t * 256;
      if (BLOCK) {
        A.template load4<true>(row0 + i / KQ, k0 + 4 * (i % KQ), ra[t]);
        W1.template load4<true>(i / KQ, k0 + 4 * (i % KQ), rb[t]);
      } else {
        A.template load4<false>(row0 + i / KQ, k0 + 4 * (i % KQ), ra[t]);
        W1.template load4<false>(i / KQ, k0 + 4 * (i % KQ), rb[t]);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int i = tid + t * 256;
      float* d = As + (i / KQ) * LD + 4 * (i % KQ);
      d[0] = ra[t][0]; d[1] = ra[t][1]; d[2] = ra[t][2]; d[3] = ra[t][3];
      float* e = Bs + (i / KQ) * LD + 4 * (i % KQ);
      e[0] = rb[t][0]; e[1] = rb[t][1]; e[2] = rb[t][2]; e[3] = rb[t][3];
    }
  };
  // the attr columns (BLOCK): 64 rows x one float4 of A (threads 0..63) and of W1 (threads 64..127)
  float rattr[4] = {0.f, 0.f, 0.f, 0.f};
  if (BLOCK) {
    if (tid < 64) A.template load4<true>(row0 + tid, KX, rattr);
    else if (tid < 128) W1.template load4<true>(tid - 64, KX, rattr);
  }
  fetch(0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {       // W2 -> LDS (first barrier below publishes it)
    const int i = tid + t * 256;
    float* d = W2s + (i >> 4) * LDH + 4 * (i & 15);
    d[0] = rw2[t][0]; d[1] = rw2[t][1]; d[2] = rw2[t][2]; d[3] = rw2[t][3];
  }
  for (int k0 = 0; k0 < KX; k0 += BK) {
    stage();
    __syncthreads();
    if (k0 + BK < KX) fetch(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float a = As[(wm * 32 + l31) * LD + kk + lhi];
      const float b = Bs[(wn * 32 + l31) * LD + kk + lhi];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (BLOCK) {
    if (tid < 128) {
      float* d = (tid < 64 ? As + tid * LD : Bs + (tid - 64) * LD);
      d[0] = rattr[0]; d[1] = rattr[1]; d[2] = rattr[2]; d[3] = rattr[3];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; kk += 2) {
      const float a = As[(wm * 32 + l31) * LD + kk + lhi];
      const float b = Bs[(wn * 32 + l31) * LD + kk + lhi];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  // layer-1 epilogue -> LDS (same arithmetic as wave_epilogue: +bias, fma(scale, shift), relu)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    Hs[row * LDH + col] = fmaxf(fmaf(acc[r] + bias1, sc1, sh1), 0.f);
  }
  __syncthreads();
  f32x16 acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll 8
  for (int kk = 0; kk < 64; kk += 2) {
    const float a = Hs[(wm * 32 + l31) * LDH + kk + lhi];
    const float b = W2s[(wn * 32 + l31) * LDH + kk + lhi];
    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc2, 0, 0, 0);
  }
  wave_epilogue(acc2, row0 + wm * 32, col, lhi, ep2, E, 64, pre2);
}

extern "C" int yolat_edge_mlp2_eval(const float* x, int64_t ldx, int64_t N, int64_t Cin,
                                    const int32_t* src_csr, const int32_t* dst_csr, const float* attr_csr,
                                    int64_t E, const float* W1, const float* b1, const float* s1,
                                    const float* t1, const float* W2, const float* b2, const float* s2,
                                    const float* t2, int64_t C, float* H2, int64_t ldh,
                                    yolat_stream_t stream) {
  if (E < 0 || N <= 0 || Cin <= 0 || !x || !W1 || !W2 || !b1) return YOLAT_E_INVALID;
  if (C != 64) return YOLAT_E_UNSUPPORTED;
  if (E == 0) return 0;
  if (!src_csr || !dst_csr || !attr_csr || !H2 || E >= (1LL << 31) || ldh < C || ldx < Cin)
    return YOLAT_E_INVALID;
  if ((s1 == nullptr) != (t1 == nullptr) || (s2 == nullptr) != (t2 == nullptr)) return YOLAT_E_INVALID;
  const long K1 = 2 * Cin + 4;
  EdgeOp a = yl_edge(x, ldx, Cin, src_csr, dst_csr, attr_csr, E);
  DenseOp w1 = yl_dense(W1, K1, C, K1), w2 = yl_dense(W2, C, C, C);
  Epilogue ep;
  ep.bias = b2; ep.scale = s2; ep.shift = t2; ep.relu = 1;
  ep.Y = H2; ep.ldy = ldh; ep.accumulate = 0; ep.stats = nullptr; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(yl_cdiv(E, 64));
  if (Cin % 32 == 0 && a.vec && w1.vec)
    hipLaunchKernelGGL(k_edge_mlp2<true>, grid, dim3(256), 0, st, a, w1, b1, s1, t1, w2, ep, (int)E);
  else
    hipLaunchKernelGGL(k_edge_mlp2<false>, grid, dim3(256), 0, st, a, w1, b1, s1, t1, w2, ep, (int)E);
  YL_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Factorised eval-mode edge MLP: layer 1 is a gather-add of per-node products (see yolat_hip.h):
//   h1[q] = relu(s1*(U[dst_q] + V[src_q] + Wc4.attr_q + b1) + t1)   (VALU, 64 floats per edge)
//   H2[q] = relu(s2*(W2.h1[q] + b2) + t2)                            (MFMA, 32 per wave per 64-edge tile)
// The K = 2*Cin part of the per-edge GEMM (64 of the 98 MFMAs of k_edge_mlp2) is gone: it was computed
// once per node by k_gemm_nt_node3.  Thread (row r, float4 column q): the 16 threads of a row share its
// two index loads; all 8 index loads and then all 12 row gathers of a thread are issued together.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_edge_uv_mlp2(const float* __restrict__ UV, long ld_uv,
                                                      const int* __restrict__ src, const int* __restrict__ dst,
                                                      const float* __restrict__ attr,
                                                      const float* __restrict__ Wc4, const float* __restrict__ b1,
                                                      const float* __restrict__ s1, const float* __restrict__ t1,
                                                      DenseOp W2, Epilogue ep2, int E) {
  constexpr int LDH = 65;
  __shared__ float Hs[64 * LDH];
  __shared__ float W2s[64 * LDH];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  const int row0 = blockIdx.x * 64;
  const int q = tid & 15, rb = tid >> 4;             // this thread: columns 4q..4q+3 of rows rb, rb+16, rb+32, rb+48
  const EpiPre pre2 = epi_prefetch(ep2, row0 + wm * 32, wn * 32 + l31, E, 64);
  // W2 -> registers -> LDS, per-column constants of layer 1
  float rw2[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    W2.template load4<false>(i >> 4, 4 * (i & 15), rw2[t]);
  }
  float4 wc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wc[j] = *reinterpret_cast<const float4*>(Wc4 + (4 * q + j) * 4);
  const float4 bb = b1 ? *reinterpret_cast<const float4*>(b1 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s1) { sc = *reinterpret_cast<const float4*>(s1 + 4 * q); sh = *reinterpret_cast<const float4*>(t1 + 4 * q); }
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
    const int i = tid + t * 256;
    float* d = W2s + (i >> 4) * LDH + 4 * (i & 15);
    d[0] = rw2[t][0]; d[1] = rw2[t][1]; d[2] = rw2[t][2]; d[3] = rw2[t][3];
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    auto one = [&](float uu, float vv, const float4& w, float b, float s, float h) {
      float z = uu + vv;
      z = fmaf(a[t].x, w.x, z); z = fmaf(a[t].y, w.y, z); z = fmaf(a[t].z, w.z, z); z = fmaf(a[t].w, w.w, z);
      return fmaxf(fmaf(z + b, s, h), 0.f);
    };
    float* hrow = Hs + (rb + 16 * t) * LDH + 4 * q;
    hrow[0] = one(u[t].x, v[t].x, wc[0], bb.x, sc.x, sh.x);
    hrow[1] = one(u[t].y, v[t].y, wc[1], bb.y, sc.y, sh.y);
    hrow[2] = one(u[t].z, v[t].z, wc[2], bb.z, sc.z, sh.z);
    hrow[3] = one(u[t].w, v[t].w, wc[3], bb.w, sc.w, sh.w);
  }
  __syncthreads();
  f32x16 acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll 8
  for (int kk = 0; kk < 64; kk += 2) {
    const float av = Hs[(wm * 32 + l31) * LDH + kk + lhi];
    const float bv = W2s[(wn * 32 + l31) * LDH + kk + lhi];
    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc2, 0, 0, 0);
  }
  wave_epilogue(acc2, row0 + wm * 32, wn * 32 + l31, lhi, ep2, E, 64, pre2);
}

// ------------------------------------------------------------------------------------------------
// Factorised edge MLP + mean aggregation in one kernel (eval): the [E,64] message matrix never reaches HBM.
// One workgroup = `npt` consecutive destination nodes (<= 16) = the contiguous CSR edge range
// [row_ptr[n0], row_ptr[n0+npt]) processed in passes of 64 edges (npt is chosen by the host so that one pass
// is the common case).  Per pass: gather-add layer 1 -> LDS -> MFMA layer 2 -> BN+ReLU -> LDS; then thread
// (node j, float4 column q) adds the pass's rows of node j in ascending edge order to its running sum.  At
// the end  f_out[n] += sum / deg  on top of the root Linear the node-side launch wrote.  No atomics; the
// per-node summation order is the CSR order, bit-identical to k_edge_uv_mlp2 + k_csr_mean_fwd.
// ------------------------------------------------------------------------------------------------
// NG = 16-node groups per tile: 1 (<= 16 nodes, the dense-graph case) or 4 (<= 64 nodes: graphs with ~1 edge per
// node — the Floorplans shape — would otherwise fill a 64-edge pass to a third).
#ifdef YOLAT_EDGE_STAMPS
// debug build only (tools/exp/r06_edge_stamps.sh): wall-clock stamps (100 MHz) of thread 0 of every node-tile workgroup.
// The stamped build is for the STRUCTURE of a workgroup's time; a stamp is a scalar memory read + a wait + a store, and the
// build that carries them schedules differently (round 6: two load re-orderings that cut the stamped workgroup from 13.4 to
// 9.2 us left the product build's launch where it was, by rocprof) — changes are judged by A/B of product builds.
__device__ long long edge_stamps_d[2][4096 * 16];
#define EDGE_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) edge_stamps_d[nx.Wp != nullptr ? 0 : 1][blockIdx.x * 16 + (k)] = wall_clock64(); } while (0)
extern "C" int yolat_debug_edge_stamps(long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(edge_stamps_d), sizeof(long long) * (size_t)n);
}
#else
#define EDGE_STAMP(k) do { } while (0)
#endif
// NEXT (NG == 1 only): the instance that also carries the next layer's node side (EdgeNext).  The last conv layer's
// launch has none, and its instance must not pay the 32 B-fragment registers for it.
// Registers: an NG == 1 workgroup is one wave per SIMD, and what decides how many of them share a CU is the register
// file (512 per lane per SIMD), before LDS (4 x 32.6 KB) and wave slots: both NG == 1 instances are bound to 4 waves per
// SIMD, i.e. <= 128 unified VGPRs, and reach it without scratch (tests/test_kernel_resources_host.py).  NG == 4 keeps
// the open bound: it spills at 128.
template <int NG, bool NEXT>
__global__ void __launch_bounds__(256, NG == 1 ? 4 : 1) k_edge_uv_mlp2_mean(const float* __restrict__ UV, long ld_uv,
                                                           const int* __restrict__ src,
                                                           const int* __restrict__ dst,
                                                           const float* __restrict__ attr,
                                                           const int* __restrict__ row_ptr, int N, int npt,
                                                           const float* __restrict__ Wc4,
                                                           const float* __restrict__ b1,
                                                           const float* __restrict__ s1,
                                                           const float* __restrict__ t1, DenseOp W2,
                                                           const float* __restrict__ b2,
                                                           const float* __restrict__ s2,
                                                           const float* __restrict__ t2, float* f_out, long ld_fo,
                                                           int E, int tiles, PoolRider rider, EdgeNext nx) {
  // workgroups past the node tiles: the next layer's node-branch tiles (EdgeNext), then the pooling-prologue rider
  // (internal.hpp) — both independent of this layer's messages
  if ((int)blockIdx.x >= tiles + nx.s_tiles) {
    yl_pool_rider(rider, blockIdx.x - tiles - nx.s_tiles, rider.blocks, threadIdx.x, 256);
    return;
  }
  constexpr int LDH = 65;
  __shared__ float Hs[64 * LDH];      // layer-1 activations of the pass, then the layer-2 messages
  __shared__ float W2s[64 * LDH];
  __shared__ int rp[16 * NG + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  if (NEXT && (int)blockIdx.x >= tiles) {
    // s'[r0 .. r0+63] = relu(((s . Wn'^T) + bn') * sn' + tn'): one 64 x 64 x 64 tile on the same LDS tiles and the same
    // MFMA loop (k ascending in pairs) as layer 2 below — bit-identical to k_gemm_nt_node3's tile
    const int r0 = (blockIdx.x - tiles) * 64;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = tid + t * 256, row = i >> 4, c4 = 4 * (i & 15);
      const float4 av = *reinterpret_cast<const float4*>(nx.s_in + (long)yl_min(r0 + row, N - 1) * nx.ld_si + c4);
      const float4 wv = *reinterpret_cast<const float4*>(nx.Wn + row * 64 + c4);
      float* da = Hs + row * LDH + c4;
      float* dw = W2s + row * LDH + c4;
      da[0] = av.x; da[1] = av.y; da[2] = av.z; da[3] = av.w;
      dw[0] = wv.x; dw[1] = wv.y; dw[2] = wv.z; dw[3] = wv.w;
    }
    const int colS = wn * 32 + l31;
    const float bS = nx.bn ? nx.bn[colS] : 0.f, scS = nx.sn[colS], shS = nx.tn[colS];
    __syncthreads();
    f32x16 accS;
#pragma unroll
    for (int r = 0; r < 16; ++r) accS[r] = 0.f;
#pragma unroll 8
    for (int kk = 0; kk < 64; kk += 2) {
      const float av = Hs[(wm * 32 + l31) * LDH + kk + lhi];
      const float bv = W2s[(wn * 32 + l31) * LDH + kk + lhi];
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, accS, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      if (row < N) nx.s_out[(long)row * nx.ld_so + colS] = fmaxf(fmaf(accS[r] + bS, scS, shS), 0.f);
    }
    return;
  }
  const int n0 = blockIdx.x * npt;
  const int nn = yl_min(npt, N - n0);                 // nodes of this tile
  EDGE_STAMP(0);
  if (tid <= 16 * NG) rp[tid] = row_ptr[yl_min(n0 + tid, n0 + nn)];
  const int q = tid & 15, rb = tid >> 4;              // gather role: columns 4q..4q+3 of rows rb + 16t
  const int col = wn * 32 + l31;                      // MFMA role: output column of this lane
  // the tile's edge range straight from global (same two addresses in every lane: one broadcast load each), so that
  // the first pass's index loads go out before the barrier below instead of after it, and the f_out rows this thread
  // finishes with at the very end: both shorten the workgroup's chain of dependent global round trips, which is what
  // a small graph's launch time consists of (715 node tiles at E = 40 k, 872 / 971 workgroups with the riders: four per CU
  // by registers and LDS, so one round of an empty GPU's 1024 slots)
  const int e0g = row_ptr[n0], e1g = row_ptr[n0 + nn];
  int di0[4], si0[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = yl_min(e0g + rb + 16 * t, E - 1);
    di0[t] = dst[e]; si0[t] = src[e];
  }
  float4 fo[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j)
    fo[j] = *reinterpret_cast<const float4*>(f_out + (long)yl_min(n0 + rb + 16 * j, N - 1) * ld_fo + 4 * q);
  float rw2[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    W2.template load4<false>(i >> 4, 4 * (i & 15), rw2[t]);
  }
  float4 wc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wc[j] = *reinterpret_cast<const float4*>(Wc4 + (4 * q + j) * 4);
  const float4 bb = b1 ? *reinterpret_cast<const float4*>(b1 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s1) { sc = *reinterpret_cast<const float4*>(s1 + 4 * q); sh = *reinterpret_cast<const float4*>(t1 + 4 * q); }
  const float bias2 = b2 ? b2[col] : 0.f, sc2 = s2 ? s2[col] : 1.f, sh2 = s2 ? t2[col] : 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    float* d = W2s + (i >> 4) * LDH + 4 * (i & 15);
    d[0] = rw2[t][0]; d[1] = rw2[t][1]; d[2] = rw2[t][2]; d[3] = rw2[t][3];
  }
  EDGE_STAMP(1);
  __syncthreads();
  EDGE_STAMP(2);
  const int e0 = e0g, e1 = e1g;
  int my_b[NG], my_e[NG];                             // aggregation role: nodes rb + 16 j, columns 4q..
  float4 sum[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    my_b[j] = rp[yl_min(rb + 16 * j, nn)]; my_e[j] = rp[yl_min(rb + 16 * j + 1, nn)];
    sum[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int c0 = e0; c0 < e1; c0 += 64) {
    int di[4], si[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (c0 == e0) { di[t] = di0[t]; si[t] = si0[t]; }          // loaded before the barrier
      else {
        const int e = yl_min(c0 + rb + 16 * t, E - 1);
        di[t] = dst[e]; si[t] = src[e];
      }
    }
    float4 u[4], v[4], a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = yl_min(c0 + rb + 16 * t, E - 1);
      u[t] = *reinterpret_cast<const float4*>(UV + (long)di[t] * ld_uv + 4 * q);
      v[t] = *reinterpret_cast<const float4*>(UV + (long)si[t] * ld_uv + 64 + 4 * q);
      a[t] = *reinterpret_cast<const float4*>(attr + (long)e * 4);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      auto one = [&](float uu, float vv, const float4& w, float b, float s, float h) {
        float z = uu + vv;
        z = fmaf(a[t].x, w.x, z); z = fmaf(a[t].y, w.y, z); z = fmaf(a[t].z, w.z, z); z = fmaf(a[t].w, w.w, z);
        return fmaxf(fmaf(z + b, s, h), 0.f);
      };
      float* hrow = Hs + (rb + 16 * t) * LDH + 4 * q;
      hrow[0] = one(u[t].x, v[t].x, wc[0], bb.x, sc.x, sh.x);
      hrow[1] = one(u[t].y, v[t].y, wc[1], bb.y, sc.y, sh.y);
      hrow[2] = one(u[t].z, v[t].z, wc[2], bb.z, sc.z, sh.z);
      hrow[3] = one(u[t].w, v[t].w, wc[3], bb.w, sc.w, sh.w);
    }
    if (c0 == e0) EDGE_STAMP(3);
    __syncthreads();
    if (c0 == e0) EDGE_STAMP(4);
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll 8
    for (int kk = 0; kk < 64; kk += 2) {
      const float av = Hs[(wm * 32 + l31) * LDH + kk + lhi];
      const float bv = W2s[(wn * 32 + l31) * LDH + kk + lhi];
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc2, 0, 0, 0);
    }
    if (c0 == e0) EDGE_STAMP(5);
    __syncthreads();                      // every wave is done reading Hs as the layer-1 tile
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      Hs[row * LDH + col] = fmaxf(fmaf(acc2[r] + bias2, sc2, sh2), 0.f);
    }
    __syncthreads();
    if (c0 == e0) EDGE_STAMP(6);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      if (rb + 16 * j < nn) {             // rows of node rb + 16 j inside this pass, ascending edge order
        const int lo = my_b[j] > c0 ? my_b[j] : c0;
        const int hi = my_e[j] < c0 + 64 ? my_e[j] : c0 + 64;
        for (int e = lo; e < hi; ++e) {
          const float* m = Hs + (e - c0) * LDH + 4 * q;
          sum[j].x += m[0]; sum[j].y += m[1]; sum[j].z += m[2]; sum[j].w += m[3];
        }
      }
    }
    if (c0 == e0) EDGE_STAMP(7);
    __syncthreads();
  }
  EDGE_STAMP(8);
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int deg = my_e[j] - my_b[j];
    if (rb + 16 * j < nn && deg > 0) {
      const float inv = 1.f / (float)deg;
      float4* o = reinterpret_cast<float4*>(f_out + (long)(n0 + rb + 16 * j) * ld_fo + 4 * q);
      float4 d = fo[j];                                // this workgroup is the only writer of its nodes' rows
      // explicit mul then add (no fma contraction): the same two roundings as k_csr_mean_fwd*
      d.x = yl_mul_rn(sum[j].x, inv) + d.x; d.y = yl_mul_rn(sum[j].y, inv) + d.y;
      d.z = yl_mul_rn(sum[j].z, inv) + d.z; d.w = yl_mul_rn(sum[j].w, inv) + d.w;
      *o = d;
      fo[j] = d;
    }
  }
  EDGE_STAMP(9);
  // ---- node side of the NEXT layer for this tile's nodes (EdgeNext, internal.hpp): [nn <= 16, 64] x [192, 64]^T
  if constexpr (NG == 1 && NEXT) {
    // all three column tiles' B fragments are fetched here in ONE batch of 48 loads, after the pass loop (nothing of the
    // edge phase is live any more, so they fit the 128 registers of four workgroups per CU; held from before the first
    // barrier they did not).  One round trip to L2 instead of three dependent ones: 16 MFMAs of 16x16x4 (~0.2 us) cover
    // nothing of a round's latency.
    float bf[3][16];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) bf[t][ks] = nx.Wp[((wave + 4 * t) * 16 + ks) * 64 + lane];
    float nbias[3];                                  // in the same batch: fetched under a column tile's MFMAs they are a round trip each
#pragma unroll
    for (int t = 0; t < 3; ++t) nbias[t] = nx.bias[(wave + 4 * t) * 16 + (lane & 15)];
    // the loop above ended with a barrier (or never ran): Hs is free; rows >= nn hold the clamped load of row N-1 or
    // stale sums — finite or not, their products only reach output rows that are never stored
    float* frow = Hs + rb * LDH + 4 * q;
    const float4 fz = (rb < nn) ? fo[0] : make_float4(0.f, 0.f, 0.f, 0.f);
    frow[0] = fz.x; frow[1] = fz.y; frow[2] = fz.z; frow[3] = fz.w;
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int ct = wave + 4 * t;                   // 12 column tiles of 16: UV' 0..7, root' 8..11
      const int col = ct * 16 + fr;
      const float bias = nbias[t];
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Hs[fr * LDH + 4 * ks + fk], bf[t][ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * fk + r;
        if (row < nn) {
          const float v = acc[r] + bias;
          if (col < 128) nx.UV[(long)(n0 + row) * nx.ld_uv + col] = v;
          else nx.root[(long)(n0 + row) * nx.ld_root + (col - 128)] = v;
        }
      }
    }
  }
  EDGE_STAMP(10);
#ifdef YOLAT_EDGE_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 4096) edge_stamps_d[nx.Wp != nullptr ? 0 : 1][blockIdx.x * 16 + 11] = (long long)((e1g - e0g + 63) / 64);
#endif
}

// ---- the phases of a node tile of k_edge_uv_mlp2_mean<1, *> above as inlined functions, for k_edge_mt_uv_mlp2_mean below:
// statement for statement that kernel's loads, products, sums and roundings, in its order.  (The one-tile kernel keeps its
// own body: routed through these functions it computes the same values but is scheduled differently — other registers,
// other instruction order — and measured 0.2-0.3 % slower one forward at a time, outside the spread of the unchanged code;
// the latency regime has to stay exactly what it was.  tests/test_gpu_eval_regime.py holds the two bit-equal.)
constexpr int EDGE_LDH = 65;
// per-thread constants of layer 1 (gather role: columns 4q..4q+3)
struct EdgeL1 { float4 wc[4]; float4 bb, sc, sh; };
__device__ __forceinline__ void edge_l1_consts(EdgeL1& k, const float* __restrict__ Wc4, const float* __restrict__ b1,
                                               const float* __restrict__ s1, const float* __restrict__ t1, int q) {
#pragma unroll
  for (int j = 0; j < 4; ++j) k.wc[j] = *reinterpret_cast<const float4*>(Wc4 + (4 * q + j) * 4);
  k.bb = b1 ? *reinterpret_cast<const float4*>(b1 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  k.sc = make_float4(1.f, 1.f, 1.f, 1.f); k.sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s1) { k.sc = *reinterpret_cast<const float4*>(s1 + 4 * q); k.sh = *reinterpret_cast<const float4*>(t1 + 4 * q); }
}
// W2 -> registers (issued early) -> LDS
__device__ __forceinline__ void edge_w2_load(const DenseOp& W2, int tid, float (&rw2)[4][4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    W2.template load4<false>(i >> 4, 4 * (i & 15), rw2[t]);
  }
}
__device__ __forceinline__ void edge_w2_store(float* W2s, int tid, const float (&rw2)[4][4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256;
    float* d = W2s + (i >> 4) * EDGE_LDH + 4 * (i & 15);
    d[0] = rw2[t][0]; d[1] = rw2[t][1]; d[2] = rw2[t][2]; d[3] = rw2[t][3];
  }
}
// one 64-edge pass, gather role: rows rb + 16 t of the pass that starts at edge c0 -> layer-1 activations in Hs
__device__ __forceinline__ void edge_gather_layer1(const float* __restrict__ UV, long ld_uv, const float* __restrict__ attr,
                                                   int c0, int E, int rb, int q, const int (&di)[4], const int (&si)[4],
                                                   const EdgeL1& k, float* Hs) {
  float4 u[4], v[4], a[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = yl_min(c0 + rb + 16 * t, E - 1);
    u[t] = *reinterpret_cast<const float4*>(UV + (long)di[t] * ld_uv + 4 * q);
    v[t] = *reinterpret_cast<const float4*>(UV + (long)si[t] * ld_uv + 64 + 4 * q);
    a[t] = *reinterpret_cast<const float4*>(attr + (long)e * 4);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    auto one = [&](float uu, float vv, const float4& w, float b, float s, float h) {
      float z = uu + vv;
      z = fmaf(a[t].x, w.x, z); z = fmaf(a[t].y, w.y, z); z = fmaf(a[t].z, w.z, z); z = fmaf(a[t].w, w.w, z);
      return fmaxf(fmaf(z + b, s, h), 0.f);
    };
    float* hrow = Hs + (rb + 16 * t) * EDGE_LDH + 4 * q;
    hrow[0] = one(u[t].x, v[t].x, k.wc[0], k.bb.x, k.sc.x, k.sh.x);
    hrow[1] = one(u[t].y, v[t].y, k.wc[1], k.bb.y, k.sc.y, k.sh.y);
    hrow[2] = one(u[t].z, v[t].z, k.wc[2], k.bb.z, k.sc.z, k.sh.z);
    hrow[3] = one(u[t].w, v[t].w, k.wc[3], k.bb.w, k.sc.w, k.sh.w);
  }
}
// the 64 x 64 x 64 product of the two LDS tiles, k ascending in pairs: this wave's 32 x 32 quarter
__device__ __forceinline__ f32x16 edge_mfma_tile(const float* Hs, const float* W2s, int wm, int wn, int l31, int lhi) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
  for (int kk = 0; kk < 64; kk += 2) {
    const float av = Hs[(wm * 32 + l31) * EDGE_LDH + kk + lhi];
    const float bv = W2s[(wn * 32 + l31) * EDGE_LDH + kk + lhi];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}
// layer 2's bias / BatchNorm / ReLU -> the pass's messages in Hs
__device__ __forceinline__ void edge_store_messages(const f32x16& acc2, float* Hs, int wm, int lhi, int col, float bias2,
                                                    float sc2, float sh2) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    Hs[row * EDGE_LDH + col] = fmaxf(fmaf(acc2[r] + bias2, sc2, sh2), 0.f);
  }
}
// aggregation role: rows of node rb + 16 j inside the pass [c0, c0 + 64), ascending edge order
template <int NG>
__device__ __forceinline__ void edge_aggregate(const float* Hs, int c0, int rb, int q, int nn, const int (&my_b)[NG],
                                               const int (&my_e)[NG], float4 (&sum)[NG]) {
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    if (rb + 16 * j < nn) {
      const int lo = my_b[j] > c0 ? my_b[j] : c0;
      const int hi = my_e[j] < c0 + 64 ? my_e[j] : c0 + 64;
      for (int e = lo; e < hi; ++e) {
        const float* m = Hs + (e - c0) * EDGE_LDH + 4 * q;
        sum[j].x += m[0]; sum[j].y += m[1]; sum[j].z += m[2]; sum[j].w += m[3];
      }
    }
  }
}
// f_out[n] = sum / deg + root term (fo: the rows loaded earlier; holds the final rows afterwards)
template <int NG>
__device__ __forceinline__ void edge_mean_out(float* f_out, long ld_fo, int n0, int rb, int q, int nn, const int (&my_b)[NG],
                                              const int (&my_e)[NG], const float4 (&sum)[NG], float4 (&fo)[NG]) {
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int deg = my_e[j] - my_b[j];
    if (rb + 16 * j < nn && deg > 0) {
      const float inv = 1.f / (float)deg;
      float4* o = reinterpret_cast<float4*>(f_out + (long)(n0 + rb + 16 * j) * ld_fo + 4 * q);
      float4 d = fo[j];                                // this workgroup is the only writer of its nodes' rows
      // explicit mul then add (no fma contraction): the same two roundings as k_csr_mean_fwd*
      d.x = yl_mul_rn(sum[j].x, inv) + d.x; d.y = yl_mul_rn(sum[j].y, inv) + d.y;
      d.z = yl_mul_rn(sum[j].z, inv) + d.z; d.w = yl_mul_rn(sum[j].w, inv) + d.w;
      *o = d;
      fo[j] = d;
    }
  }
}
// s'[r0 .. r0+63] = relu(((s . Wn'^T) + bn') * sn' + tn'): one 64 x 64 x 64 tile on the same LDS tiles and the same
// MFMA loop (k ascending in pairs) as layer 2 — bit-identical to k_gemm_nt_node3's tile
__device__ __forceinline__ void edge_s_tile(const EdgeNext& nx, int N, int r0, float* Hs, float* W2s, int tid, int wm, int wn,
                                            int l31, int lhi) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + t * 256, row = i >> 4, c4 = 4 * (i & 15);
    const float4 av = *reinterpret_cast<const float4*>(nx.s_in + (long)yl_min(r0 + row, N - 1) * nx.ld_si + c4);
    const float4 wv = *reinterpret_cast<const float4*>(nx.Wn + row * 64 + c4);
    float* da = Hs + row * EDGE_LDH + c4;
    float* dw = W2s + row * EDGE_LDH + c4;
    da[0] = av.x; da[1] = av.y; da[2] = av.z; da[3] = av.w;
    dw[0] = wv.x; dw[1] = wv.y; dw[2] = wv.z; dw[3] = wv.w;
  }
  const int colS = wn * 32 + l31;
  const float bS = nx.bn ? nx.bn[colS] : 0.f, scS = nx.sn[colS], shS = nx.tn[colS];
  __syncthreads();
  const f32x16 accS = edge_mfma_tile(Hs, W2s, wm, wn, l31, lhi);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    if (row < N) nx.s_out[(long)row * nx.ld_so + colS] = fmaxf(fmaf(accS[r] + bS, scS, shS), 0.f);
  }
}
// node side of the NEXT layer for the nodes of ALL of a workgroup's tiles [tA, tB) (EdgeNext, internal.hpp), run once after
// the tile loop: per tile [nn <= 16, 64] x [192, 64]^T.  The B fragments depend on (wave, lane) only, so the 48 KB of Wp are
// fetched once per workgroup, as one batch of 48 loads per lane, instead of three dependent rounds of 16 per tile.  The
// tiles' finished f_out rows are re-read from global by the thread (rb, q) that wrote them (or left them as they were:
// degree 0), in the same batch: nothing is held across the tile loop.  Up to four tiles' rows are staged into rows 16 i ..
// of Hs (64 rows; free after the loop: it ended with a barrier or never ran) and each tile runs the three column-tile rounds
// of the one-tile kernel on the held fragments: ks ascending, the same MFMA, bias added after, the same stores.
__device__ __forceinline__ void edge_next_node_side_tiles(const EdgeNext& nx, const float* f_out, long ld_fo, int N, int npt,
                                                          int tA, int tB, int rb, int q, int wave, int lane, float* Hs) {
  // the rows of the group of tiles that starts at g0: rows of tiles past the group's last repeat that tile's and are never
  // read.  The first group's re-reads lead the batch, ahead of the fragments: what waits for this workgroup's last f_out
  // store then has every load of the phase in flight behind it
  int g0 = tA, cnt = yl_min(4, tB - tA);
  float4 fz[4];
  auto load_rows = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n0 = (g0 + yl_min(i, cnt - 1)) * npt;
      fz[i] = *reinterpret_cast<const float4*>(f_out + (long)yl_min(n0 + rb, N - 1) * ld_fo + 4 * q);
    }
  };
  load_rows();
  float bf[3][16];
  const float* wp = nx.Wp + (wave * 16 * 64 + lane);   // one base: the 48 loads differ by compile-time offsets
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) bf[t][ks] = wp[(4 * t * 16 + ks) * 64];
  const int fr = lane & 15, fk = lane >> 4;
  float bias[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) bias[t] = nx.bias[(wave + 4 * t) * 16 + fr];
  for (;;) {
    // rows >= nn are zero as in the one-tile kernel (their products only reach output rows that are never stored)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n0 = (g0 + yl_min(i, cnt - 1)) * npt;
      float* frow = Hs + (16 * i + rb) * EDGE_LDH + 4 * q;
      const bool in = rb < yl_min(npt, N - n0);
      frow[0] = in ? fz[i].x : 0.f; frow[1] = in ? fz[i].y : 0.f; frow[2] = in ? fz[i].z : 0.f; frow[3] = in ? fz[i].w : 0.f;
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const int n0 = (g0 + i) * npt;
      const int nn = yl_min(npt, N - n0);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int col = (wave + 4 * t) * 16 + fr;    // 12 column tiles of 16: UV' 0..7, root' 8..11
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Hs[(16 * i + fr) * EDGE_LDH + 4 * ks + fk], bf[t][ks], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * fk + r;
          if (row < nn) {
            const float v = acc[r] + bias[t];
            if (col < 128) nx.UV[(long)(n0 + row) * nx.ld_uv + col] = v;
            else nx.root[(long)(n0 + row) * nx.ld_root + (col - 128)] = v;
          }
        }
      }
    }
    g0 += 4;
    if (g0 >= tB) break;
    cnt = yl_min(4, tB - g0);
    load_rows();
    __syncthreads();                                 // the previous group's rows have been read
  }
}

// ------------------------------------------------------------------------------------------------
// Several node tiles per workgroup (the THROUGHPUT regime of the eval forward, forward_eval.hip; NG == 1 shapes only).
// Under load a tile workgroup holds a quarter of a CU for as long as it lives, and 3.0-3.7 us of the 13.8 / 9.5 us of a
// k_edge_uv_mlp2_mean<1, *> workgroup are its start: the row_ptr -> edge-id round trips and staging the same 16 KB W2
// into LDS, once per ~14 nodes (profiles/r06_edge_stamps.txt).  Here a workgroup owns T consecutive tiles: W2, Wc4, the
// folded vectors and layer 2's constants are loaded once, and while tile t runs, the row_ptr range and the first pass's
// src / dst ids of tile t + 1 are on their way (consecutive tiles own consecutive CSR ranges, so tile t + 1 starts at tile
// t's end: its 64 dst ids, 64 src ids and 17 row_ptr entries are ONE load per thread, issued at the top of tile t next to
// that tile's f_out rows, landed with tile t's gathers and parked in the other half of a 2 x 145-int LDS array).  Tiles
// after the first start at the UV gather.  Per tile every product, sum and rounding is k_edge_uv_mlp2_mean<1, *>'s, in
// its order (the bodies above): bit-identical results (tests/test_gpu_eval_regime.py).  The next layer's node side (NEXT)
// runs once per workgroup, behind the last tile (edge_next_node_side_tiles): the packed weight is fetched once, not per tile
// (tests/test_gpu_edge_next_once.py).
// Grid: wgs = ceil(tiles / T) tile workgroups, then the node-branch tiles and the pooling rider as in the one-tile kernel.
// Bound like it: 256 threads, <= 128 VGPRs, no scratch, 4 x LDS <= 160 KB (tests/test_edge_mt_resources_host.py).
// ------------------------------------------------------------------------------------------------
template <bool NEXT>
__global__ void __launch_bounds__(256, 4) k_edge_mt_uv_mlp2_mean(const float* __restrict__ UV, long ld_uv,
                                                                 const int* __restrict__ src, const int* __restrict__ dst,
                                                                 const float* __restrict__ attr,
                                                                 const int* __restrict__ row_ptr, int N, int npt,
                                                                 const float* __restrict__ Wc4, const float* __restrict__ b1,
                                                                 const float* __restrict__ s1, const float* __restrict__ t1,
                                                                 DenseOp W2, const float* __restrict__ b2,
                                                                 const float* __restrict__ s2, const float* __restrict__ t2,
                                                                 float* f_out, long ld_fo, int E, int tiles, int T, int wgs,
                                                                 PoolRider rider, EdgeNext nx) {
  if ((int)blockIdx.x >= wgs + nx.s_tiles) {
    yl_pool_rider(rider, blockIdx.x - wgs - nx.s_tiles, rider.blocks, threadIdx.x, 256);
    return;
  }
  constexpr int LDH = EDGE_LDH;
  __shared__ float Hs[64 * LDH];
  __shared__ float W2s[64 * LDH];
  // a tile's start, written one tile ahead: [0, 64) dst ids and [64, 128) src ids of its first pass, [128, 145) its rp
  __shared__ int ahead[2][64 + 64 + 17];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  if (NEXT && (int)blockIdx.x >= wgs) {
    edge_s_tile(nx, N, (blockIdx.x - wgs) * 64, Hs, W2s, tid, wm, wn, l31, lhi);
    return;
  }
  const int q = tid & 15, rb = tid >> 4;
  const int col = wn * 32 + l31;
  const int tA = blockIdx.x * T, tB = yl_min(tA + T, tiles);   // this workgroup's tiles
  // this thread's share of the start of the tile at node nA whose edges begin at eA (tid >= 145: nothing)
  auto start_load = [&](int nA, int eA) -> int {
    if (tid < 64) return dst[yl_min(eA + tid, E - 1)];
    if (tid < 128) return src[yl_min(eA + tid - 64, E - 1)];
    if (tid < 145) return row_ptr[yl_min(nA + tid - 128, nA + yl_min(npt, N - nA))];
    return 0;
  };
  {
    const int n0 = tA * npt;
    const int e0g = row_ptr[n0];                      // broadcast load; the ids go out before the barrier below
    const int st = start_load(n0, e0g);
    float rw2[4][4];
    edge_w2_load(W2, tid, rw2);
    if (tid < 145) ahead[0][tid] = st;
    edge_w2_store(W2s, tid, rw2);
  }
  // the per-column constants of the two layers: loaded from global once.  Without the next layer's node side they stay in
  // registers through all tiles; the instance with it parks them in LDS (2.5 KB) and re-reads them at the top of every tile
  // (from when the node side ran per tile with 32 B-fragment registers; kept: with the node side behind the loop the
  // registers-only form was not measured)
  __shared__ EdgeL1 k1s[NEXT ? 16 : 1];
  __shared__ float c2s[NEXT ? 3 * 64 : 1];
  EdgeL1 k1;
  float bias2, sc2, sh2;
  if constexpr (NEXT) {
    if (rb == 0) edge_l1_consts(k1s[q], Wc4, b1, s1, t1, q);
    if (tid < 64) { c2s[tid] = b2 ? b2[tid] : 0.f; c2s[64 + tid] = s2 ? s2[tid] : 1.f; c2s[128 + tid] = s2 ? t2[tid] : 0.f; }
  } else {
    edge_l1_consts(k1, Wc4, b1, s1, t1, q);
    bias2 = b2 ? b2[col] : 0.f; sc2 = s2 ? s2[col] : 1.f; sh2 = s2 ? t2[col] : 0.f;
  }
  for (int t = tA; t < tB; ++t) {
    // the barrier that publishes ahead[cur] (and W2s for the first tile) and ends the previous tile's use of Hs
    __syncthreads();
    if constexpr (NEXT) { k1 = k1s[q]; bias2 = c2s[col]; sc2 = c2s[64 + col]; sh2 = c2s[128 + col]; }
    const int* cur = ahead[(t - tA) & 1];
    int* nxt = ahead[(t - tA + 1) & 1];
    const int n0 = t * npt;
    const int nn = yl_min(npt, N - n0);
    const int e0 = cur[128], e1 = cur[128 + nn];
    int my_b[1], my_e[1];
    float4 sum[1], fo[1];
    my_b[0] = cur[128 + yl_min(rb, nn)]; my_e[0] = cur[128 + yl_min(rb + 1, nn)];
    sum[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    fo[0] = *reinterpret_cast<const float4*>(f_out + (long)yl_min(n0 + rb, N - 1) * ld_fo + 4 * q);
    const bool more = t + 1 < tB;
    int st = 0;
    if (more) st = start_load(n0 + npt, e1);          // tile t + 1 begins where this one ends
    if (e0 >= e1 && more && tid < 145) nxt[tid] = st;  // no pass below: park it now (the next top barrier publishes it)
    for (int c0 = e0; c0 < e1; c0 += 64) {
      int di[4], si[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c0 == e0) { di[u] = cur[rb + 16 * u]; si[u] = cur[64 + rb + 16 * u]; }
        else {
          const int e = yl_min(c0 + rb + 16 * u, E - 1);
          di[u] = dst[e]; si[u] = src[e];
        }
      }
      edge_gather_layer1(UV, ld_uv, attr, c0, E, rb, q, di, si, k1, Hs);
      if (c0 == e0 && more && tid < 145) nxt[tid] = st;           // landed with (before) the gathers
      __syncthreads();
      const f32x16 acc2 = edge_mfma_tile(Hs, W2s, wm, wn, l31, lhi);
      __syncthreads();
      edge_store_messages(acc2, Hs, wm, lhi, col, bias2, sc2, sh2);
      __syncthreads();
      edge_aggregate<1>(Hs, c0, rb, q, nn, my_b, my_e, sum);
      __syncthreads();
    }
    if constexpr (NEXT) {
      // a use of the f_out rows on every path (they landed with the gathers): a lane that stores nothing would otherwise leave
      // the loop with the load formally pending, and the wait for it behind the loop also waits for the last tile's store
      asm volatile("" ::"v"(fo[0].x), "v"(fo[0].y), "v"(fo[0].z), "v"(fo[0].w));
    }
    edge_mean_out<1>(f_out, ld_fo, n0, rb, q, nn, my_b, my_e, sum, fo);
  }
  if constexpr (NEXT) {
    // the B-fragment addresses are derived here from a lane id the compiler cannot see through: computed above the tile loop
    // they would be registers held through every edge phase
    int lane_t = lane;
    asm volatile("" : "+v"(lane_t));
    edge_next_node_side_tiles(nx, f_out, ld_fo, N, npt, tA, tB, rb, q, wave, lane_t, Hs);
  }
}

// ------------------------------------------------------------------------------------------------
// Wave-specialised factorised edge MLP + mean aggregation (round 2) — the large-graph path.
// Why (profiles/r02_base_fwd_cfg5_pmc_sq_*.txt and the phase ablation in profiles/r02_edge_ablation.txt, cfg 5): the
// node-tiled kernel above runs its phases — gather, layer-1 VALU, layer-2 MFMA, aggregation — one after the other
// in every wave, and because all resident workgroups start together and contend for the same pipes they stay in
// lockstep: the phase times ADD (87 us without the MFMAs + 105 us of MFMA phase = 192 us) although the MFMA pipe
// needs only ~75 us of it; its 64-row passes are also only 75 % full and W2 is re-staged for every 96 edges.
// Here a 512-thread workgroup owns the edge range [w*chunk, (w+1)*chunk) moved to node boundaries (the node holding
// edge w*chunk is dst[w*chunk]: no search) and walks it in FULL 64-edge passes with two kinds of waves:
//   waves 0-3 "producers": per pass the row gathers U[dst] + V[src] + attr (issued one pass ahead of their use, the
//              indices two passes ahead), layer 1 on the VALU -> LDS tile Hs[(p+1)&1], and the per-node mean of the
//              messages of pass p-1 (segment table built from dst with one ballot per pass; the running sum of a
//              node that straddles two passes travels through 65 floats of LDS);
//   waves 4-7 "consumers": W2's MFMA B fragments in 32 registers for the whole kernel, per pass 8 ds_read_b128 (the
//              tile is stored k-parity-interleaved, row stride 68: one conflict-free read feeds four MFMAs) +
//              32 v_mfma_f32_32x32x2_f32 on Hs[p&1], BN+ReLU epilogue -> Ms[p&1].
// One s_barrier per pass; every SIMD hosts one producer and one consumer wave of each of the two resident
// workgroups.
//
// X6 = false: layer 2 on v_mfma_f32_32x32x2_f32 — the same arithmetic in the same order as k_edge_uv_mlp2 +
//   k_csr_mean_fwd (bit-identical results).  Measured 180 us at cfg 5 against 213 us for the node tiles: on gfx950 the
//   fp32-input MFMA executes on the SIMD's VECTOR ALUs (tools/exp/pipe_overlap.hip: the MFMA time and the VALU time
//   of two waves on one SIMD ADD, 124 + 104 -> 222 us), so specialising waves cannot overlap the two, and a single
//   VALU-heavy wave per SIMD issues one instruction per ~7 cycles (tools/exp/valu_rate.hip).
// X6 = true (the product path for large graphs): layer 2 as an fp32 GEMM EMULATED on the bf16 matrix cores, which
//   do run beside the vector ALUs: a = a_h + a_m + a_l with three bfloat16 terms (truncation splits, 8 + 8 + 8 = 24
//   significand bits: the split is exact), a.b = a_h b_h + (a_h b_m + a_m b_h + a_h b_l + a_l b_h + a_m b_m) + O(2^-24):
//   six v_mfma_f32_32x32x16_bf16 (32 cycles each) per 16 k instead of eight fp32 MFMAs (64 cycles each), exact
//   products, fp32 accumulation.  The result differs from the fp32-MFMA kernels only by the summation order
//   and the three dropped cross terms (< (8 + 2^-6) 2^-24 |a||b| per product); tests/test_gpu_edge_eval_elements.py holds
//   it per element to the fp32 kernels' derived bound plus that term (tests/edge_eval_ref.py: edge_stage_ref, x6).
// FOLD: layer 1's bias / BatchNorm live in UV and Wc4 (node-side epilogue; b1 = s1 = t1 = NULL) and layer 2's bias
//   in t2 (b2 = NULL): h1 = relu(U + V + Wc4.attr), message = relu(s2 * (W2.h1) + t2) — 6 instead of 8 VALU
//   operations per hidden activation (packed fp32 math) and 2 instead of 3 per message.
// ------------------------------------------------------------------------------------------------
typedef __bf16 yl_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned yl_u32x4 __attribute__((ext_vector_type(4)));
// exact 3-way bfloat16 split of 8 fp32 values (truncation: every term keeps the next 8 significand bits)
__device__ __forceinline__ void yl_split8(const float x[8], yl_bf16x8& h, yl_bf16x8& m, yl_bf16x8& l) {
  yl_u32x4 ph, pm, pl;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned x0 = __float_as_uint(x[2 * i]), x1 = __float_as_uint(x[2 * i + 1]);
    // h = top 8 significand bits, hm = top 16: m = hm - h and l = x - hm are exact and need 8 bits each
    const yl_f32x2 xv = {x[2 * i], x[2 * i + 1]};
    const yl_f32x2 hv = {__uint_as_float(x0 & 0xffff0000u), __uint_as_float(x1 & 0xffff0000u)};
    const yl_f32x2 hmv = {__uint_as_float(x0 & 0xffffff00u), __uint_as_float(x1 & 0xffffff00u)};
    const yl_f32x2 mv = hmv - hv, lv = xv - hmv;     // v_pk_add_f32 with negated operand
    ph[i] = __builtin_amdgcn_perm(x1, x0, 0x07060302u);
    pm[i] = __builtin_amdgcn_perm(__float_as_uint(mv.y), __float_as_uint(mv.x), 0x07060302u);
    pl[i] = __builtin_amdgcn_perm(__float_as_uint(lv.y), __float_as_uint(lv.x), 0x07060302u);
  }
  h = *reinterpret_cast<yl_bf16x8*>(&ph);
  m = *reinterpret_cast<yl_bf16x8*>(&pm);
  l = *reinterpret_cast<yl_bf16x8*>(&pl);
}

template <bool FOLD, bool X6>
__global__ void __launch_bounds__(512, 4) k_edge_uv_mlp2_mean_ws(const float* __restrict__ UV, long ld_uv,
                                                                 const int* __restrict__ src,
                                                                 const int* __restrict__ dst,
                                                                 const float* __restrict__ attr,
                                                                 const int* __restrict__ row_ptr, int N, int E, int chunk,
                                                                 const float* __restrict__ Wc4,
                                                                 const float* __restrict__ b1,
                                                                 const float* __restrict__ s1,
                                                                 const float* __restrict__ t1,
                                                                 const float* __restrict__ W2,
                                                                 const float* __restrict__ b2,
                                                                 const float* __restrict__ s2,
                                                                 const float* __restrict__ t2, float* f_out, long ld_fo) {
  constexpr int LDH = 68, TILE = 64 * LDH;
  __shared__ __attribute__((aligned(16))) float Hs[2 * TILE];   // layer-1 activations, k-parity-interleaved
  __shared__ __attribute__((aligned(16))) float Ms[2 * TILE];   // layer-2 messages, row-major
  __shared__ int seg_start[2][66];                              // first row of the k-th node of the pass (+ end)
  __shared__ int seg_node[2][64];
  __shared__ int seg_info[2][4];                                // #nodes, first continues from / last continues into
  __shared__ __attribute__((aligned(16))) float carry_s[2][64];
  __shared__ int carry_cnt_s[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // ---- this workgroup's edge range, moved to node boundaries (uniform)
  const long c_lo = (long)blockIdx.x * chunk;
  if (c_lo >= E) return;
  const long c_hi = c_lo + chunk;
  int eS = 0, eE = E;
  if (c_lo > 0) {
    const int n = dst[c_lo];
    eS = (row_ptr[n] == (int)c_lo) ? (int)c_lo : row_ptr[n + 1];
  }
  if (c_hi < E) {
    const int n = dst[c_hi];
    eE = (row_ptr[n] == (int)c_hi) ? (int)c_hi : row_ptr[n + 1];
  }
  if (eS >= eE) return;
  const int np = (eE - eS + 63) >> 6;

  if (wave >= 4) {
    // ================================ consumers: layer 2 on the matrix cores ================================
    const int cw = wave - 4, wm = cw >> 1, wn = cw & 1, l31 = lane & 31, lhi = lane >> 5;
    const int col = wn * 32 + l31;
    const float bias2 = (!FOLD && b2) ? b2[col] : 0.f, sc2 = s2 ? s2[col] : 1.f, sh2 = s2 ? t2[col] : 0.f;
    auto store_messages = [&](const f32x16& acc, int p) {
      float* ms = Ms + (p & 1) * TILE;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        ms[row * LDH + col] = FOLD ? fmaxf(fmaf(acc[r], sc2, sh2), 0.f) : fmaxf(fmaf(acc[r] + bias2, sc2, sh2), 0.f);
      }
    };
    if (X6) {
      // W2[col][16 ks + 8 lhi + 0..7] as three bfloat16 fragments per k step, resident for the whole kernel.
      // FOLD: the BatchNorm scale s2[col] is multiplied into W2's row before the split and the shift t2[col] is the
      // accumulator's initial value, so the epilogue is one add (the two accumulators) and the ReLU.
      yl_bf16x8 Bh[4], Bm[4], Bl[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float4* wp = reinterpret_cast<const float4*>(W2 + (long)col * 64 + 16 * ks + 8 * lhi);
        const float4 w0 = wp[0], w1 = wp[1];
        float x[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        if (FOLD) {
#pragma unroll
          for (int i = 0; i < 8; ++i) x[i] *= sc2;
        }
        yl_split8(x, Bh[ks], Bm[ks], Bl[ks]);
      }
      __syncthreads();                                // barrier 0: Hs[0] is complete
      for (int p = 0; p < np; ++p) {
        const float* arow = Hs + (p & 1) * TILE + (wm * 32 + l31) * LDH + 8 * lhi;
        f32x16 accM, accS;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accM[r] = FOLD ? sh2 : 0.f; accS[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const float4 a0 = *reinterpret_cast<const float4*>(arow + 16 * ks);
          const float4 a1 = *reinterpret_cast<const float4*>(arow + 16 * ks + 4);
          const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          yl_bf16x8 Ah, Am, Al;
          yl_split8(x, Ah, Am, Al);
          // two accumulators, three products each, alternating: no MFMA waits on the one issued just before it
          accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[ks], accS, 0, 0, 0);
          accM = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[ks], accM, 0, 0, 0);
          accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh[ks], accS, 0, 0, 0);
          accM = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm[ks], accM, 0, 0, 0);
          accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm[ks], accS, 0, 0, 0);
          accM = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[ks], accM, 0, 0, 0);
        }
        float* ms = Ms + (p & 1) * TILE;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
          const float z = accM[r] + accS[r];
          ms[row * LDH + col] = FOLD ? fmaxf(z, 0.f) : fmaxf(fmaf(z + bias2, sc2, sh2), 0.f);
        }
        __syncthreads();                              // barrier p+1: Ms[p&1] complete, Hs[p&1] free
      }
      return;
    }
    float bfrag[32];                                  // bfrag[m] = W2[col][2m + lhi]
    {
      const float4* wrow = reinterpret_cast<const float4*>(W2 + (long)col * 64);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float4 f = wrow[j];
        bfrag[2 * j] = lhi ? f.y : f.x;
        bfrag[2 * j + 1] = lhi ? f.w : f.z;
      }
    }
    __syncthreads();                                  // barrier 0: Hs[0] is complete
    for (int p = 0; p < np; ++p) {
      // fp32 path: Hs rows are k-parity-interleaved (position(k) = (k & 1) * 32 + (k >> 1)), so the A operands of four
      // consecutive MFMAs (k = 2m + lhi) are one ds_read_b128
      const float* arow = Hs + (p & 1) * TILE + (wm * 32 + l31) * LDH + lhi * 32;
      f32x16 acc2;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll
      for (int m4 = 0; m4 < 8; ++m4) {
        const float4 av = *reinterpret_cast<const float4*>(arow + 4 * m4);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bfrag[4 * m4 + 0], acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bfrag[4 * m4 + 1], acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bfrag[4 * m4 + 2], acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bfrag[4 * m4 + 3], acc2, 0, 0, 0);
      }
      store_messages(acc2, p);
      __syncthreads();                                // barrier p+1: Ms[p&1] complete, Hs[p&1] free
    }
    return;
  }

  // ================================== producers: gathers, layer 1, mean ==================================
  const int q = tid & 15, rb = tid >> 4;              // gather role: columns 4q..4q+3 of rows rb + 16t;
                                                      // aggregation role: nodes rb, rb+16, .. of the pass, same columns
  float4 wc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wc[j] = *reinterpret_cast<const float4*>(Wc4 + (4 * q + j) * 4);
  float4 bb = make_float4(0.f, 0.f, 0.f, 0.f), sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!FOLD) {
    if (b1) bb = *reinterpret_cast<const float4*>(b1 + 4 * q);
    if (s1) { sc = *reinterpret_cast<const float4*>(s1 + 4 * q); sh = *reinterpret_cast<const float4*>(t1 + 4 * q); }
  }
  int di[4], si[4];
  float4 u[4], v[4], a[4];
  // every load below is unconditional (addresses clamped into the range), so the compiler can count the loads in
  // flight: a pass beyond the range re-reads the last edge and its tile is never consumed
  // (uniform base + 32-bit byte offset: one VALU operation per address; the host checks that UV / attr / the index
  // arrays are smaller than 4 GiB)
  const unsigned ldb = (unsigned)ld_uv * 4u, qb = 16u * q;
  auto load_idx = [&](int c0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned eb = 4u * (unsigned)yl_min(c0 + rb + 16 * t, eE - 1);
      di[t] = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(dst) + eb);
      si[t] = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(src) + eb);
    }
  };
  auto gather = [&](int c0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned e = (unsigned)yl_min(c0 + rb + 16 * t, eE - 1);
      u[t] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(UV) + ((unsigned)di[t] * ldb + qb));
      v[t] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(UV) + ((unsigned)si[t] * ldb + qb + 256u));
      a[t] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(attr) + 16u * e);
    }
  };
  auto layer1 = [&](float* hs) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      auto one = [&](float uu, float vv, const float4& w, float b, float s, float h) {
        float z = uu + vv;
        z = fmaf(a[t].x, w.x, z); z = fmaf(a[t].y, w.y, z); z = fmaf(a[t].z, w.z, z); z = fmaf(a[t].w, w.w, z);
        return fmaxf(fmaf(z + b, s, h), 0.f);
      };
      float h0, h1, h2, h3;
      if (FOLD) {
        // packed fp32 math (v_pk_add_f32 / v_pk_fma_f32: two IEEE operations per instruction, same roundings)
        yl_f32x2 z02 = {u[t].x + v[t].x, u[t].z + v[t].z}, z13 = {u[t].y + v[t].y, u[t].w + v[t].w};
        const yl_f32x2 ax = {a[t].x, a[t].x}, ay = {a[t].y, a[t].y}, az = {a[t].z, a[t].z}, aw = {a[t].w, a[t].w};
        z02 = __builtin_elementwise_fma(ax, (yl_f32x2){wc[0].x, wc[2].x}, z02);
        z13 = __builtin_elementwise_fma(ax, (yl_f32x2){wc[1].x, wc[3].x}, z13);
        z02 = __builtin_elementwise_fma(ay, (yl_f32x2){wc[0].y, wc[2].y}, z02);
        z13 = __builtin_elementwise_fma(ay, (yl_f32x2){wc[1].y, wc[3].y}, z13);
        z02 = __builtin_elementwise_fma(az, (yl_f32x2){wc[0].z, wc[2].z}, z02);
        z13 = __builtin_elementwise_fma(az, (yl_f32x2){wc[1].z, wc[3].z}, z13);
        z02 = __builtin_elementwise_fma(aw, (yl_f32x2){wc[0].w, wc[2].w}, z02);
        z13 = __builtin_elementwise_fma(aw, (yl_f32x2){wc[1].w, wc[3].w}, z13);
        h0 = fmaxf(z02.x, 0.f); h2 = fmaxf(z02.y, 0.f); h1 = fmaxf(z13.x, 0.f); h3 = fmaxf(z13.y, 0.f);
      } else {
        h0 = one(u[t].x, v[t].x, wc[0], bb.x, sc.x, sh.x);
        h1 = one(u[t].y, v[t].y, wc[1], bb.y, sc.y, sh.y);
        h2 = one(u[t].z, v[t].z, wc[2], bb.z, sc.z, sh.z);
        h3 = one(u[t].w, v[t].w, wc[3], bb.w, sc.w, sh.w);
      }
      if (X6) {                                       // natural k order: the consumers read 8 consecutive k per lane
        *reinterpret_cast<float4*>(hs + (rb + 16 * t) * LDH + 4 * q) = make_float4(h0, h1, h2, h3);
      } else {
        float* hrow = hs + (rb + 16 * t) * LDH + 2 * q;
        *reinterpret_cast<float2*>(hrow) = make_float2(h0, h2);
        *reinterpret_cast<float2*>(hrow + 32) = make_float2(h1, h3);
      }
    }
  };
  // segment table of pass P from its 64 destination ids (lane = row); every producer wave writes the same values
  int dm_cur = dst[yl_min(eS + lane, eE - 1)], dm_nxt = dst[yl_min(eS + 64 + lane, eE - 1)], prev_last = -1;
  auto meta = [&](int P) {
    const int c0 = eS + 64 * P, bsel = P & 1;
    const int nrows = yl_min(64, eE - c0);
    const int dprev = __shfl_up(dm_cur, 1);
    const bool start = lane < nrows && (lane == 0 || dm_cur != dprev);
    const unsigned long long mask = __ballot(start);
    const int k = __popcll(mask & ((1ull << lane) - 1ull));
    if (start) { seg_start[bsel][k] = lane; seg_node[bsel][k] = dm_cur; }
    if (lane == 0) {
      const int nseg = __popcll(mask);
      seg_start[bsel][nseg] = nrows;
      seg_info[bsel][0] = nseg;
      seg_info[bsel][1] = (P > 0 && prev_last == dm_cur) ? 1 : 0;
    }
    const int first_next = __shfl(dm_nxt, 0);
    if (lane == 63) seg_info[bsel][2] = (c0 + 64 < eE && first_next == dm_cur) ? 1 : 0;
    prev_last = __shfl(dm_cur, 63);
    dm_cur = dm_nxt;
    dm_nxt = dst[yl_min(c0 + 128 + lane, eE - 1)];
  };
  // f_out row of this thread's FIRST node of pass P (the common case: <= 16 nodes per pass; further nodes load on
  // demand).  Issued one whole interval before aggregate(P) adds to it, unconditionally and clamped so that the
  // compiler can count the loads in flight: the wait in aggregate() then leaves the younger prefetches (next row
  // gathers, indices) in flight instead of draining them.  seg_node was written by this wave itself in meta(P).
  float4 fo0 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fo_load = [&](int P) {
    const int bsel = P & 1;
    const int k = yl_min(rb, seg_info[bsel][0] - 1);
    fo0 = *reinterpret_cast<const float4*>(f_out + (long)seg_node[bsel][k] * ld_fo + 4 * q);
  };
  auto aggregate = [&](int P) {
    const int bsel = P & 1;
    const float* ms = Ms + bsel * TILE + 4 * q;
    const int nseg = seg_info[bsel][0], cont_in = seg_info[bsel][1], cont_out = seg_info[bsel][2];
    for (int k = rb; k < nseg; k += 16) {
      const int lo = seg_start[bsel][k], hi = seg_start[bsel][k + 1];
      float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
      int cn = 0;
      if (k == 0 && cont_in) {
        sm = *reinterpret_cast<const float4*>(&carry_s[bsel ^ 1][4 * q]);
        cn = carry_cnt_s[bsel ^ 1];
      }
      for (int r = lo; r < hi; ++r) {
        const float4 m = *reinterpret_cast<const float4*>(ms + r * LDH);
        sm.x += m.x; sm.y += m.y; sm.z += m.z; sm.w += m.w;
      }
      cn += hi - lo;
      if (k == nseg - 1 && cont_out) {                // the node continues in the next pass
        *reinterpret_cast<float4*>(&carry_s[bsel][4 * q]) = sm;
        if (q == 0) carry_cnt_s[bsel] = cn;
      } else {
        const float inv = 1.f / (float)cn;
        float4* o = reinterpret_cast<float4*>(f_out + (long)seg_node[bsel][k] * ld_fo + 4 * q);
        float4 d = fo0;
        if (k != rb) d = *o;
        // explicit mul then add (no fma contraction): the same two roundings as k_csr_mean_fwd*
        d.x = yl_mul_rn(sm.x, inv) + d.x; d.y = yl_mul_rn(sm.y, inv) + d.y;
        d.z = yl_mul_rn(sm.z, inv) + d.z; d.w = yl_mul_rn(sm.w, inv) + d.w;
        *o = d;
      }
    }
  };
  load_idx(eS);
  gather(eS);
  load_idx(eS + 64);
  layer1(Hs);
  gather(eS + 64);
  load_idx(eS + 128);
  __syncthreads();                                    // barrier 0
  for (int p = 0; p < np; ++p) {
    layer1(Hs + ((p + 1) & 1) * TILE);                // pass p+1 (gathered during pass p-1 / the barrier)
    gather(eS + 64 * (p + 2));
    load_idx(eS + 64 * (p + 3));
    meta(p);
    if (p >= 1) aggregate(p - 1);                     // adds onto fo0 = rows loaded at the end of the last interval
    fo_load(p);
    __syncthreads();                                  // barrier p+1
  }
  aggregate(np - 1);
}

// nodes per node-tile workgroup: ~56 edges on average so that a single 64-edge pass is the common case
// (measured at cfg 5: 9 nodes / one pass 208 us, 12 nodes / a second mostly-empty pass 242 us, 16 nodes /
// two full passes 194 us — on big graphs two passes halve the per-workgroup W2 staging)
long yl_edge_tile_npt(long N, long E) {
  if (E <= 0) return 64;              // (the bf16 node-tile launch of a graph without edges; fp32 callers return earlier)
  long npt = (56 * N) / E;
  const long npt2 = (112 * N) / E < 16 ? (112 * N) / E : 16;
  if (npt2 >= 2 * npt - 2 && N / (npt2 > 0 ? npt2 : 1) >= 8192) npt = npt2;
  if (npt < 1) npt = 1;
  if (npt > 64) npt = 64;
  return npt;
}
int yl_edge_tile_groups(int64_t N, int64_t E) {
  if (N <= 0 || E <= 0) return 0;
  const int variant = E >= 131072 ? (yl_strict_fp32() ? YOLAT_EDGE_WS_F32 : YOLAT_EDGE_WS_X6) : YOLAT_EDGE_TILES;
  if (variant != YOLAT_EDGE_TILES) return 0;
  return yl_edge_tile_npt(N, E) <= 16 ? 1 : 4;
}

int yl_edge_uv_mlp2_mean_eval_impl(const float* UV, int64_t ld_uv, const int32_t* src_csr, const int32_t* dst_csr,
                                   const float* attr_csr, const int32_t* row_ptr, int64_t N, int64_t E, const float* Wc4,
                                   const float* b1, const float* s1, const float* t1, const float* W2, const float* b2,
                                   const float* s2, const float* t2, int64_t C, float* f_out, int64_t ld_fo, int variant,
                                   const PoolRider* rider, int* rode, const EdgeNext* next, int* did_next,
                                   yolat_stream_t stream, int tiles_per_wg) {
  if (rode) *rode = 0;
  if (did_next) *did_next = 0;
  if (E < 0 || N <= 0 || !UV || !Wc4 || !W2 || !row_ptr || !f_out) return YOLAT_E_INVALID;
  if (variant < YOLAT_EDGE_AUTO || variant > YOLAT_EDGE_WS_X6) return YOLAT_E_INVALID;
  if (tiles_per_wg < 1 || tiles_per_wg > YOLAT_EDGE_MT_MAX) return YOLAT_E_INVALID;
  if (C != 64) return YOLAT_E_UNSUPPORTED;
  if (E == 0) return 0;
  if (!src_csr || !dst_csr || !attr_csr || E >= (1LL << 31) || ld_fo < C || ld_uv < 2 * C) return YOLAT_E_INVALID;
  if ((s1 == nullptr) != (t1 == nullptr) || (s2 == nullptr) != (t2 == nullptr)) return YOLAT_E_INVALID;
  if (ld_uv % 4 != 0 || ld_fo % 4 != 0 || !yl_aligned16(UV) || !yl_aligned16(attr_csr) || !yl_aligned16(Wc4) ||
      (b1 && !yl_aligned16(b1)) || !yl_aligned16(f_out) || (s1 && (!yl_aligned16(s1) || !yl_aligned16(t1))))
    return YOLAT_E_UNSUPPORTED;
  // folded form: layer 1's bias / BatchNorm already applied to UV and Wc4 by the caller, layer 2's bias inside t2
  const bool fold = b1 == nullptr && s1 == nullptr && b2 == nullptr;
  const long ws_wgs = 512;            // persistent workgroups of the wave-specialised kernels: two per CU
  // the persistent kernel addresses UV / attr / the index arrays with 32-bit byte offsets
  const bool ws_ok = yl_aligned16(W2) && E >= 64 && N * ld_uv * 4 < (1LL << 32) && E * 16 < (1LL << 32);
  if (variant == YOLAT_EDGE_AUTO) {
    variant = E >= 131072 ? (yl_strict_fp32() ? YOLAT_EDGE_WS_F32 : YOLAT_EDGE_WS_X6) : YOLAT_EDGE_TILES;
    if (!ws_ok) variant = YOLAT_EDGE_TILES;
  } else if (variant != YOLAT_EDGE_TILES && !ws_ok) {
    return YOLAT_E_UNSUPPORTED;
  }
  if (variant != YOLAT_EDGE_TILES) {
    // 2 workgroups of 512 threads per CU, each walking a contiguous edge range in full 64-edge passes
    long chunk = ((E + ws_wgs - 1) / ws_wgs + 63) / 64 * 64;
    if (chunk < 64) chunk = 64;
    const unsigned grid = (unsigned)((E + chunk - 1) / chunk);
#define YL_WS_LAUNCH(F, X)                                                                                          \
  hipLaunchKernelGGL((k_edge_uv_mlp2_mean_ws<F, X>), dim3(grid), dim3(512), 0, (hipStream_t)stream, UV, (long)ld_uv,   \
                     src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)E, (int)chunk, Wc4, b1, s1, t1, W2, b2, s2, t2, \
                     f_out, (long)ld_fo)
    if (variant == YOLAT_EDGE_WS_X6) { if (fold) YL_WS_LAUNCH(true, true); else YL_WS_LAUNCH(false, true); }
    else { if (fold) YL_WS_LAUNCH(true, false); else YL_WS_LAUNCH(false, false); }
#undef YL_WS_LAUNCH
    YL_LAUNCH_CHECK();
    return 0;
  }
  const long npt = yl_edge_tile_npt(N, E);
  DenseOp w2 = yl_dense(W2, C, C, C);
  const int tiles = yl_cdiv(N, npt);
  PoolRider pr{};
  if (rider && rider->blocks > 0) { pr = *rider; if (rode) *rode = 1; }
  EdgeNext nx{};
  if (next && next->Wp && npt <= 16) {
    if (!next->bias || !next->UV || !next->root || next->UV == UV) return YOLAT_E_INVALID;
    if (next->s_tiles > 0 && (!next->s_in || !next->Wn || !next->sn || !next->tn || !next->s_out || next->ld_si % 4 != 0 ||
                              !yl_aligned16(next->s_in) || !yl_aligned16(next->Wn)))
      return YOLAT_E_INVALID;
    nx = *next;
    if (did_next) *did_next = 1;
  }
  // several tiles per workgroup: only where the one-tile kernel would be an NG == 1 instance; otherwise it is that kernel
  if (tiles_per_wg > 1 && npt <= 16) {
    const int wgs = yl_cdiv(tiles, tiles_per_wg);
    const unsigned mt_grid = (unsigned)wgs + (unsigned)nx.s_tiles + (unsigned)pr.blocks;
    if (nx.Wp != nullptr)
      hipLaunchKernelGGL((k_edge_mt_uv_mlp2_mean<true>), dim3(mt_grid), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv,
                         src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)npt, Wc4, b1, s1, t1, w2, b2, s2, t2, f_out,
                         (long)ld_fo, (int)E, tiles, tiles_per_wg, wgs, pr, nx);
    else
      hipLaunchKernelGGL((k_edge_mt_uv_mlp2_mean<false>), dim3(mt_grid), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv,
                         src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)npt, Wc4, b1, s1, t1, w2, b2, s2, t2, f_out,
                         (long)ld_fo, (int)E, tiles, tiles_per_wg, wgs, pr, nx);
    YL_LAUNCH_CHECK();
    return 0;
  }
  const unsigned grid = (unsigned)tiles + (unsigned)nx.s_tiles + (unsigned)pr.blocks;
  if (npt <= 16 && nx.Wp != nullptr)
    hipLaunchKernelGGL((k_edge_uv_mlp2_mean<1, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv,
                       src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)npt, Wc4, b1, s1, t1, w2, b2, s2, t2, f_out,
                       (long)ld_fo, (int)E, tiles, pr, nx);
  else if (npt <= 16)
    hipLaunchKernelGGL((k_edge_uv_mlp2_mean<1, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv,
                       src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)npt, Wc4, b1, s1, t1, w2, b2, s2, t2, f_out,
                       (long)ld_fo, (int)E, tiles, pr, nx);
  else
    hipLaunchKernelGGL((k_edge_uv_mlp2_mean<4, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv,
                       src_csr, dst_csr, attr_csr, row_ptr, (int)N, (int)npt, Wc4, b1, s1, t1, w2, b2, s2, t2, f_out,
                       (long)ld_fo, (int)E, tiles, pr, nx);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_edge_uv_mlp2_mean_eval_variant(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                                    const int32_t* dst_csr, const float* attr_csr,
                                                    const int32_t* row_ptr, int64_t N, int64_t E, const float* Wc4,
                                                    const float* b1, const float* s1, const float* t1, const float* W2,
                                                    const float* b2, const float* s2, const float* t2, int64_t C,
                                                    float* f_out, int64_t ld_fo, int variant, yolat_stream_t stream) {
  return yl_edge_uv_mlp2_mean_eval_impl(UV, ld_uv, src_csr, dst_csr, attr_csr, row_ptr, N, E, Wc4, b1, s1, t1, W2, b2, s2,
                                        t2, C, f_out, ld_fo, variant, nullptr, nullptr, nullptr, nullptr, stream);
}

// The node-tile kernel (YOLAT_EDGE_TILES) with `tiles_per_wg` consecutive tiles per workgroup: 1 is the one-tile kernel,
// 2 .. YOLAT_EDGE_MT_MAX select k_edge_mt_uv_mlp2_mean where the tiles hold <= 16 nodes (elsewhere the argument has no effect).
extern "C" int yolat_edge_uv_mlp2_mean_eval_mt(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                               const int32_t* dst_csr, const float* attr_csr, const int32_t* row_ptr,
                                               int64_t N, int64_t E, const float* Wc4, const float* b1, const float* s1,
                                               const float* t1, const float* W2, const float* b2, const float* s2,
                                               const float* t2, int64_t C, float* f_out, int64_t ld_fo, int tiles_per_wg,
                                               yolat_stream_t stream) {
  return yl_edge_uv_mlp2_mean_eval_impl(UV, ld_uv, src_csr, dst_csr, attr_csr, row_ptr, N, E, Wc4, b1, s1, t1, W2, b2, s2,
                                        t2, C, f_out, ld_fo, YOLAT_EDGE_TILES, nullptr, nullptr, nullptr, nullptr, stream,
                                        tiles_per_wg);
}

// yolat_edge_uv_mlp2_mean_eval_mt with the next layer's node side (EdgeNext, internal.hpp) in the same launch, as the eval
// forward's chain issues it: Wp [192 x 64 packed], bias [192] -> UV' [N, ld_uvn >= 128], root' [N, ld_root >= 64]; s_in
// (nullable: no node-branch tiles) . Wn^T, bn (nullable), sn, tn -> s_out.  *did_next = 1 when the launch carried it
// (tiles of <= 16 nodes).  For tests and tools, not part of the C ABI header.
extern "C" int yolat_debug_edge_uv_mlp2_mean_eval_next(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                                       const int32_t* dst_csr, const float* attr_csr, const int32_t* row_ptr,
                                                       int64_t N, int64_t E, const float* Wc4, const float* b1, const float* s1,
                                                       const float* t1, const float* W2, const float* b2, const float* s2,
                                                       const float* t2, int64_t C, float* f_out, int64_t ld_fo, int tiles_per_wg,
                                                       const float* Wp, const float* bias, float* UVn, int64_t ld_uvn,
                                                       float* root, int64_t ld_root, const float* s_in, int64_t ld_si,
                                                       const float* Wn, const float* bn, const float* sn, const float* tn,
                                                       float* s_out, int64_t ld_so, int* did_next, yolat_stream_t stream) {
  if (N <= 0 || !Wp || ld_uvn < 2 * C || ld_root < C || (s_in && ld_so < C)) return YOLAT_E_INVALID;
  EdgeNext nx{};
  nx.Wp = Wp; nx.bias = bias; nx.UV = UVn; nx.ld_uv = (long)ld_uvn; nx.root = root; nx.ld_root = (long)ld_root;
  nx.s_in = s_in; nx.ld_si = (long)ld_si; nx.Wn = Wn; nx.bn = bn; nx.sn = sn; nx.tn = tn; nx.s_out = s_out; nx.ld_so = (long)ld_so;
  nx.s_tiles = s_in ? (int)yl_cdiv(N, 64) : 0;
  return yl_edge_uv_mlp2_mean_eval_impl(UV, ld_uv, src_csr, dst_csr, attr_csr, row_ptr, N, E, Wc4, b1, s1, t1, W2, b2, s2,
                                        t2, C, f_out, ld_fo, YOLAT_EDGE_TILES, nullptr, nullptr, &nx, did_next, stream,
                                        tiles_per_wg);
}

extern "C" int yolat_edge_uv_mlp2_mean_eval(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                            const int32_t* dst_csr, const float* attr_csr,
                                            const int32_t* row_ptr, int64_t N, int64_t E, const float* Wc4,
                                            const float* b1, const float* s1, const float* t1, const float* W2,
                                            const float* b2, const float* s2, const float* t2, int64_t C,
                                            float* f_out, int64_t ld_fo, yolat_stream_t stream) {
  return yolat_edge_uv_mlp2_mean_eval_variant(UV, ld_uv, src_csr, dst_csr, attr_csr, row_ptr, N, E, Wc4, b1, s1, t1, W2,
                                              b2, s2, t2, C, f_out, ld_fo, YOLAT_EDGE_AUTO, stream);
}

extern "C" int yolat_edge_uv_mlp2_eval(const float* UV, int64_t ld_uv, const int32_t* src_csr,
                                       const int32_t* dst_csr, const float* attr_csr, int64_t E, const float* Wc4,
                                       const float* b1, const float* s1, const float* t1, const float* W2,
                                       const float* b2, const float* s2, const float* t2, int64_t C, float* H2,
                                       int64_t ldh, yolat_stream_t stream) {
  if (E < 0 || !UV || !Wc4 || !W2) return YOLAT_E_INVALID;
  if (C != 64) return YOLAT_E_UNSUPPORTED;
  if (E == 0) return 0;
  if (!src_csr || !dst_csr || !attr_csr || !H2 || E >= (1LL << 31) || ldh < C || ld_uv < 2 * C) return YOLAT_E_INVALID;
  if ((s1 == nullptr) != (t1 == nullptr) || (s2 == nullptr) != (t2 == nullptr)) return YOLAT_E_INVALID;
  if (ld_uv % 4 != 0 || !yl_aligned16(UV) || !yl_aligned16(attr_csr) || !yl_aligned16(Wc4) || (b1 && !yl_aligned16(b1)) ||
      (s1 && (!yl_aligned16(s1) || !yl_aligned16(t1))))
    return YOLAT_E_UNSUPPORTED;
  DenseOp w2 = yl_dense(W2, C, C, C);
  Epilogue ep;
  ep.bias = b2; ep.scale = s2; ep.shift = t2; ep.relu = 1;
  ep.Y = H2; ep.ldy = ldh; ep.accumulate = 0; ep.stats = nullptr; ep.seg = nullptr; ep.pool = nullptr; ep.ldpool = 0;
  hipLaunchKernelGGL(k_edge_uv_mlp2, dim3(yl_cdiv(E, 64)), dim3(256), 0, (hipStream_t)stream, UV, (long)ld_uv, src_csr,
                     dst_csr, attr_csr, Wc4, b1, s1, t1, w2, ep, (int)E);
  YL_LAUNCH_CHECK();
  return 0;
}
