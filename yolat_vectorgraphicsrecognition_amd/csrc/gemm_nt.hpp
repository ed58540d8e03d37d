// gemm_nt.hpp — the fp32 MFMA NT GEMM tile, its kernels and the node side of a factorised conv layer.
#pragma once
#include "epilogue.hpp"

// ------------------------------------------------------------------------------------------------
// NT GEMM:  Y[M,N] = epi( A[M,K] . B[N,K]^T )   — 256 threads, 2x2 waves, wave tile (BM/2)x(BN/2)
// built from 32x32x2 fp32 MFMAs.  LDS tiles As[BM][BK+1], Bs[BN][BK+1] (the +1 dword pad makes the
// per-lane column reads of the fragments conflict-free).  The global loads of the next K-tile are
// issued into registers before the MFMAs of the current one (software pipeline), so HBM/L2 latency
// hides under the 64-cycle fp32 MFMAs.
//   MFMA operand layout (cdna_hip_programming.md §3): A: lane l holds A[i=l&31][k=l>>5];
//   B: lane l holds B[k=l>>5][j=l&31].
// B_NFAST: the B loader is contiguous along n (transposed operands) -> map consecutive threads to
// consecutive n when staging.
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int BK, class AL, class BL, bool B_NFAST>
__device__ __forceinline__ void gemm_nt_tile(const AL& A, const BL& B, const Epilogue& ep, int M, int N, int K,
                                             int rt_, int ct_) {
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 32, TN = WN / 32;
  constexpr int LD = BK + 1;
  constexpr int KQ = BK / 4;
  constexpr int NA = (BM * KQ) / 256, NB = (BN * KQ) / 256;   // float4 loads per thread per tile
  static_assert((BM * KQ) % 256 == 0 && (BN * KQ) % 256 == 0, "tile/thread mismatch");
  // (at least the 4 x [32][YL_STAGE_LD] floats of the epilogue's store staging, which re-uses the operand tiles)
  constexpr int SMEM = (BM + BN) * LD > 4 * 32 * YL_STAGE_LD ? (BM + BN) * LD : 4 * 32 * YL_STAGE_LD;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  float* As = smem;
  float* Bs = smem + BM * LD;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int row0 = rt_ * BM, col0 = ct_ * BN;
  const bool fastA = A.vec != 0, fastB = B.vec != 0;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float ra[NA][4], rb[NB][4];
  auto fetch = [&](int k0) {
    const bool full = (k0 + BK <= K);           // wave-uniform
    if (full && fastA) {
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        const int i = tid + t * 256;
        A.template load4<true>(row0 + i / KQ, k0 + 4 * (i % KQ), ra[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        const int i = tid + t * 256;
        A.template load4<false>(row0 + i / KQ, k0 + 4 * (i % KQ), ra[t]);
      }
    }
    if (full && fastB) {
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        const int i = tid + t * 256;
        const int n = B_NFAST ? (i % BN) : (i / KQ);
        const int kq = B_NFAST ? (i / BN) : (i % KQ);
        B.template load4<true>(col0 + n, k0 + 4 * kq, rb[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        const int i = tid + t * 256;
        const int n = B_NFAST ? (i % BN) : (i / KQ);
        const int kq = B_NFAST ? (i / BN) : (i % KQ);
        B.template load4<false>(col0 + n, k0 + 4 * kq, rb[t]);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int t = 0; t < NA; ++t) {
      const int i = tid + t * 256;
      float* d = As + (i / KQ) * LD + 4 * (i % KQ);
      d[0] = ra[t][0]; d[1] = ra[t][1]; d[2] = ra[t][2]; d[3] = ra[t][3];
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int i = tid + t * 256;
      const int n = B_NFAST ? (i % BN) : (i / KQ);
      const int kq = B_NFAST ? (i / BN) : (i % KQ);
      float* d = Bs + n * LD + 4 * kq;
      d[0] = rb[t][0]; d[1] = rb[t][1]; d[2] = rb[t][2]; d[3] = rb[t][3];
    }
  };

  EpiPre pre[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      pre[i][j] = epi_prefetch(ep, row0 + wm * WM + i * 32, col0 + wn * WN + j * 32 + l31, M, N);
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    stage();
    __syncthreads();
    if (k0 + BK < K) fetch(k0 + BK);      // in flight while the MFMAs below run
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[(wm * WM + i * 32 + l31) * LD + kk + lhi];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[(wn * WN + j * 32 + l31) * LD + kk + lhi];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // spelled out with compile-time indices: the compiler refuses to unroll a loop around the (large) inlined
  // epilogue for TM*TN = 4, and a rolled loop indexes acc[][] dynamically = accumulators in scratch memory
  static_assert(TM <= 2 && TN <= 2, "epilogue expansion covers up to 2x2 sub-tiles");
#define YL_EPI(i, j)                                                                                              \
  if constexpr ((i) < TM && (j) < TN)                                                                             \
    wave_epilogue(acc[i][j], row0 + wm * WM + (i) * 32, col0 + wn * WN + (j) * 32 + l31, lhi, ep, M, N, pre[i][j], \
                  smem + wave * (32 * YL_STAGE_LD));
  YL_EPI(0, 0) YL_EPI(0, 1) YL_EPI(1, 0) YL_EPI(1, 1)
#undef YL_EPI
}

template <int BM, int BN, int BK, class AL, class BL, bool B_NFAST>
__global__ void __launch_bounds__(256) k_gemm_nt(AL A, BL B, Epilogue ep, int M, int N, int K) {
  int rt_, ct_;
  yl_xcd_tile(rt_, ct_);
  gemm_nt_tile<BM, BN, BK, AL, BL, B_NFAST>(A, B, ep, M, N, K, rt_, ct_);
}

// Two independent GEMMs with the same M, N <= BN and K in ONE launch (blockIdx.y picks the problem): the
// root Linear (+ fused CSR mean) and the node-branch Linear+BN+ReLU of a conv layer are 157 workgroups each
// at cfg 2 — separately they are two launch/drain latencies on a quarter-filled GPU.
template <int BM, int BN, int BK, class AL, class BL>
__global__ void __launch_bounds__(256) k_gemm_nt_pair(AL A0, BL B0, Epilogue e0, AL A1, BL B1, Epilogue e1,
                                                      int M, int N, int K) {
  if (blockIdx.y == 0) gemm_nt_tile<BM, BN, BK, AL, BL, false>(A0, B0, e0, M, N, K, blockIdx.x, 0);
  else gemm_nt_tile<BM, BN, BK, AL, BL, false>(A1, B1, e1, M, N, K, blockIdx.x, 0);
}

// Operands / epilogues of the node side of a factorised conv layer (built by yl_build_node_uv, dense.hip)
struct NodeUv {
  DenseOp af, wuv, wr, as, wn;
  Epilogue euv, er, en;
  int N, C, Cin;
};
// ------------------------------------------------------------------------------------------------
// Node side of the FIRST conv layer of a large graph as an output stream (launcher: dense.hip yl_node3_smallk).  K = in_channels = 5 raw Bezier features -> 256 outputs per node
// (UV [N, 128], root [N, 64], node branch [N, 64]; architecture3cc_rpn_gp_iter2.py:110-113 with torch_vertex.py:319-337
// factorised): with K <= 8 there is nothing for the matrix cores to do, the launch is a 100 - 200 MB output stream.  One
// wave owns 8 consecutive rows per step, lane = four consecutive output columns with their weights in registers (4 x K
// fma per row), 16-byte (fp32) / 8-byte (bf16) stores that cover whole cache lines.  Same epilogue arithmetic as wave_epilogue (bias, scale / shift, ReLU, bf16 = nearest even);
// the sum over k runs in ascending order.  Measured at N = 200 k (tools/exp/node3_bench.py): 39 us for the 205 MB of
// fp32 outputs = 5.3 TB/s, against 6.8 - 7.8 TB/s of a plain fill on this part (tools/exp/stream_bw.py) and 57 - 65 us
// for the 64x64 MFMA tiles of k_gemm_nt_node3 (one load -> LDS -> MFMA -> store chain per 16 KB of output; 80 - 90 us
// together with the CSR emission they were co-scheduled with).  With the stores switched off the kernel runs 22 us
// (its ~44 vector-ALU operations per row), with the FMAs switched off 45: the store stream is the bound.
// ------------------------------------------------------------------------------------------------
constexpr int N3_KMAX = 8, N3_ROWS = 32, N3_ITERS = 4;        // 4 waves x 8 consecutive rows per step, steps per workgroup
// WAVES waves per workgroup (8 consecutive rows per wave and step), ITERS steps: the 256-thread stream kernel is <4, 4>,
// the node-side workgroups of the one-launch graph preparation (graph.hip k_prep_small, 1024 threads) are <16, 1>
template <int WAVES = 4, int ITERS = N3_ITERS>
__device__ __forceinline__ void node3_smallk_body(const NodeUv& a, int vb) {
  constexpr int ROWS = 8 * WAVES;
  // ALL inputs of the workgroup's 128 rows are fetched up front into LDS (lane (row u = lane / 8, k = lane % 8) of the
  // row's wave; read back as two uniform-address 16-byte reads per row), so that the row loop holds no load: on this
  // ISA loads and stores share one in-order counter, and a load issued behind the previous step's stores made every
  // step wait for those stores' acknowledgements (51 -> 44 us).
  __shared__ __attribute__((aligned(16))) float xs[ITERS][WAVES][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, Cin = a.Cin, N = a.N;
  const int r0 = vb * (ROWS * ITERS), r1 = yl_min(r0 + ROWS * ITERS, N);
  const int c4 = 4 * lane;
  const int prob = c4 < 2 * C ? 0 : (c4 < 3 * C ? 1 : 2);
  const int col = prob == 0 ? c4 : (prob == 1 ? c4 - 2 * C : c4 - 3 * C);
  const int relu = prob == 0 ? a.euv.relu : (prob == 1 ? a.er.relu : a.en.relu);
  float* Y = prob == 0 ? a.euv.Y : (prob == 1 ? a.er.Y : a.en.Y);
  unsigned short* Yh = prob == 0 ? a.euv.Yh : (prob == 1 ? a.er.Yh : a.en.Yh);
  const long ldy = prob == 0 ? a.euv.ldy : (prob == 1 ? a.er.ldy : a.en.ldy);
  const int lu = lane >> 3, lk = lane & 7;
  float fa[ITERS], sa[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    // (clamped addresses + select, here and for the weights below: a load under a condition becomes a branch with
    // its own wait, and the kernel's start was a chain of ~30 such round trips)
    const long row = yl_min(r0 + ROWS * it + 8 * wave + lu, N - 1);
    const int kc = yl_min(lk, Cin - 1);
    const float f = a.af.p[row * a.af.ld + kc], g = a.as.p[row * a.as.ld + kc];
    fa[it] = lk < Cin ? f : 0.f;
    sa[it] = lk < Cin ? g : 0.f;
  }
  // the 256 weight rows (5 KB) and per-column constants: one row / one column per thread, through LDS.  (Every lane
  // fetching its own 4 x K weights straight from memory touched 64 different cache lines per load instruction, in
  // every one of 1563 workgroups: 44 -> 39 us.)
  __shared__ __attribute__((aligned(16))) float wl[256][N3_KMAX];
  __shared__ float cl[3][256];
  if (threadIdx.x < 256) {
    const int t = threadIdx.x;                              // virtual column t of [UV | root | node branch]
    const int tp = t < 2 * C ? 0 : (t < 3 * C ? 1 : 2);
    const int tc = tp == 0 ? t : (tp == 1 ? t - 2 * C : t - 3 * C);
    const float* __restrict__ twp = tp == 0 ? a.wuv.p : (tp == 1 ? a.wr.p : a.wn.p);
    const long tld = tp == 0 ? a.wuv.ld : (tp == 1 ? a.wr.ld : a.wn.ld);
    const float* tb = tp == 0 ? a.euv.bias : (tp == 1 ? a.er.bias : a.en.bias);
    const float* ts = tp == 0 ? a.euv.scale : (tp == 1 ? a.er.scale : a.en.scale);
    const float* th = tp == 0 ? a.euv.shift : (tp == 1 ? a.er.shift : a.en.shift);
    float wr_[N3_KMAX];
#pragma unroll
    for (int k = 0; k < N3_KMAX; ++k) wr_[k] = twp[(long)tc * tld + yl_min(k, Cin - 1)];
    const float vb_ = (tb ? tb : twp)[tb ? tc : 0], vs_ = (ts ? ts : twp)[ts ? tc : 0], vh_ = (ts ? th : twp)[ts ? tc : 0];
#pragma unroll
    for (int k = 0; k < N3_KMAX; ++k) wl[t][k] = k < Cin ? wr_[k] : 0.f;
    cl[0][t] = tb ? vb_ : 0.f;
    cl[1][t] = ts ? vs_ : 1.f;
    cl[2][t] = ts ? vh_ : 0.f;
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) { xs[it][wave][0][lane] = fa[it]; xs[it][wave][1][lane] = sa[it]; }
  __syncthreads();
  float w[4][N3_KMAX], b[4], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 w0 = *reinterpret_cast<const float4*>(&wl[c4 + j][0]), w1 = *reinterpret_cast<const float4*>(&wl[c4 + j][4]);
    w[j][0] = w0.x; w[j][1] = w0.y; w[j][2] = w0.z; w[j][3] = w0.w;
    w[j][4] = w1.x; w[j][5] = w1.y; w[j][6] = w1.z; w[j][7] = w1.w;
    b[j] = cl[0][c4 + j]; sc[j] = cl[1][c4 + j]; sh[j] = cl[2][c4 + j];
  }
  const float floor = relu ? 0.f : -INFINITY;
#pragma unroll 1
  for (int it = 0; it < ITERS; ++it) {
    const float* mine = xs[it][wave][prob == 2 ? 1 : 0];
    const int rb = r0 + ROWS * it + 8 * wave;
    if (rb >= r1) break;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float4 x0 = *reinterpret_cast<const float4*>(mine + 8 * u);
      const float4 x1 = *reinterpret_cast<const float4*>(mine + 8 * u + 4);
      const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < N3_KMAX; ++k) acc = fmaf(x[k], w[j][k], acc);
        v[j] = fmaxf(fmaf(acc + b[j], sc[j], sh[j]), floor);
      }
      const int row = rb + u;
      if (row < r1) {
        if (Yh != nullptr) {
          uint2 o;
          o.x = yl_pack_bf16(v[0], v[1]); o.y = yl_pack_bf16(v[2], v[3]);
          *reinterpret_cast<uint2*>(Yh + (long)row * ldy + col) = o;
        } else {
          *reinterpret_cast<float4*>(Y + (long)row * ldy + col) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

// tile y of row tile x: y = 0,1 -> UV halves, 2 -> root Linear, 3 -> node-branch Linear
template <int BK>
__device__ __forceinline__ void node_uv_tile(const NodeUv& a, int x, int y) {
  if (y < 2) gemm_nt_tile<64, 64, BK, DenseOp, DenseOp, false>(a.af, a.wuv, a.euv, a.N, 2 * a.C, a.Cin, x, y);
  else if (y == 2) gemm_nt_tile<64, 64, BK, DenseOp, DenseOp, false>(a.af, a.wr, a.er, a.N, a.C, a.Cin, x, 0);
  else gemm_nt_tile<64, 64, BK, DenseOp, DenseOp, false>(a.as, a.wn, a.en, a.N, a.C, a.Cin, x, 0);
}

// Node side of a factorised conv layer in one launch: blockIdx.y = 0,1 -> the two 64-column halves of
// UV = f_in.Wuv^T (N = 128 outputs), 2 -> root Linear, 3 -> node-branch Linear+BN+ReLU.
template <int BK>
__global__ void __launch_bounds__(256) k_gemm_nt_node3(NodeUv a) {
  node_uv_tile<BK>(a, blockIdx.x, blockIdx.y);
}
