// gemm_sk_tile.inc — the body of k_gemm_nt_sk (gemm_sk.hpp), included as TEXT by the kernels that run it: in scope are
// A, B (operand layouts AL / BL with load4), ep, M, N, K and the constant B_NFAST; YL_SK_TAIL is 0 or 1.
//   YL_SK_TAIL 0   k_gemm_nt_sk itself: the tile leaves through wave_epilogue.
//   YL_SK_TAIL 1   k_cls_tail (cls_tail.hip), `tail` in scope: wave 0's finished tile goes to tail.tile() instead of the
//                  store, and every wave ends in tail.finish().
// Text, not a template: with the body behind a __device__ function (by value, by reference, LDS inside or outside) every
// k_gemm_nt_sk instance came out with another register allocation — tools/kernel_isa_diff.py must say SAME for them.
  constexpr int BT = 32, BK = 128, LD = BK + 1;
  __shared__ float smem[2 * BT * LD];
  float* As = smem;
  float* Bs = smem + BT * LD;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, lhi = lane >> 5;
  int rt_, ct_;
  yl_xcd_tile(rt_, ct_);
  const int row0 = rt_ * BT, col0 = ct_ * BT;
  const bool fastA = A.vec != 0, fastB = B.vec != 0;
  // Staging map: float4 slot i (0..1023) -> (row, kq).  32 consecutive lanes cover a 4-row x 8-kq patch:
  // each row gets a full 128-B line from global, and with LD = 129 the ds_write_b32 banks
  // (row + 4*kq + j) mod 32 of a 32-lane group are all distinct.  (The naive row = i/32, kq = i%32 map
  // is a 4-way bank conflict on every write and made this kernel LDS-write-bound.)
  auto map_r = [](int i) { return 4 * ((i >> 5) & 7) + ((i & 31) >> 3); };
  auto map_q = [](int i) { return 8 * (i >> 8) + (i & 7); };
  const EpiPre pre = epi_prefetch(ep, row0, col0 + l31, M, N);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // Two register sets = two K-chunks in flight: with ~1 workgroup per CU (P is a few hundred rows)
  // there is no other wave to hide the L2/MALL latency of the 4.7 MB classifier weight behind.
  float ra0[4][4], rb0[4][4], ra1[4][4], rb1[4][4];
  auto fetch = [&](int k0, float (&ra)[4][4], float (&rb)[4][4]) {
    const bool full = (k0 + BK <= K);
    if (full && fastA) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + t * 256;
        A.template load4<true>(row0 + map_r(i), k0 + 4 * map_q(i), ra[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + t * 256;
        A.template load4<false>(row0 + map_r(i), k0 + 4 * map_q(i), ra[t]);
      }
    }
    if (full && fastB) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + t * 256;
        const int n = B_NFAST ? (i % BT) : map_r(i);
        const int kq = B_NFAST ? (i / BT) : map_q(i);
        B.template load4<true>(col0 + n, k0 + 4 * kq, rb[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + t * 256;
        const int n = B_NFAST ? (i % BT) : map_r(i);
        const int kq = B_NFAST ? (i / BT) : map_q(i);
        B.template load4<false>(col0 + n, k0 + 4 * kq, rb[t]);
      }
    }
  };
  auto stage = [&](float (&ra)[4][4], float (&rb)[4][4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = tid + t * 256;
      float* d = As + map_r(i) * LD + 4 * map_q(i);
      d[0] = ra[t][0]; d[1] = ra[t][1]; d[2] = ra[t][2]; d[3] = ra[t][3];
      const int n = B_NFAST ? (i % BT) : map_r(i);
      const int kq = B_NFAST ? (i / BT) : map_q(i);
      float* e = Bs + n * LD + 4 * kq;
      e[0] = rb[t][0]; e[1] = rb[t][1]; e[2] = rb[t][2]; e[3] = rb[t][3];
    }
  };
  auto compute = [&]() {
    const int kb = wave * 32;
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) {
      const float a = As[l31 * LD + kb + kk + lhi];
      const float b = Bs[l31 * LD + kb + kk + lhi];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  };

  fetch(0, ra0, rb0);
  if (BK < K) fetch(BK, ra1, rb1);
  for (int k0 = 0; k0 < K; k0 += 2 * BK) {
    stage(ra0, rb0);
    __syncthreads();
    if (k0 + 2 * BK < K) fetch(k0 + 2 * BK, ra0, rb0);
    compute();
    __syncthreads();
    if (k0 + BK >= K) break;
    stage(ra1, rb1);
    __syncthreads();
    if (k0 + 3 * BK < K) fetch(k0 + 3 * BK, ra1, rb1);
    compute();
    __syncthreads();
  }
#if YL_SK_TAIL
  // the tail's own operands: in flight under the reduction and the epilogue.  (Fetched at the kernel's start they are five
  // registers on top of the loop's peak, 172 -> 180; fetched under the last chunk's MFMAs the loop still peaks at 180; here
  // both register sets are dead and the kernel holds k_gemm_nt_sk's 172.)
  const auto tpre = tail.prefetch(col0, tid);
#endif
  // fixed-order reduction of the 4 K-partials: waves 1..3 park theirs in LDS, wave 0 adds 1,2,3
  float* red = smem;   // [3][16][64]
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += red[(w * 16 + r) * 64 + lane];
#if YL_SK_TAIL
    tail.tile(acc, row0, col0 + l31, lhi, ep, M, N, pre, smem);
  }
  tail.finish(tpre, rt_, ct_, (int)gridDim.y, M, smem, tid);
#else
    wave_epilogue(acc, row0, col0 + l31, lhi, ep, M, N, pre);
  }
#endif
