// fx_w_movers.inc — the W-tile movers of the rows kernels, included as TEXT by k_fusion_rows_x6 (fusion_x6.hip),
// k_fusion_rows_f16x3 (fusion_f16x3.hip) and k_fusion_rows_rn (rownorm.hip): the one copy.  In scope: wparts[] (the
// problem's split weights [F, KD], 2-byte elements: 3 parts bf16 or 2 parts half), Ws (the two LDS buffers [parts][64][RS]),
// tid, F and the constants T, KD, CPR (16-byte chunks per row), RS (LDS row stride), NW (pieces per thread and tile);
// FX_W_CLAMP is 1 where F % 64 may be non-zero (rows past F - 1 re-read row F - 1), else 0.  It defines load_w(ct, rw):
// column tile ct into registers, in flight while the current tile's MFMAs run, and store_w(buf, rw): into LDS buffer buf.
// Text, not a template, for gemm_sk_tile.inc's reason: as members of a mover struct the same statements gave all three
// kernels other instructions — tools/kernel_isa_diff.py must say SAME for them.
  // W tile pieces: thread tid moves 16-byte piece (tid + T t) of the [parts][64][KD] tile; 64 * CPR is a multiple of
  // T, so the part (hi / mid / lo) of piece t is a compile-time constant
  constexpr int PER = 64 * CPR / T;                         // pieces per thread and part
  static_assert((64 * CPR) % T == 0, "part boundary inside a thread's pieces");
  const unsigned wr0 = (unsigned)tid / CPR, wk = ((unsigned)tid % CPR) * 8;   // row (of the first piece), k offset
  auto load_w = [&](int ct, fx_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const int part = t / PER;
      const unsigned r = wr0 + (unsigned)(t % PER) * (T / CPR);
#if FX_W_CLAMP
      rw[t] = *reinterpret_cast<const fx_u32x4*>(wparts[part] + (unsigned)yl_min(ct * 64 + (int)r, F - 1) * KD + wk);
#else
      rw[t] = *reinterpret_cast<const fx_u32x4*>(wparts[part] + (unsigned)(ct * 64 + (int)r) * KD + wk);
#endif
    }
  };
  auto store_w = [&](int buf, const fx_u32x4* rw) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      const int part = t / PER;
      const unsigned r = wr0 + (unsigned)(t % PER) * (T / CPR);
      *reinterpret_cast<fx_u32x4*>(&Ws[buf][part * 64 * RS + r * RS + wk]) = rw[t];
    }
  };
