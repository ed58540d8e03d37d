// act.hip — the leaky activations of torch_nn.py:9-20 (LeakyReLU(0.2), PReLU(num_parameters = 1)):
//   act(y) = y > 0 ? y : a * y,   the slope a read from DEVICE memory by every kernel (an in-place edit of a PReLU weight is
//   seen by the next launch and by a hipGraph replay).
// yolat_scale_shift_act, yolat_segment_act_max, yolat_fusion_pair_eval_act, yolat_pool_init_signed (eval), yolat_bn_act_bwd
// (training).  The activation-aware instantiation of the eval rows kernel is in fusion_x6.hip (yolat_fusion_pair_eval_x6_act).
// Nothing here assumes a >= 0: a PReLU slope may turn negative, the activation is then not monotone, so the per-proposal
// maximum is taken over ACTIVATED values and the backward decides by the sign of the recomputed BatchNorm output, never by
// the sign of a stored activation.
#include "base.hpp"

namespace {
__device__ __forceinline__ float yl_act(float y, float a) { return y > 0.f ? y : a * y; }      // NaN: a * NaN = NaN
// max that keeps a NaN once seen (torch's amax / scatter-max propagate it; fmaxf drops it)
__device__ __forceinline__ float yl_max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// Z = act(Y * scale + shift); scale == nullptr: Z = act(Y).  Z may be Y.
__global__ void __launch_bounds__(256) k_scale_shift_act(const float* Y, long ldy, long M, int C, const float* scale,
                                                         const float* shift, const float* slope, float* Z, long ldz) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (c >= C) return;
  const float a = *slope;
  const float sc = scale ? scale[c] : 1.f, sh = scale ? shift[c] : 0.f;
  for (long r = (long)blockIdx.y * 4 + (threadIdx.x >> 6); r < M; r += (long)gridDim.y * 4) {
    const float y = Y[r * ldy + c];
    Z[r * ldz + c] = yl_act(scale ? fmaf(y, sc, sh) : y, a);
  }
}

// out[p, c] = max over the rows of proposal p of act(Y[r, c]) (0 for a proposal without rows): one workgroup per
// (64 columns, proposal), 4 rows in flight, exact for signed values, no atomics — every element has one writer.
__global__ void __launch_bounds__(256) k_segment_act_max(const float* __restrict__ Y, long ldy, int N, int F,
                                                         const float* __restrict__ slope, const int* __restrict__ seg_ptr,
                                                         int P, float* out, long ldo) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const float a = *slope;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    int r0 = seg_ptr[p], r1 = seg_ptr[p + 1];
    r0 = r0 < 0 ? 0 : r0; r1 = r1 > N ? N : r1;            // (a malformed batch is flagged elsewhere: stay inside Y)
    float m = -INFINITY;
    if (c < F)
      for (int r = r0 + ty; r < r1; r += 4) m = yl_max_nan(m, yl_act(Y[(long)r * ldy + c], a));
    red[ty][cl] = m;
    __syncthreads();
    if (ty == 0 && c < F) {
      for (int t = 1; t < 4; ++t) m = yl_max_nan(m, red[t][cl]);
      out[(long)p * ldo + c] = r1 > r0 ? m : 0.f;
    }
    __syncthreads();
  }
}

// start values of the signed pooling (segmax.hpp fx_signed_max): -inf for a proposal with rows, 0 for one without
__global__ void __launch_bounds__(256) k_pool_init_signed(const int* __restrict__ seg_ptr, int P, int F, float* pool,
                                                          long ldpool) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= F) return;
  for (int p = blockIdx.y; p < P; p += gridDim.y)
    pool[(long)p * ldpool + c] = seg_ptr[p + 1] > seg_ptr[p] ? -INFINITY : 0.f;
}

// ---- backward of Z = act(BN_train(Y)) ------------------------------------------------------------------------------
// with y' = scale * Y + shift (recomputed), g' = y' > 0 ? g : a * g:
//   per 256-row block and column: (sum g', sum g' * xhat, sum_{y' <= 0} g * y')            k_bn_act_bwd_partial
//   fp64 sums over the blocks in block order -> dgamma, dbeta, coef, per-column dalpha     k_bn_act_bwd_finalize
//   dalpha = sum over the columns in a fixed tree                                           k_dalpha_reduce
//   dY = scale * (g' - c1 - xhat * c2)                                                      k_bn_act_bwd_apply
// Every sum has a fixed order: two runs are bit-identical.
constexpr int BNA_ROWS = 256;
__global__ void __launch_bounds__(256) k_bn_act_bwd_partial(const float* dZ, long lddz, const float* Y, long ldy, long M, int C,
                                                            const float* mean, const float* invstd, const float* scale,
                                                            const float* shift, const float* slope, float* part) {
  __shared__ float red[3][4][64];
  const int cl = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const long r0 = (long)blockIdx.y * BNA_ROWS;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < C) {
    const float a = *slope;
    const float mu = mean[c], is = invstd[c], sc = scale[c], sh = shift[c];
    long r1 = r0 + BNA_ROWS;
    if (r1 > M) r1 = M;
    for (long r = r0 + ty; r < r1; r += 4) {
      const float y = Y[r * ldy + c];
      float g = dZ[r * lddz + c];
      const float yb = fmaf(y, sc, sh);
      if (!(yb > 0.f)) { s3 += g * yb; g *= a; }
      s1 += g;
      s2 += g * ((y - mu) * is);
    }
  }
  red[0][ty][cl] = s1; red[1][ty][cl] = s2; red[2][ty][cl] = s3;
  __syncthreads();
  if (ty == 0 && c < C) {
    for (int t = 1; t < 4; ++t) { s1 += red[0][t][cl]; s2 += red[1][t][cl]; s3 += red[2][t][cl]; }
    float* o = part + ((long)blockIdx.y * C + c) * 3;
    o[0] = s1; o[1] = s2; o[2] = s3;
  }
}

__global__ void __launch_bounds__(64) k_bn_act_bwd_finalize(const float* part, long nb, long M, int C, float* dgamma,
                                                            float* dbeta, int accumulate, float* coef, float* col_da) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0, d = 0.0;
  for (long i = 0; i < nb; ++i) {
    const float* t = part + (i * C + c) * 3;
    a += (double)t[0]; b += (double)t[1]; d += (double)t[2];
  }
  float dg = (float)b, dbt = (float)a;
  if (accumulate) { dg += dgamma[c]; dbt += dbeta[c]; }
  dgamma[c] = dg; dbeta[c] = dbt;
  coef[c] = (float)(a / (double)M);
  coef[C + c] = (float)(b / (double)M);
  col_da[c] = (float)d;
}

__global__ void __launch_bounds__(256) k_dalpha_reduce(const float* col_da, int C, float* dalpha, int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) s += (double)col_da[c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dalpha = (float)red[0] + (accumulate ? *dalpha : 0.f);
}

__global__ void __launch_bounds__(256) k_bn_act_bwd_apply(const float* dZ, long lddz, const float* Y, long ldy, long M, int C,
                                                          const float* mean, const float* invstd, const float* scale,
                                                          const float* shift, const float* slope, const float* coef,
                                                          float* dY, long lddy) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (c >= C) return;
  const float a = *slope;
  const float mu = mean[c], is = invstd[c], sc = scale[c], sh = shift[c];
  const float c1 = coef[c], c2 = coef[C + c];
  for (long r = (long)blockIdx.y * 4 + (threadIdx.x >> 6); r < M; r += (long)gridDim.y * 4) {
    const float y = Y[r * ldy + c];
    float g = dZ[r * lddz + c];
    if (!(fmaf(y, sc, sh) > 0.f)) g *= a;
    const float xh = (y - mu) * is;
    dY[r * lddy + c] = sc * (g - c1 - xh * c2);
  }
}
}  // namespace

extern "C" int yolat_scale_shift_act(const float* Y, int64_t ldy, int64_t M, int64_t C, const float* scale,
                                     const float* shift, const float* slope, float* Z, int64_t ldz,
                                     yolat_stream_t stream) {
  if (M < 0 || C <= 0 || !slope || (scale != nullptr && !shift) || (M > 0 && (!Y || !Z))) return YOLAT_E_INVALID;
  if (M == 0) return 0;
  int gy = yl_cdiv(M, 4);
  if (gy > 2048) gy = 2048;
  hipLaunchKernelGGL(k_scale_shift_act, dim3(yl_cdiv(C, 64), gy), dim3(256), 0, (hipStream_t)stream, Y, (long)ldy, (long)M,
                     (int)C, scale, shift, slope, Z, (long)ldz);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_segment_act_max(const float* Y, int64_t ldy, int64_t N, int64_t F, const float* slope,
                                     const int32_t* seg_ptr, int64_t P, float* out, int64_t ldo, yolat_stream_t stream) {
  if (N < 0 || F <= 0 || P <= 0 || (N > 0 && !Y) || !slope || !seg_ptr || !out) return YOLAT_E_INVALID;
  const int gy = P > 32768 ? 32768 : (int)P;
  hipLaunchKernelGGL(k_segment_act_max, dim3(yl_cdiv(F, 64), gy), dim3(256), 0, (hipStream_t)stream, Y, (long)ldy, (int)N,
                     (int)F, slope, seg_ptr, (int)P, out, (long)ldo);
  YL_LAUNCH_CHECK();
  return 0;
}

extern "C" int yolat_pool_init_signed(const int32_t* seg_ptr, int64_t P, int64_t F, float* pool, int64_t ldpool,
                                      yolat_stream_t stream) {
  if (P <= 0 || F <= 0 || !seg_ptr || !pool || ldpool < F) return YOLAT_E_INVALID;
  const int gy = P > 16384 ? 16384 : (int)P;
  hipLaunchKernelGGL(k_pool_init_signed, dim3(yl_cdiv(F, 256), gy), dim3(256), 0, (hipStream_t)stream, seg_ptr, (int)P,
                     (int)F, pool, (long)ldpool);
  YL_LAUNCH_CHECK();
  return 0;
}

// columns of the fusion block computed per pass: the [N, chunk] BatchNorm output is the only scratch, kept <= 64 MiB
static long act_chunk_cols(long N, long F) {
  long fc = ((16L << 20) / (N > 0 ? N : 1)) / 64 * 64;
  if (fc < 64) fc = 64;
  return fc < F ? fc : F;
}

extern "C" size_t yolat_fusion_pair_eval_act_work_elems(int64_t N, int64_t F) {
  if (N <= 0 || F <= 0) return 0;
  return (size_t)N * (size_t)act_chunk_cols(N, F);
}

extern "C" int yolat_fusion_pair_eval_act(const float* A, int64_t lda, int64_t N, int64_t D, const float* Wf, const float* bf,
                                          const float* sf, const float* tf, int64_t F, const float* slope_f,
                                          const int32_t* seg_ptr, float* pool, int64_t ldpool, const float* S, int64_t lds,
                                          int64_t P, const float* Wfs, const float* bfs, const float* sfs, const float* tfs,
                                          const float* slope_s, float* Ys, int64_t ldys, float* work,
                                          yolat_stream_t stream) {
  if (N <= 0 || D <= 0 || F <= 0 || P <= 0 || !A || !Wf || !sf || !tf || !slope_f || !seg_ptr || !pool || !work)
    return YOLAT_E_INVALID;
  const long fc = act_chunk_cols(N, F);
  for (long c0 = 0; c0 < F; c0 += fc) {
    const long w = F - c0 < fc ? F - c0 : fc;
    // the BatchNorm output of columns [c0, c0 + w) for every node, then activation + per-proposal maximum
    YL_TRY(yolat_linear_fwd(A, lda, N, D, nullptr, nullptr, 0, Wf + c0 * D, D, bf ? bf + c0 : nullptr, w, sf + c0, tf + c0, 0,
                            work, w, 0, nullptr, stream));
    YL_TRY(yolat_segment_act_max(work, w, N, w, slope_f, seg_ptr, P, pool + c0, ldpool, stream));
  }
  if (S != nullptr) {
    if (!Wfs || !sfs || !tfs || !slope_s || !Ys) return YOLAT_E_INVALID;
    YL_TRY(yolat_linear_fwd(S, lds, P, D, nullptr, nullptr, 0, Wfs, D, bfs, F, sfs, tfs, 0, Ys, ldys, 0, nullptr, stream));
    YL_TRY(yolat_scale_shift_act(Ys, ldys, P, F, nullptr, nullptr, slope_s, Ys, ldys, stream));
  }
  return 0;
}

extern "C" size_t yolat_bn_act_bwd_work_elems(int64_t M, int64_t C) {
  return (size_t)(3 * (long)yl_cdiv(M, BNA_ROWS) * C + 3 * C);
}

extern "C" int yolat_bn_act_bwd(const float* dZ, int64_t lddz, const float* Y, int64_t ldy, int64_t M, int64_t C,
                                const float* save_mean, const float* save_invstd, const float* scale, const float* shift,
                                const float* slope, float* dgamma, float* dbeta, float* dslope, int accumulate, float* dY,
                                int64_t lddy, float* work, yolat_stream_t stream) {
  if (M <= 0 || C <= 0 || !dZ || !Y || !save_mean || !save_invstd || !scale || !shift || !slope || !dgamma || !dbeta ||
      !dY || !work)
    return YOLAT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const long nb = yl_cdiv(M, BNA_ROWS);
  float* part = work;
  float* coef = work + 3 * nb * C;
  float* col_da = coef + 2 * C;
  hipLaunchKernelGGL(k_bn_act_bwd_partial, dim3(yl_cdiv(C, 64), (unsigned)nb), dim3(256), 0, st, dZ, (long)lddz, Y, (long)ldy,
                     (long)M, (int)C, save_mean, save_invstd, scale, shift, slope, part);
  YL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bn_act_bwd_finalize, dim3(yl_cdiv(C, 64)), dim3(64), 0, st, part, nb, (long)M, (int)C, dgamma, dbeta,
                     accumulate, coef, col_da);
  YL_LAUNCH_CHECK();
  if (dslope != nullptr) {
    hipLaunchKernelGGL(k_dalpha_reduce, dim3(1), dim3(256), 0, st, col_da, (int)C, dslope, accumulate);
    YL_LAUNCH_CHECK();
  }
  int gy = yl_cdiv(M, 4);
  if (gy > 2048) gy = 2048;
  hipLaunchKernelGGL(k_bn_act_bwd_apply, dim3(yl_cdiv(C, 64), gy), dim3(256), 0, st, dZ, (long)lddz, Y, (long)ldy, (long)M,
                     (int)C, save_mean, save_invstd, scale, shift, slope, coef, dY, (long)lddy);
  YL_LAUNCH_CHECK();
  return 0;
}
