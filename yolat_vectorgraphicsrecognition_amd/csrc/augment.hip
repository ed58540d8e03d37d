// augment.hip — the training augmentation of the reference's dataset (SESYDFloorPlan.random_transfer,
// Datasets/graph_dict3.py:283-298, with __transform__ :236-258) and the proposal boxes it rebuilds afterwards
// (update_bbox, :934-959), applied IN PLACE to a collated batch that is already on the device: one launch per batch.
//
// Per graph b the host draws (augment.draw_params) scale, angle, translation and the two flips of `pos` and hands over
//   params[b] = { cos(angle), sin(angle), scale, tx, ty, flip_x, flip_y, 0 }          (8 doubles, flips 0.0 / 1.0)
// — the kernel calls no trigonometry.  A node of graph b moves, in float64 and in the reference's operation order
// (subtract the centre, flip, rotate, add the centre, add the translation, scale; every product and every sum rounded on
// its own: contraction is off, so the numpy host path augment.augment_item computes the same bits), is rounded ONCE to
// fp32 and written to pos and to the two position columns of x.  The box of a proposal is the min / max of its nodes'
// ROUNDED coordinates (rounding is monotone: the same as rounding the float64 min / max, which is what the reference's
// float64 update_bbox followed by torch.tensor(..., float32) gives).
//
// Lane mapping.  Proposals of this domain hold 4 - 40 nodes (25 at the fixed-size configurations): a group of AUG_G = 16
// lanes owns one proposal and walks its node range 16 nodes at a time — 1.9 steps per proposal on average at 4 - 40 nodes,
// 2 at 25, 70 - 78 % of the lanes busy — then reduces the four extremes with four xor-shuffles inside the group and lane 0
// stores the row (16 bytes).  Consecutive groups own consecutive proposals = consecutive node ranges, so a wave's loads
// and stores cover one contiguous stretch of pos.  A proposal of 1 node reduces over 15 neutral lanes; a proposal of
// more than 1024 nodes is just a longer walk.  No atomics.  Traffic per batch: 8 N + 4 P bytes read (pos, the
// segment pointers), 16 N + 16 P written (pos, the two columns of x, bbox).
#include "base.hpp"

constexpr int AUG_G = 16;                    // lanes per proposal
constexpr int AUG_THREADS = 256;
constexpr int AUG_PER_WG = AUG_THREADS / AUG_G;

__device__ __forceinline__ long aug_clamp(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the graph of proposal p: the last b in [0, B) with prop[b] <= p < prop[b + 1]; B when no graph holds it
// (prop: entries already clamped to [0, P], in LDS)
__device__ __forceinline__ int aug_graph_of_lds(const int* prop, int B, int p) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prop[mid] <= p) lo = mid; else hi = mid;
  }
  return (p >= prop[lo] && p < prop[lo + 1]) ? lo : B;
}
__device__ __forceinline__ int aug_graph_of(const int64_t* __restrict__ prop_ptr, int B, long P, long p) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (aug_clamp(prop_ptr[mid], P) <= p) lo = mid; else hi = mid;
  }
  return (p >= aug_clamp(prop_ptr[lo], P) && p < aug_clamp(prop_ptr[lo + 1], P)) ? lo : B;
}

// every product and sum of the transform is rounded on its own (the host path's numpy does the same): no fma
#pragma clang fp contract(off)

// At the batch sizes of this domain (2 - 4 MB of traffic) the launch is a few microseconds long and what it waits for is
// its chain of DEPENDENT loads, not bandwidth.  So: the segment pointers and the group's first positions are requested
// before anything else (their addresses need no graph), and the per-graph proposal offsets go through LDS once per
// workgroup (STAGED: B + 1 <= 256; one coalesced load) so that the bisection for the proposal's graph costs LDS reads,
// not log2(B) round trips to L2.  The chain is then two loads deep: prop_ptr -> params, beside seg_ptr -> pos.
template <bool STAGED>
static __global__ void __launch_bounds__(AUG_THREADS) k_augment_batch(
    float* __restrict__ pos, float* __restrict__ x, long ldx, int col_x, int col_y, const int* __restrict__ seg_ptr,
    const int64_t* __restrict__ prop_ptr, float* __restrict__ bbox, const double* __restrict__ params, int N, int P, int B) {
  __shared__ int s_prop[AUG_THREADS];
  const int lg = threadIdx.x & (AUG_G - 1);
  const int p = blockIdx.x * AUG_PER_WG + (threadIdx.x / AUG_G);
  // (no early return: the barrier and the shuffles below want every wave whole; a group without a proposal walks an
  // empty range)
  const int pc = yl_min(p, P - 1);
  const int s0 = seg_ptr[pc], s1 = seg_ptr[pc + 1];       // unconditional (a load under a condition waits on its own)
  const int n0 = (int)aug_clamp(s0, N);
  int n1 = (int)aug_clamp(s1, N);
  int n = n0 + lg;
  float2 v = *reinterpret_cast<const float2*>(pos + 2 * (long)yl_min(n, N - 1));     // speculative: a valid address
  int b;
  if (STAGED) {
    s_prop[threadIdx.x] = (int)aug_clamp(prop_ptr[yl_min((int)threadIdx.x, B)], P);
    __syncthreads();
    b = aug_graph_of_lds(s_prop, B, pc);
  } else {
    b = aug_graph_of(prop_ptr, B, P, pc);
  }
  if (b >= B || p >= P) n1 = n0;                   // a proposal of no graph stays as it is; a group past P has none
  const double* q = params + 8 * (long)yl_min(b, B - 1);
  const double c = q[0], s = q[1], scale = q[2], tx = q[3], ty = q[4];
  const bool fx = q[5] != 0.0, fy = q[6] != 0.0;
  const double ns = -s;
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  while (n < n1) {
    double px = (double)v.x - 0.5, py = (double)v.y - 0.5;               // pos -= center                   (:249)
    px = fx ? -px : px;                                                  // the two flips                   (:250-253)
    py = fy ? -py : py;
    const double a0 = px * c, a1 = py * ns, b0 = px * s, b1 = py * c;    // pos @ [[cos, sin], [-sin, cos]] (:254)
    double rx = a0 + a1, ry = b0 + b1;
    rx = rx + 0.5; ry = ry + 0.5;                                        // pos += center                   (:255)
    rx = rx + tx; ry = ry + ty;                                          // pos += translate                (:256)
    const double c0 = rx * scale, c1 = ry * 0.0, d0 = rx * 0.0, d1 = ry * scale;   // pos @ diag(scale)     (:257)
    const float ox = (float)(c0 + c1), oy = (float)(d0 + d1);            // the one rounding to fp32
    const int nn = n + AUG_G;
    if (nn < n1) v = *reinterpret_cast<const float2*>(pos + 2 * (long)nn);         // the next step's, before the stores
    *reinterpret_cast<float2*>(pos + 2 * (long)n) = make_float2(ox, oy);
    float* xr = x + (long)n * ldx;
    xr[col_x] = ox;
    xr[col_y] = oy;
    lo_x = fminf(lo_x, ox); hi_x = fmaxf(hi_x, ox);
    lo_y = fminf(lo_y, oy); hi_y = fmaxf(hi_y, oy);
    n = nn;
  }
#pragma unroll
  for (int m = AUG_G / 2; m >= 1; m >>= 1) {
    lo_x = fminf(lo_x, __shfl_xor(lo_x, m)); hi_x = fmaxf(hi_x, __shfl_xor(hi_x, m));
    lo_y = fminf(lo_y, __shfl_xor(lo_y, m)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, m));
  }
  // a proposal without a node keeps its row (update_bbox would emit no row for it)
  if (lg == 0 && n1 > n0) *reinterpret_cast<float4*>(bbox + 4 * (long)p) = make_float4(lo_x, lo_y, hi_x, hi_y);
}

extern "C" int yolat_augment_batch(float* pos, float* x, int64_t ldx, int64_t col_x, int64_t col_y,
                                   const int32_t* seg_ptr, const int64_t* prop_ptr, float* bbox, const double* params,
                                   int64_t N, int64_t P, int64_t B, yolat_stream_t stream) {
  if (N < 0 || P < 0 || B < 0 || N >= (1LL << 31) - 1 || P >= (1LL << 31) - AUG_PER_WG || B >= (1LL << 31) - 1)
    return YOLAT_E_INVALID;
  if (N == 0 || P == 0 || B == 0) return 0;
  if (!pos || !x || !seg_ptr || !prop_ptr || !bbox || !params) return YOLAT_E_INVALID;
  if (col_x < 0 || col_y < 0 || col_x == col_y || col_x >= ldx || col_y >= ldx) return YOLAT_E_INVALID;
  if ((((uintptr_t)pos) & 7) != 0 || !yl_aligned16(bbox) || (((uintptr_t)params) & 7) != 0) return YOLAT_E_INVALID;
  const dim3 grid(yl_cdiv(P, AUG_PER_WG)), block(AUG_THREADS);
  if (B + 1 <= AUG_THREADS)
    hipLaunchKernelGGL(k_augment_batch<true>, grid, block, 0, (hipStream_t)stream, pos, x, (long)ldx, (int)col_x,
                       (int)col_y, seg_ptr, prop_ptr, bbox, params, (int)N, (int)P, (int)B);
  else
    hipLaunchKernelGGL(k_augment_batch<false>, grid, block, 0, (hipStream_t)stream, pos, x, (long)ldx, (int)col_x,
                       (int)col_y, seg_ptr, prop_ptr, bbox, params, (int)N, (int)P, (int)B);
  YL_LAUNCH_CHECK();
  return 0;
}
