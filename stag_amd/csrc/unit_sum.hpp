// unit_sum.hpp — what the plan-order sum kernels share: agg_half.hip (8 channels a lane) and agg_w1.hip (4).
//
// A launch walks the plan's units in plan order (one team of LPE lanes per unit; no plan: one unit per row).  A team
// sums its unit in blocks of edges: a block's terms are summed from zero and folded into the unit's sum in order,
// Kahan-compensated once the unit is longer than kKahanMinLen (AggTeam::fold_into's rule).  A segment of a long row
// leaves its fp32 partial in the plan's workspace; a second small launch (one workgroup per long row and channel tile)
// adds every long row's partials and applies the row scale.  No atomics, no arrival counters: two launches with the
// same inputs give the same bits.
// The argument struct A is HalfArgs or W1Args: the fields used here have the same names in both.
#pragma once
#include "agg_kernel.hpp"   // load4 / store4, kKahanMinLen, kCombineGroup (read-only helpers)
#include "entry_args.hpp"   // lanes_for

namespace stag {

// the unit a team serves (plan order; no plan: unit i = row i); false past the end
template <int LPE, class A>
__device__ __forceinline__ bool unit_of(const A& a, int& row, int& start, int& len, int& slot) {
  const int64_t rec = (int64_t)blockIdx.x * (256 / LPE) + threadIdx.x / LPE;
  if (rec >= a.n_units) return false;
  if (a.units) {
    const int4 q = *reinterpret_cast<const int4*>(a.units + rec);
    slot = q.w;
    row = slot >= 0 ? a.long_rows[q.x] : q.x;
    start = q.y;
    len = q.z;
  } else {
    row = (int)rec;
    start = a.indptr[row];
    len = a.indptr[row + 1] - start;
    slot = -1;
  }
  return true;
}

// dst_scale[v], then the mean's reciprocal
template <class A>
__device__ __forceinline__ float row_scale(const A& a, int v, int deg) {
  float dv = a.dst_scale ? a.dst_scale[v] : 1.0f;
  if (a.mean) dv *= __builtin_amdgcn_rcpf((float)(deg > 1 ? deg : 1));
  return dv;
}

// a block sum into the unit's sum: plain, or compensated when the unit is longer than kKahanMinLen
template <int N>
__device__ __forceinline__ void fold_block(bool kahan, const float (&t)[N], float (&acc)[N], float (&comp)[N]) {
  if (kahan) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const float y = t[q] - comp[q];
      const float n = acc[q] + y;
      comp[q] = (n - acc[q]) - y;
      acc[q] = n;
    }
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] += t[q];
  }
}

// a lane's N consecutive channels from k0 on, 4 at a time
template <int N>
__device__ __forceinline__ void store_n(float* p, int k0, int D, bool vec, const float (&v)[N]) {
#pragma unroll
  for (int h = 0; h < N; h += 4) {
    const float q[4] = {v[h], v[h + 1], v[h + 2], v[h + 3]};
    store4(p, k0 + h, D, vec, q);
  }
}

// The merge of a long row's partials, CPL channels per lane: the body of agg_w1_merge_kernel (CPL = 4); agg_half_merge_kernel
// is this at CPL = 8 written out (agg_half.hip says why).
// One workgroup per long row (a hub row has hundreds of segments: one team adding them one after the other is a chain
// of dependent loads — 39 us for the 13,000-edge hub of the arxiv-shaped graph).  The two-level form of two_level_sum
// (agg_kernel.hpp): Kahan sums of GROUPS of kCombineGroup partials in segment order, one group per team and round,
// then team 0 folds the group sums in group order — a group's Kahan residual joins the second level's compensation.
// Groups are cut by segment index alone, so the arithmetic does not depend on the teams per workgroup (the row's
// width), only on the row's segments.
template <int CPL, int LPE, class A>
__device__ __forceinline__ void seg_merge(const A& a) {
  constexpr int T = 256 / LPE, kAhead = 8;
  __shared__ float part[T][2][LPE * CPL];        // a round's group sums and what they still owe (2 CPL KB)
  const int r = blockIdx.x, team = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const int k0 = CPL * (blockIdx.y * LPE + lane);
  const bool live = k0 < a.D;                    // (no early return: the workgroup meets at barriers)
  const int row = a.long_rows[r];
  const int s0 = a.long_seg_ptr[r], s1 = a.long_seg_ptr[r + 1];
  const bool vec = a.ovec != 0;
  float sum[CPL], comp[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) sum[q] = comp[q] = 0.f;
  for (int g0 = s0; g0 < s1; g0 += kCombineGroup * T) {   // uniform over the workgroup
    const int gs = g0 + team * kCombineGroup;
    if (live && gs < s1) {
      const int ge = min(gs + kCombineGroup, s1);
      float gsum[CPL], gres[CPL];
#pragma unroll
      for (int q = 0; q < CPL; ++q) gsum[q] = gres[q] = 0.f;
      for (int s = gs; s < ge; s += kAhead) {
        float t[kAhead][CPL];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
          if (s + j < ge) {
#pragma unroll
            for (int h = 0; h < CPL; h += 4)
              load4(a.ws + (int64_t)(s + j) * a.D, k0 + h, a.D, vec, reinterpret_cast<float (&)[4]>(t[j][h]));
          }
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j)
          if (s + j < ge) fold_block(true, t[j], gsum, gres);
      }
#pragma unroll
      for (int q = 0; q < CPL; ++q) { part[team][0][lane * CPL + q] = gsum[q]; part[team][1][lane * CPL + q] = gres[q]; }
    }
    __syncthreads();
    if (team == 0 && live) {
      for (int j = 0; j < T && g0 + j * kCombineGroup < s1; ++j) {
        float g[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          g[q] = part[j][0][lane * CPL + q];
          comp[q] += part[j][1][lane * CPL + q];           // true group sum = its sum - its residual
        }
        fold_block(true, g, sum, comp);
      }
    }
    __syncthreads();                                       // the next round overwrites the group sums
  }
  if (team != 0 || !live) return;
  const float dv = row_scale(a, row, a.indptr[row + 1] - a.indptr[row]);
#pragma unroll
  for (int q = 0; q < CPL; ++q) sum[q] = (sum[q] - comp[q]) * dv;
  store_n(a.out + (int64_t)row * a.ldo, k0, a.D, vec, sum);
}

// ---- host: the two launches of a pass ----------------------------------------------------------------------------------
// fwd(lpe, grid): one team per unit, channels past a team's go to further tiles (grid.y); merge(lpe, grid): one
// workgroup per long row and channel tile, when the plan has segments.  cpl: channels per lane.
template <class Fwd, class Merge>
hipError_t unit_sum_launch(int D, int cpl, int min_lanes, int64_t n_units, int32_t n_long, int32_t n_seg, const Fwd& fwd,
                           const Merge& merge) {
  const int nchunk = (D + cpl - 1) / cpl;
  const int lpe = lanes_for(nchunk, min_lanes);
  const int T = 256 / lpe;
  const int tiles = (nchunk + lpe - 1) / lpe;
  const dim3 grid((unsigned)((n_units + T - 1) / T), tiles);
  if (grid.x > 0) fwd(lpe, grid);
  if (n_seg > 0 && n_long > 0) merge(lpe, dim3(n_long, tiles));
  return hipGetLastError();
}

}  // namespace stag
