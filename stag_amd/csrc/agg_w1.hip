// agg_w1.hip — stag_agg_fwd_w1: aggregation with ONE weight per edge, shared by all channels (gfx950).
//
//   out[v, k] = dscale[v] * (sum | mean)_{p in row v} w1[p] * sscale[u_p] * x[u_p, k]
//
// w1[p] is element 0 of the noise stream's block at (pos_base + nidx[p] | p, chunk 0) — what stag_noise_materialize
// writes at Dn = 1 — or an explicit w[E] by edge id: DropEdge (Bernoulli), DropEdge with renormalisation upstream, one
// learned weight per edge (an AmortizedDistribution(in, 1)).  The per-channel kernels draw a Philox block per edge and
// 4 channels; here a weight costs one block per EDGE, and the draw leaves the hot loop altogether:
//   a team of LPE lanes (4 channels a lane) takes its unit in ROUNDS of up to LPE edges.  Lane l loads indices[p0 + l],
//   nidx and — explicit weights, [E, 1] parameters — its edge's values by edge id (coalesced across the team), and
//   draws the weight of ITS edge: one Philox block per lane and round.  The team then walks the round in groups of
//   4 positions: (u_j, w_j) come from lane j by __shfl, the rows of a group are all requested before the first is
//   used, and AN EDGE WHOSE WEIGHT IS EXACTLY 0.0 IS NOT GATHERED (a team-uniform branch): a dropped Bernoulli edge, a
//   relu'd non-positive draw, an explicit zero.  On finite x that changes no bit — blocks are cut by POSITION (4
//   consecutive edges of the round, kept or not; a block sum starts at +0 and fma(0, x, t) = t), which is why the kept
//   edges are not compacted first: compaction would move the block boundaries with the draw.  On a non-finite row
//   the skip yields 0 where a multiply would yield NaN: the edge is absent, as after DGL's DropEdge.
// Block sums are folded into the unit's sum in order, Kahan-compensated once the unit is longer than kKahanMinLen
// (AggTeam::fold_into's rule).  A segment of a long row leaves its fp32 partial in the plan's workspace; a second small
// launch (one workgroup per long row) adds every long row's partials group by group in segment order and applies the
// row scale.  No atomics, no arrival counters: two launches with the same inputs give the same bits.
// agg_kernel.hpp and noise.hpp are included for their helpers only.
#include "agg_w1.hpp"
#include "entry_args.hpp"
#include "agg_kernel.hpp"   // load4 / store4, kKahanMinLen, kCombineGroup, u32x4_t (read-only helpers)

// A/B only (tools/ab_bench.py): 1 = multiply by a zero weight instead of skipping its row.  The contract is the skip.
#ifndef STAG_W1_NO_SKIP
#define STAG_W1_NO_SKIP 0
#endif

namespace stag {
namespace {

// positions of a round whose rows are requested together: one block of 4, as in the kernels without a draw (58-60 VGPRs,
// 7-8 waves per SIMD).  8 (two blocks; A/B only, teams of 8 lanes and more) keeps 86-89 VGPRs and 5 waves and is slower
// wherever edges are dropped: profiles/r15/edge_weight.txt.  The bits do not depend on it.
#ifndef STAG_W1_GROUP
#define STAG_W1_GROUP 4
#endif
template <int LPE>
constexpr int w1_group() { return LPE >= 8 ? STAG_W1_GROUP : 4; }

// the unit a team serves (plan order; no plan: unit i = row i); false past the end
template <int LPE>
__device__ __forceinline__ bool w1_unit(const W1Args& a, int& row, int& start, int& len, int& slot) {
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

__device__ __forceinline__ float w1_row_scale(const W1Args& a, int v, int deg) {
  float dv = a.dst_scale ? a.dst_scale[v] : 1.0f;
  if (a.mean) dv *= __builtin_amdgcn_rcpf((float)(deg > 1 ? deg : 1));
  return dv;
}

// the weight of the edge at CSR position p: stag_noise_materialize's w[eid, 0] at Dn = 1, bit for bit
template <int KIND>
__device__ __forceinline__ float w1_weight(const W1Args& a, const PhiloxKey& key, int p) {
  const bool by_edge = KIND == kExplicit || a.pmode == STAG_PARAM_PER_EDGE1;
  const int64_t ed = (by_edge && a.eid) ? a.eid[p] : p;
  if constexpr (KIND == kExplicit) {
    const float t = a.p0[ed];
    return (a.nflags & kFlagRelu) ? fmaxf(t, 0.f) : t;
  } else {
    float q0 = a.p0s, q1 = a.p1s;                       // (a scalar log-scale was exponentiated on the host)
    if (a.pmode == STAG_PARAM_PER_CHANNEL) {            // a one-element row: how a device scalar travels
      q0 = a.p0[0];
      q1 = a.p1 ? a.p1[0] : 0.f;
    } else if (a.pmode == STAG_PARAM_PER_EDGE1) {
      q0 = a.p0[ed];
      q1 = a.p1 ? a.p1[ed] : 0.f;
      if (a.nflags & kFlagLogScale) q1 = exp_scale(q1);
    }
    const float pa[4] = {q0, 0.f, 0.f, 0.f}, pb[4] = {q1, 0.f, 0.f, 0.f};
    const uint32_t pos = a.pos_lo + (uint32_t)(a.nidx ? a.nidx[p] : p);
    float w[4];
    draw4<KIND>(pos, a.pos_hi << 20, key, pa, pb, a.nflags & (kFlagRelu | kFlagLogScale), w);   // chunk 0
    return w[0];
  }
}

template <int KIND, int LPE>
__global__ __launch_bounds__(256) void agg_w1_fwd_kernel(const W1Args a) {
  constexpr int G = w1_group<LPE>();
  const int lane = threadIdx.x % LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);        // the lane's 4 channels
  // (no early return for a lane without channels: it still loads and draws the edges of its position in a round)
  const bool live = k0 < a.D;
  int row, start, len, slot;
  if (!w1_unit<LPE>(a, row, start, len, slot)) return;
  PhiloxKey key{};
  if constexpr (KIND >= kNormal) key = resolve_epoch(a.key);
  const uint32_t koff = (uint32_t)k0 * 4u;
  const bool xv = a.xvec != 0, narrow = a.x_bytes != 0;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  const bool kahan = len > kKahanMinLen;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, comp[4] = {0.f, 0.f, 0.f, 0.f};
  const int end = start + len;
  for (int r0 = start; r0 < end; r0 += LPE) {
    // the round: lane l owns the edge at r0 + l
    const int n = min(LPE, end - r0);
    int u = 0;
    float w = 0.f, ws = 0.f;                             // past the round's end: a zero weight, never gathered
    if (lane < n) {
      const int p = r0 + lane;
      u = a.indices[p];
      w = w1_weight<KIND>(a, key, p);
      ws = w;
      if (a.src_scale && (STAG_W1_NO_SKIP || w != 0.f)) ws = w * a.src_scale[u];
    }
    for (int j0 = 0; j0 < n; j0 += G) {                  // n is uniform over the team
      int uq[G];
      float wq[G], sq[G], xr[G][4];
      bool take[G];
#pragma unroll
      for (int q = 0; q < G; ++q) {
        uq[q] = __shfl(u, j0 + q, LPE);
        wq[q] = __shfl(w, j0 + q, LPE);
        sq[q] = a.src_scale ? __shfl(ws, j0 + q, LPE) : wq[q];
        take[q] = live && (STAG_W1_NO_SKIP ? j0 + q < n : wq[q] != 0.f);
      }
#pragma unroll
      for (int q = 0; q < G; ++q) {
        if (take[q]) {                                   // the skip: uniform over the lanes of a team that have channels
          if (xv) {
            u32x4_t t;
            if (narrow) {
              t = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(__umul24((uint32_t)uq[q], a.ldxb) + koff), 0, 0);
            } else {
              const char* r = reinterpret_cast<const char*>(a.x) + (uint64_t)(uint32_t)uq[q] * a.ldxb + koff;
              t = *reinterpret_cast<const u32x4_t*>(r);
            }
            xr[q][0] = __uint_as_float(t.x); xr[q][1] = __uint_as_float(t.y);
            xr[q][2] = __uint_as_float(t.z); xr[q][3] = __uint_as_float(t.w);
          } else {
            const char* r = reinterpret_cast<const char*>(a.x) + (uint64_t)(uint32_t)uq[q] * a.ldxb;
            load4(reinterpret_cast<const float*>(r), k0, a.D, false, xr[q]);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < G; b += 4) {                   // a block: 4 consecutive positions, summed from +0
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = b; q < b + 4; ++q) {
          if (take[q]) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = __builtin_fmaf(sq[q], xr[q][c], t[c]);
          }
        }
        if (j0 + b < n) {                                // (a block past the round's end is not a block of the sum)
          if (kahan) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float y = t[c] - comp[c];
              const float s = acc[c] + y;
              comp[c] = (s - acc[c]) - y;
              acc[c] = s;
            }
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += t[c];
          }
        }
      }
    }
  }
  if (!live) return;
  if (slot >= 0) {   // a segment: its partial, added by agg_w1_merge_kernel
    store4(a.ws + (int64_t)slot * a.D, k0, a.D, a.ovec != 0, acc);
    return;
  }
  const float dv = w1_row_scale(a, row, len);
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] *= dv;
  store4(a.out + (int64_t)row * a.ldo, k0, a.D, a.ovec != 0, acc);
}

// One workgroup per long row and channel tile: Kahan sums of GROUPS of kCombineGroup partials in segment order, one
// group per team and round, then team 0 folds the group sums in group order — a group's Kahan residual joins the
// second level's compensation (the two-level form of agg_half_merge_kernel).  Groups are cut by segment index alone.
template <int LPE>
__global__ __launch_bounds__(256) void agg_w1_merge_kernel(const W1Args a) {
  constexpr int T = 256 / LPE, kAhead = 8;
  __shared__ float part[T][2][LPE * 4];          // a round's group sums and what they still owe (8 KB)
  const int r = blockIdx.x, team = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);
  const bool live = k0 < a.D;                    // (no early return: the workgroup meets at barriers)
  const int row = a.long_rows[r];
  const int s0 = a.long_seg_ptr[r], s1 = a.long_seg_ptr[r + 1];
  const bool vec = a.ovec != 0;
  float sum[4] = {0.f, 0.f, 0.f, 0.f}, comp[4] = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = s0; g0 < s1; g0 += kCombineGroup * T) {   // uniform over the workgroup
    const int gs = g0 + team * kCombineGroup;
    if (live && gs < s1) {
      const int ge = min(gs + kCombineGroup, s1);
      float gsum[4] = {0.f, 0.f, 0.f, 0.f}, gres[4] = {0.f, 0.f, 0.f, 0.f};
      for (int s = gs; s < ge; s += kAhead) {
        float t[kAhead][4];
#pragma unroll
        for (int j = 0; j < kAhead; ++j)
          if (s + j < ge) load4(a.ws + (int64_t)(s + j) * a.D, k0, a.D, vec, t[j]);
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
          if (s + j < ge) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float y = t[j][c] - gres[c];
              const float n = gsum[c] + y;
              gres[c] = (n - gsum[c]) - y;
              gsum[c] = n;
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) { part[team][0][lane * 4 + c] = gsum[c]; part[team][1][lane * 4 + c] = gres[c]; }
    }
    __syncthreads();
    if (team == 0 && live) {
      for (int j = 0; j < T && g0 + j * kCombineGroup < s1; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          comp[c] += part[j][1][lane * 4 + c];             // true group sum = its sum - its residual
          const float y = part[j][0][lane * 4 + c] - comp[c];
          const float n = sum[c] + y;
          comp[c] = (n - sum[c]) - y;
          sum[c] = n;
        }
      }
    }
    __syncthreads();                                       // the next round overwrites the group sums
  }
  if (team != 0 || !live) return;
  const float dv = w1_row_scale(a, row, a.indptr[row + 1] - a.indptr[row]);
#pragma unroll
  for (int c = 0; c < 4; ++c) sum[c] = (sum[c] - comp[c]) * dv;
  store4(a.out + (int64_t)row * a.ldo, k0, a.D, vec, sum);
}

template <int KIND>
void w1_fwd_kind(const W1Args& a, int lpe, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
    hipLaunchKernelGGL((agg_w1_fwd_kernel<KIND, decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace

hipError_t w1_fwd_launch(const W1Args& a, int kind, int32_t n_seg, hipStream_t s) {
  const int nchunk = (a.D + 3) / 4;
  const int lpe = lanes_for(nchunk, 4);   // 4 channels per lane
  const int T = 256 / lpe;
  const int tiles = (nchunk + lpe - 1) / lpe;
  const dim3 grid((unsigned)(((int64_t)a.n_units + T - 1) / T), tiles);
  if (grid.x > 0) {
    switch (kind) {
      case kExplicit: w1_fwd_kind<kExplicit>(a, lpe, grid, s); break;
      case kNormal: w1_fwd_kind<kNormal>(a, lpe, grid, s); break;
      case kUniform: w1_fwd_kind<kUniform>(a, lpe, grid, s); break;
      default: w1_fwd_kind<kBernoulli>(a, lpe, grid, s); break;
    }
  }
  if (n_seg > 0 && a.n_long > 0) {
    const dim3 mg(a.n_long, tiles);                      // one workgroup per long row and channel tile
    pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
      hipLaunchKernelGGL((agg_w1_merge_kernel<decltype(L)::value>), mg, dim3(256), 0, s, a);
    });
  }
  return hipGetLastError();
}

}  // namespace stag

using namespace stag;

extern "C" int stag_agg_fwd_w1(const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx, int32_t D,
                               const stag_noise_spec* spec, int32_t reduce, const float* src_scale,
                               const float* dst_scale, float* out, int64_t ldo, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(csr);
  if (rc) return rc;
  if (!x || !spec || !out) return STAG_EINVAL;
  if (D <= 0 || ldx < 0 || (ldx > 0 && ldx < D) || ldo < D) return STAG_EINVAL;
  if (reduce != STAG_REDUCE_SUM && reduce != STAG_REDUCE_MEAN) return STAG_EINVAL;
  if (spec->kind < STAG_NOISE_EXPLICIT || spec->kind > STAG_NOISE_BERNOULLI) return STAG_EINVAL;   // NONE: stag_agg_fwd's
  if (spec->deriv != 0) return STAG_EINVAL;
  const bool drawn = spec->kind >= STAG_NOISE_NORMAL;
  if (drawn && spec->param_mode == STAG_PARAM_PER_EDGE) return STAG_EINVAL;   // [E, Dn] parameters at Dn = 1 are [E, 1]
  if (spec->kind == STAG_NOISE_EXPLICIT && spec->group != 0 && spec->group != 1 && spec->group != D) return STAG_EINVAL;
  const bool use_plan = plan_in_use(plan);
  if (use_plan && check_plan_units(plan, kPlanCounts)) return STAG_EINVAL;
  // the width-1 spec as stag_noise_materialize reads it: kind, parameters, counter bounds, the log-scale
  // (STAG_ENOSYS: a per-channel log-scale, exponentiated by the caller)
  rc = check_spec(spec, csr->n_edges, 1);
  if (rc) return rc;
  // what the two-launch route (stag_noise_materialize at width 1, stag_agg_fwd with group = D) keeps
  if (spec->in_norm || ldx == 0 || spec->chunk_base != 0) return STAG_ENOSYS;
  rc = check_positions(spec, csr->n_edges, 1, drawn);   // one 2^32 range of the global position per call
  if (rc) return rc;
  const int32_t n_seg = use_plan ? plan->n_seg : 0;
  if (use_plan && (rc = check_plan_segments(plan, kPlanSegPtr | kPlanWorkspace, stag_plan_workspace_bytes(n_seg, D, 0)))) return rc;
  if (csr->n_dst == 0) return STAG_OK;

  W1Args a{};
  a.indptr = csr->indptr; a.indices = csr->indices; a.eid = csr->eid; a.nidx = csr->nidx;
  a.n_rows = csr->n_dst; a.D = D;
  a.x = x; a.ldxb = (uint32_t)(ldx * 4);
  {
    // 32-bit byte offsets and 24-bit multiplies behind a buffer descriptor when they reach every row, else 64-bit addresses
    const uint64_t xbytes = csr->n_src > 0 ? ((uint64_t)(csr->n_src - 1) * (uint64_t)ldx + (uint64_t)D) * 4u : 0u;
    const bool narrow = xbytes > 0 && xbytes < (1ull << 32) && csr->n_src < (1 << 24) && (uint64_t)ldx * 4u < (1u << 24);
    a.x_bytes = narrow ? (uint32_t)xbytes : 0u;
    if (!narrow && (uint64_t)ldx * 4u >= (1ull << 32)) return STAG_ENOSYS;   // a row stride past 32 bits of bytes
  }
  a.xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  fill_spec(a, spec, 0);   // (flags: relu and the log-scale; a derivative was refused above)
  a.src_scale = src_scale; a.dst_scale = dst_scale; a.mean = reduce == STAG_REDUCE_MEAN;
  fill_plan(a, csr, plan);   // plan->xcd_order is ignored: the units are walked in plan order
  a.out = out; a.ldo = ldo;
  a.ovec = D % 4 == 0 && aligned16(out) && ldo % 4 == 0 && (n_seg == 0 || aligned16(plan->workspace));
  return w1_fwd_launch(a, spec->kind, n_seg, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}
