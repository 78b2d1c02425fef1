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
// How the plan's units are walked, a block sum is folded and a long row's segments are merged: unit_sum.hpp.
// agg_kernel.hpp and noise.hpp are included for their helpers only.
#include "agg_w1.hpp"
#include "unit_sum.hpp"     // the unit walk, the block fold, the row scale, the segment merge; agg_kernel.hpp's load4, u32x4_t

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
  if (!unit_of<LPE>(a, row, start, len, slot)) return;
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
          fold_block(kahan, t, acc, comp);
        }
      }
    }
  }
  if (!live) return;
  if (slot >= 0) {   // a segment: its partial, added by agg_w1_merge_kernel
    store4(a.ws + (int64_t)slot * a.D, k0, a.D, a.ovec != 0, acc);
    return;
  }
  const float dv = row_scale(a, row, len);
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] *= dv;
  store4(a.out + (int64_t)row * a.ldo, k0, a.D, a.ovec != 0, acc);
}

template <int LPE>
__global__ __launch_bounds__(256) void agg_w1_merge_kernel(const W1Args a) { seg_merge<4, LPE>(a); }

template <int KIND>
void w1_fwd_kind(const W1Args& a, int lpe, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
    hipLaunchKernelGGL((agg_w1_fwd_kernel<KIND, decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace

hipError_t w1_fwd_launch(const W1Args& a, int kind, int32_t n_seg, hipStream_t s) {
  return unit_sum_launch(a.D, 4, 4, a.n_units, a.n_long, n_seg,
      [&](int lpe, dim3 grid) {
        pick<kExplicit, kNormal, kUniform, kBernoulli>(kind, [&](auto K) { w1_fwd_kind<decltype(K)::value>(a, lpe, grid, s); });
      },
      [&](int lpe, dim3 grid) {
        pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
          hipLaunchKernelGGL((agg_w1_merge_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      });
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
  if ((rc = narrow_rows(csr->n_src, ldx, D, 4, a.x_bytes))) return rc;
  a.xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  fill_spec(a, spec, 0);   // (flags: relu and the log-scale; a derivative was refused above)
  a.src_scale = src_scale; a.dst_scale = dst_scale; a.mean = reduce == STAG_REDUCE_MEAN;
  fill_plan(a, csr, plan);   // plan->xcd_order is ignored: the units are walked in plan order
  a.out = out; a.ldo = ldo;
  a.ovec = D % 4 == 0 && aligned16(out) && ldo % 4 == 0 && (n_seg == 0 || aligned16(plan->workspace));
  return w1_fwd_launch(a, spec->kind, n_seg, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}
