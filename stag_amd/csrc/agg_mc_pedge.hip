// agg_mc_pedge.hip — stag_agg_fwd_mc_pedge: Monte-Carlo samples of an aggregation whose noise has [E, D] parameters
// (STAG_PARAM_PER_EDGE: the loc / log_scale heads of an AmortizedDistribution(in, in)), from ONE pass over the gathered
// rows AND over the two parameter tables (gfx950).
//
//   out_s[v, k] = dscale[v] * (sum | mean)_{p in row v} w_s[p, k] * sscale[u_p] * x[u_p, k]        s = 0 .. n_samples - 1
//
// w_s[p, k] is stag_agg_fwd's weight for the same spec at offset + s * offset_stride, bit for bit: element k % 4 of the
// Philox block at (pos_base + nidx[p] | p, chunk k / 4) through draw4 with the lane's four values of p0[e, k0 .. k0 + 3]
// and p1[e, k0 .. k0 + 3], e = eid[p] | p.  What the samples of an edge share is loaded once: the column id, the edge id
// and the position, the lane's 4 values of each parameter row (the log-scale is exponentiated where it is loaded), the
// source scale and the lane's 4 channels of the row.  What differs is the draw: one Philox block per sample, with the
// sample's own key.  A pass carries K = 1, 2 or 4 samples; every sample has its own block sums, unit sums and
// compensation terms, and no operation mixes two samples, so a sample's bits do not depend on the pass it rides in.
// How the plan's units are walked, a block sum is folded and a long row's segments are merged: unit_sum.hpp (a block
// is 4 consecutive positions, summed from +0).  A segment leaves K partial rows in the plan's workspace, sample-major
// ([K][n_seg][D]), so that the merge of a sample is seg_merge on that sample's slice (grid.z = the sample).
// agg_kernel.hpp and noise.hpp are included for their helpers only.
#include "agg_mc_pedge.hpp"
#include "unit_sum.hpp"     // the unit walk, the block fold, the row scale, the segment merge; agg_kernel.hpp's load4, u32x4_t

namespace stag {
namespace {

template <int KIND, int K, int LPE>
__global__ __launch_bounds__(256)
void agg_mc_pedge_fwd_kernel(const McPEdgeArgs a) {
  const int lane = threadIdx.x % LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);        // the lane's 4 channels
  int row, start, len, slot;
  if (!unit_of<LPE>(a, row, start, len, slot)) return;
  if (k0 >= a.D) return;                               // (lanes do not exchange anything: a lane without channels leaves)
  PhiloxKey key[K];
  key[0] = resolve_epoch(a.key);
#pragma unroll
  for (int s = 1; s < K; ++s) key[s] = key_plus(key[0], (uint64_t)s * a.mc_stride);
  const uint32_t c1 = (uint32_t)(k0 >> 2) | (a.pos_hi << 20);   // Philox counter word 1 (chunk_base = 0: the entry point)
  const int dflags = a.nflags & (kFlagRelu | kFlagLogScale);
  const uint32_t koff = (uint32_t)k0 * 4u;
  const bool xv = a.xvec != 0, narrow = a.x_bytes != 0, pv = a.pvec != 0;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  const bool kahan = len > kKahanMinLen;
  float acc[K][4], comp[K][4];
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[s][c] = comp[s][c] = 0.f;
  const int end = start + len;
  for (int b0 = start; b0 < end; b0 += 4) {            // a block: 4 consecutive positions, summed from +0
    int u[4];
    int64_t ed[4];
    uint32_t nn[4];
    float pa[4][4], pb[4][4], xr[4][4];
    // what the K samples of an edge share, once per edge
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u[j] = 0; ed[j] = 0; nn[j] = 0;
      if (b0 + j < end) {
        const int p = b0 + j;
        u[j] = a.indices[p];
        ed[j] = a.eid ? a.eid[p] : p;
        nn[j] = a.pos_lo + (uint32_t)(a.nidx ? a.nidx[p] : p);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b0 + j < end) {
        load4(a.p0 + ed[j] * a.D, k0, a.D, pv, pa[j]);   // (rows D floats apart, as stag_agg_fwd takes them)
        load4(a.p1 + ed[j] * a.D, k0, a.D, pv, pb[j]);
        if (a.nflags & kFlagLogScale) {
#pragma unroll
          for (int c = 0; c < 4; ++c) pb[j][c] = exp_scale(pb[j][c]);
        }
        if (xv) {
          u32x4_t t;
          if (narrow) {
            t = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(__umul24((uint32_t)u[j], a.ldxb) + koff), 0, 0);
          } else {
            const char* r = reinterpret_cast<const char*>(a.x) + (uint64_t)(uint32_t)u[j] * a.ldxb + koff;
            t = *reinterpret_cast<const u32x4_t*>(r);
          }
          xr[j][0] = __uint_as_float(t.x); xr[j][1] = __uint_as_float(t.y);
          xr[j][2] = __uint_as_float(t.z); xr[j][3] = __uint_as_float(t.w);
        } else {
          const char* r = reinterpret_cast<const char*>(a.x) + (uint64_t)(uint32_t)u[j] * a.ldxb;
          load4(reinterpret_cast<const float*>(r), k0, a.D, false, xr[j]);
        }
        if (a.src_scale) {                             // stag_agg_fwd's order: the row is scaled, then weighted
          const float ss = a.src_scale[u[j]];
#pragma unroll
          for (int c = 0; c < 4; ++c) xr[j][c] *= ss;
        }
      }
    }
    float t[K][4];
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) t[s][c] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b0 + j < end) {
#pragma unroll
        for (int s = 0; s < K; ++s) {                  // the draws: the one thing a sample does not share
          float w[4];
          draw4<KIND>(nn[j], c1, key[s], pa[j], pb[j], dflags, w);
#pragma unroll
          for (int c = 0; c < 4; ++c) t[s][c] = __builtin_fmaf(w[c], xr[j][c], t[s][c]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < K; ++s) fold_block(kahan, t[s], acc[s], comp[s]);
  }
  const bool ov = a.ovec != 0;
  if (slot >= 0) {   // a segment: K partials, added per sample by agg_mc_pedge_merge_kernel
#pragma unroll
    for (int s = 0; s < K; ++s) store4(a.ws + ((int64_t)s * a.n_seg + slot) * a.D, k0, a.D, ov, acc[s]);
    return;
  }
  const float dv = row_scale(a, row, len);
#pragma unroll
  for (int s = 0; s < K; ++s) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[s][c] *= dv;
    store4(a.out + (int64_t)s * a.sample_stride + (int64_t)row * a.ldo, k0, a.D, ov, acc[s]);
  }
}

// the merge of sample blockIdx.z: seg_merge on that sample's slice of the workspace and of the output
template <int LPE>
__global__ __launch_bounds__(256) void agg_mc_pedge_merge_kernel(McPEdgeArgs a) {
  a.ws += (int64_t)blockIdx.z * a.n_seg * a.D;
  a.out += (int64_t)blockIdx.z * a.sample_stride;
  seg_merge<4, LPE>(a);
}

template <int KIND, int K>
void mc_pedge_fwd_kind(const McPEdgeArgs& a, int lpe, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
    hipLaunchKernelGGL((agg_mc_pedge_fwd_kernel<KIND, K, decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace

hipError_t mc_pedge_launch(const McPEdgeArgs& a, int kind, int k, hipStream_t s) {
  return unit_sum_launch(a.D, 4, 4, a.n_units, a.n_long, a.n_seg,
      [&](int lpe, dim3 grid) {
        pick<kNormal, kUniform>(kind, [&](auto KD) {
          pick<4, 2, 1>(k, [&](auto KS) { mc_pedge_fwd_kind<decltype(KD)::value, decltype(KS)::value>(a, lpe, grid, s); });
        });
      },
      [&](int lpe, dim3 grid) {
        grid.z = (unsigned)k;
        pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
          hipLaunchKernelGGL((agg_mc_pedge_merge_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      });
}

}  // namespace stag

using namespace stag;

extern "C" int stag_agg_fwd_mc_pedge(const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx, int32_t D,
                                     const stag_noise_spec* spec, int32_t n_samples, int64_t offset_stride, int32_t reduce,
                                     const float* src_scale, const float* dst_scale, float* out, int64_t ldo,
                                     int64_t sample_stride, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(csr);
  if (rc) return rc;
  if (!x || !spec || !out) return STAG_EINVAL;
  if (D <= 0 || ldx < 0 || (ldx > 0 && ldx < D) || ldo < D) return STAG_EINVAL;
  if (n_samples < 1 || offset_stride < 0) return STAG_EINVAL;
  if (n_samples > 1 && sample_stride < (int64_t)csr->n_dst * ldo) return STAG_EINVAL;
  if (reduce != STAG_REDUCE_SUM && reduce != STAG_REDUCE_MEAN) return STAG_EINVAL;
  if (spec->kind < STAG_NOISE_NORMAL || spec->kind > STAG_NOISE_BERNOULLI) return STAG_EINVAL;   // NONE / EXPLICIT: no draw
  if (spec->param_mode != STAG_PARAM_PER_EDGE) return STAG_EINVAL;   // PER_EDGE1: stag_agg_fwd_mc_edge's; SCALAR / PER_CHANNEL: stag_agg_fwd_mc's
  if (spec->deriv != 0) return STAG_EINVAL;
  const bool use_plan = plan_in_use(plan);
  if (use_plan && check_plan_units(plan, kPlanCounts)) return STAG_EINVAL;
  rc = check_spec(spec, csr->n_edges, D);               // a NULL p0 / p1 (a graph with edges), the counter bounds of stag_agg_fwd
  if (rc) return rc;
  // what the loop over stag_agg_fwd keeps
  if (spec->in_norm || ldx == 0 || spec->chunk_base != 0 || spec->kind == STAG_NOISE_BERNOULLI) return STAG_ENOSYS;
  rc = check_positions(spec, csr->n_edges, D, true);    // one 2^32 range of the global position per call
  if (rc) return rc;
  const int32_t n_seg = use_plan ? plan->n_seg : 0;
  if (use_plan && (rc = check_plan_segments(plan, kPlanSegPtr | kPlanWorkspace,
                                            stag_plan_workspace_bytes(n_seg, kMcPEdgeMaxK * D, 0)))) return rc;

  McPEdgeArgs a{};
  a.indptr = csr->indptr; a.indices = csr->indices; a.eid = csr->eid; a.nidx = csr->nidx;
  a.n_rows = csr->n_dst; a.D = D;
  a.x = x; a.ldxb = (uint32_t)(ldx * 4);
  if ((rc = narrow_rows(csr->n_src, ldx, D, 4, a.x_bytes))) return rc;
  if (csr->n_dst == 0) return STAG_OK;
  a.xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  a.pvec = D % 4 == 0 && aligned16(spec->p0) && aligned16(spec->p1);
  a.src_scale = src_scale; a.dst_scale = dst_scale; a.mean = reduce == STAG_REDUCE_MEAN;
  fill_plan(a, csr, plan);   // plan->xcd_order is ignored: the units are walked in plan order
  a.n_seg = n_seg > 0 ? n_seg : 0;
  a.ldo = ldo; a.sample_stride = sample_stride; a.mc_stride = (uint64_t)offset_stride;
  a.ovec = D % 4 == 0 && aligned16(out) && ldo % 4 == 0 && (n_samples == 1 || sample_stride % 4 == 0) &&
           (n_seg <= 0 || aligned16(plan->workspace));
  // the largest built pass first (4, then 2, then 1 samples); every pass starts its own samples at the right offset
  stag_noise_spec sp = *spec;
  for (int32_t s0 = 0; s0 < n_samples;) {
    int k = kMcPEdgeMaxK;
    while (k > n_samples - s0) k >>= 1;
    sp.offset = spec->offset + (uint64_t)s0 * (uint64_t)offset_stride;
    fill_spec(a, &sp, 0);   // (flags: relu and the log-scale; a derivative was refused above)
    a.out = out + (int64_t)s0 * sample_stride;
    if (mc_pedge_launch(a, spec->kind, k, (hipStream_t)stream) != hipSuccess) return STAG_EIO;
    s0 += k;
  }
  return STAG_OK;
}
