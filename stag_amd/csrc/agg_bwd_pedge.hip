// agg_bwd_pedge.hip — stag_agg_bwd_pedge: the backward of an aggregation whose noise has [E, D] parameters
// (STAG_PARAM_PER_EDGE: the loc / log_scale heads of an AmortizedDistribution(in, in)) from ONE pass over the
// source-major CSR (gfx950): dx AND the two [E, D] gradient tables.
//
//   dx[u, k]       = row_scale[u] * sum_{p in row u} w[p, k] * (g_scale[v_p] * g[v_p, k])
//   dp_i[eid_p, k] = D_i[p, k] * (row_scale[u] * x[u, k]) * (g_scale[v_p] * g[v_p, k])                  i = 0, 1
//
// w, D_0 and D_1 come from one Philox block per edge and chunk (draw4_grad at (pos_base + nidx[p], chunk k / 4)): the row
// of x the gradients need is the unit's own row on this CSR, the row of g is the one the dx pass gathers anyway, and the
// lane's 4 values of p0[e, :] and p1[e, :] serve the weight and both derivatives.  There is no channel sum: the two
// gradient rows of an edge are stored where the edge is walked and need no merge.
// The walk is agg_mc_pedge.hip's at one sample: a team of LPE lanes per unit of the plan, 4 channels a lane, further
// channel tiles in grid.y, blocks of 4 consecutive positions whose loads are all requested before the first is used.  How
// a block's dx terms are folded and a long row's segments are merged: unit_sum.hpp (a block is summed from +0).  So dx is
// stag_agg_fwd_mc_pedge(csr_t, x = g, n_samples = 1, SUM, src_scale = g_scale, dst_scale = row_scale) bit for bit, and
// dp_i are stag_agg_bwd_w_mc's at one sample (products only, in that entry's association).  No atomics, no arrival
// counters.  agg_kernel.hpp and noise.hpp are included for their helpers only.
#include "agg_bwd_pedge.hpp"
#include "unit_sum.hpp"     // the unit walk, the block fold, the row scale, the segment merge; agg_kernel.hpp's load4, u32x4_t

namespace stag {
namespace {

template <int KIND, int LPE>
__global__ __launch_bounds__(256)
void agg_bwd_pedge_kernel(const BwdPEdgeArgs a) {
  const int lane = threadIdx.x % LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);        // the lane's 4 channels
  int row, start, len, slot;
  if (!unit_of<LPE>(a, row, start, len, slot)) return;
  if (k0 >= a.D) return;                               // (lanes do not exchange anything: a lane without channels leaves)
  const PhiloxKey key = resolve_epoch(a.key);
  const uint32_t c1 = (uint32_t)(k0 >> 2) | (a.pos_hi << 20);   // Philox counter word 1 (chunk_base = 0: the entry point)
  const int dflags = a.nflags & (kFlagRelu | kFlagLogScale);
  const uint32_t koff = (uint32_t)k0 * 4u;
  const bool gv = a.gvec != 0, narrow = a.g_bytes != 0, pv = a.pvec != 0, wv = a.wvec != 0, two = a.dp1 != nullptr;
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g), 0, (int)a.g_bytes, 0x00020000);
  const bool kahan = len > kKahanMinLen;
  // the unit's own: x[u] times row_scale[u], once
  float xs[4];
  load4(a.x + (int64_t)row * a.ldx, k0, a.D, a.xvec != 0, xs);
  if (a.dst_scale) {
    const float rs = a.dst_scale[row];
#pragma unroll
    for (int c = 0; c < 4; ++c) xs[c] *= rs;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, comp[4] = {0.f, 0.f, 0.f, 0.f};
  const int end = start + len;
  for (int b0 = start; b0 < end; b0 += 4) {            // a block: 4 consecutive positions, dx terms summed from +0
    int v[4];
    int64_t ed[4];
    uint32_t nn[4];
    float pa[4][4], pb[4][4], gr[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0; ed[j] = 0; nn[j] = 0;
      if (b0 + j < end) {
        const int p = b0 + j;
        v[j] = a.indices[p];
        ed[j] = a.eid[p];
        nn[j] = a.pos_lo + (uint32_t)a.nidx[p];
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
        if (gv) {
          u32x4_t t;
          if (narrow) {
            t = __builtin_amdgcn_raw_buffer_load_b128(rg, (int)(__umul24((uint32_t)v[j], a.ldgb) + koff), 0, 0);
          } else {
            const char* r = reinterpret_cast<const char*>(a.g) + (uint64_t)(uint32_t)v[j] * a.ldgb + koff;
            t = *reinterpret_cast<const u32x4_t*>(r);
          }
          gr[j][0] = __uint_as_float(t.x); gr[j][1] = __uint_as_float(t.y);
          gr[j][2] = __uint_as_float(t.z); gr[j][3] = __uint_as_float(t.w);
        } else {
          const char* r = reinterpret_cast<const char*>(a.g) + (uint64_t)(uint32_t)v[j] * a.ldgb;
          load4(reinterpret_cast<const float*>(r), k0, a.D, false, gr[j]);
        }
        if (a.g_scale) {                               // stag_agg_bwd's order: the row is scaled, then weighted
          const float gs = a.g_scale[v[j]];
#pragma unroll
          for (int c = 0; c < 4; ++c) gr[j][c] *= gs;
        }
      }
    }
    float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b0 + j < end) {
        float w[4], d0[4], d1[4];
        draw4_grad<KIND>(nn[j], c1, key, pa[j], pb[j], dflags, w, d0, d1);   // the one block of the edge and chunk
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t[c] = __builtin_fmaf(w[c], gr[j][c], t[c]);
          const float val = xs[c] * gr[j][c];
          d0[c] *= val;
          d1[c] *= val;
        }
        store4(a.dp0 + ed[j] * a.ldp, k0, a.D, wv, d0);
        if (two) store4(a.dp1 + ed[j] * a.ldp, k0, a.D, wv, d1);
      }
    }
    fold_block(kahan, t, acc, comp);
  }
  if (!a.out) return;                                  // parameter gradients only
  const bool ov = a.ovec != 0;
  if (slot >= 0) {   // a segment: its dx partial, added by agg_bwd_pedge_merge_kernel
    store4(a.ws + (int64_t)slot * a.D, k0, a.D, ov, acc);
    return;
  }
  const float dv = row_scale(a, row, len);
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] *= dv;
  store4(a.out + (int64_t)row * a.ldo, k0, a.D, ov, acc);
}

template <int LPE>
__global__ __launch_bounds__(256) void agg_bwd_pedge_merge_kernel(const BwdPEdgeArgs a) {
  seg_merge<4, LPE>(a);
}

}  // namespace

hipError_t bwd_pedge_launch(const BwdPEdgeArgs& a, int kind, hipStream_t s) {
  return unit_sum_launch(a.D, 4, 4, a.n_units, a.n_long, a.out ? a.n_seg : 0,
      [&](int lpe, dim3 grid) {
        pick<kNormal, kUniform>(kind, [&](auto KD) {
          pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
            hipLaunchKernelGGL((agg_bwd_pedge_kernel<decltype(KD)::value, decltype(L)::value>), grid, dim3(256), 0, s, a);
          });
        });
      },
      [&](int lpe, dim3 grid) {
        pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
          hipLaunchKernelGGL((agg_bwd_pedge_merge_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      });
}

}  // namespace stag

using namespace stag;

extern "C" int stag_agg_bwd_pedge(const stag_csr* csr_t, const stag_plan* plan_t, const float* g, int64_t ldg, int32_t D,
                                  const stag_noise_spec* spec, const float* g_scale, const float* row_scale,
                                  const float* x, int64_t ldx, float* dx, int64_t ldo,
                                  float* dp0, float* dp1, int64_t ldp, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(csr_t);
  if (rc) return rc;
  if (!g || !spec || !x || !dp0) return STAG_EINVAL;
  if (D <= 0 || ldg < D || ldx < 0 || (ldx > 0 && ldx < D) || (dx && ldo < D) || ldp < D) return STAG_EINVAL;
  if (spec->kind != STAG_NOISE_NORMAL && spec->kind != STAG_NOISE_UNIFORM) return STAG_EINVAL;   // no reparameterised draw
  if (spec->param_mode != STAG_PARAM_PER_EDGE) return STAG_EINVAL;   // PER_EDGE1: stag_agg_bwd_edge's; SCALAR / PER_CHANNEL: stag_agg_bwd_dp's
  if (spec->deriv != 0) return STAG_EINVAL;
  // the parameters and their gradients live at edge ids, the noise at forward positions
  if (csr_t->n_edges > 0 && (!csr_t->eid || !csr_t->nidx)) return STAG_EINVAL;
  // a plan without units; the long rows of its segments and, for dx, where their partials go
  if (check_plan(plan_t, dx ? (kPlanCounts | kPlanSegPtr | kPlanWorkspace) : kPlanCounts)) return STAG_EINVAL;
  rc = check_spec(spec, csr_t->n_edges, D);             // a NULL p0 / p1 (a graph with edges), the counter bounds of stag_agg_fwd
  if (rc) return rc;
  // what stag_agg_bwd + stag_agg_bwd_w keep
  if (spec->in_norm || ldx == 0 || spec->chunk_base != 0) return STAG_ENOSYS;
  if (ldx >= (1ll << 30) || ldg >= (1ll << 30)) return STAG_ENOSYS;
  rc = check_positions(spec, csr_t->n_edges, D, true);  // one 2^32 range of the global position per call
  if (rc) return rc;
  const bool use_plan = plan_in_use(plan_t);
  const int32_t n_seg = (use_plan && plan_t->n_seg > 0) ? plan_t->n_seg : 0;
  if (dx && n_seg > 0 && plan_t->workspace_bytes < stag_plan_workspace_bytes(n_seg, D, 0)) return STAG_ENOMEM;

  BwdPEdgeArgs a{};
  a.g = g; a.ldgb = (uint32_t)(ldg * 4);
  if ((rc = narrow_rows(csr_t->n_src, ldg, D, 4, a.g_bytes))) return rc;
  // no edge: nothing per edge to write; with dx the walk below stores every row's zero (no per-edge array is read)
  if (csr_t->n_dst == 0 || (csr_t->n_edges == 0 && !dx)) return STAG_OK;
  a.indptr = csr_t->indptr; a.indices = csr_t->indices; a.eid = csr_t->eid; a.nidx = csr_t->nidx;
  a.n_rows = csr_t->n_dst; a.D = D;
  a.gvec = D % 4 == 0 && ldg % 4 == 0 && aligned16(g);
  a.g_scale = g_scale;
  a.x = x; a.ldx = ldx; a.xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  a.pvec = D % 4 == 0 && aligned16(spec->p0) && aligned16(spec->p1);
  a.dst_scale = row_scale; a.mean = 0;
  fill_plan(a, csr_t, plan_t);   // plan_t->xcd_order is ignored: the units are walked in plan order
  a.n_seg = n_seg;
  a.out = dx; a.ldo = ldo;
  a.ovec = D % 4 == 0 && aligned16(dx) && ldo % 4 == 0 && (n_seg <= 0 || aligned16(plan_t->workspace));
  a.dp0 = dp0; a.dp1 = dp1; a.ldp = ldp;
  a.wvec = D % 4 == 0 && ldp % 4 == 0 && aligned16(dp0) && (!dp1 || aligned16(dp1));
  fill_spec(a, spec, 0);   // (flags: relu and the log-scale; a derivative selector was refused above)
  if (bwd_pedge_launch(a, spec->kind, (hipStream_t)stream) != hipSuccess) return STAG_EIO;
  return STAG_OK;
}
