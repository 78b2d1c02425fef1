// agg_bwd_w_mc.hip — stag_agg_bwd_w_mc: the per-edge parameter gradients of a Monte-Carlo batch (the backward of
// stag_agg_fwd_mc_edge and stag_agg_fwd_mc_pedge with respect to the amortised parameters) from ONE pass over the
// gathered rows and the parameter tables (gfx950).
//
//   dw_i[eid_p, k] = sum_{s = 0 .. n_samples - 1} D_i,s[p, k] * (sscale[u_p] * x[u_p, k]) * (gscale[v] * g_s[v, k])     i = 0, 1
//
// D_0,s / D_1,s are the two derivatives of the draw at offset + s * offset_stride: what stag_agg_bwd_w (api.hip,
// agg_bwd_w_body<LPE, VEC, 2>) writes to dw / dw1 for that spec.  The walk is that kernel's: a team of LPE lanes per
// unit of the plan, 4 channels per lane, two edges in flight, the channel tiles walked inside the team.  What the
// samples of an edge share is loaded once: the column id, the edge id and the position, the source scale, the lane's 4
// channels of x[u] and the lane's 4 values of each parameter row (or the edge's two scalars; the log-scale is
// exponentiated where it is loaded).  The K gradient rows of a pass are the unit's own rows and live in registers, times
// g_scale[v].  Per sample: one Philox block at the sample's key and two multiply-adds into the running sums, which start
// from sample 0's term.  Each gradient row is written once per pass; a later pass of the call (n_samples > K) starts its
// sums from what the previous pass left — the same lane owns the same edge and the passes are in stream order.
// No atomics.  agg_kernel.hpp and noise.hpp are included for their helpers only.
#include "agg_bwd_w_mc.hpp"
#include "unit_sum.hpp"     // the unit walk; agg_kernel.hpp's load4, store4 and team_sum

namespace stag {
namespace {

template <int KIND, int K, int LPE>
__global__ __launch_bounds__(256)
void agg_bwd_w_mc_kernel(const BwdWMcArgs a) {
  const int c = threadIdx.x % LPE;
  int v, rb, len, slot;
  if (!unit_of<LPE>(a, v, rb, len, slot)) return;
  const int D = a.D;
  const int ntile = ((D + 3) / 4 + LPE - 1) / LPE;
  PhiloxKey key[K];
  key[0] = resolve_epoch(a.key);
#pragma unroll
  for (int s = 1; s < K; ++s) key[s] = key_plus(key[0], (uint64_t)s * a.mc_stride);
  const int dflags = a.nflags & (kFlagRelu | kFlagLogScale);
  const bool xvec = a.xvec != 0, gvec = a.gvec != 0, pvec = a.pvec != 0, wvec = a.wvec != 0;
  const bool edge1 = a.pmode == STAG_PARAM_PER_EDGE1, two = a.dw1 != nullptr, reduce_k = a.reduce_k != 0;
  const bool fresh = reduce_k || !a.accumulate;          // the sums start from sample 0's term
  const float* grow = a.g + (int64_t)v * a.ldg;
  const float gs = a.g_scale ? a.g_scale[v] : 1.0f;
  float gv[K][4];
  auto load_g = [&](int k0) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      load4(grow + (int64_t)s * a.g_sample_stride, k0, D, gvec, gv[s]);
      if (a.g_scale) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gv[s][q] *= gs;
      }
    }
  };
#pragma unroll
  for (int s = 0; s < K; ++s) gv[s][0] = gv[s][1] = gv[s][2] = gv[s][3] = 0.f;
  if (ntile == 1 && c * 4 < D) load_g(c * 4);
  const int end = rb + len;
  for (int p0 = rb; p0 < end; p0 += 2) {
    int u[2];
    int64_t ed[2];
    uint32_t nn[2];
    float ss[2], q0[2] = {0.f, 0.f}, q1[2] = {0.f, 0.f}, tot0[2] = {0.f, 0.f}, tot1[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool live = p0 + j < end;
      u[j] = live ? a.indices[p0 + j] : 0;
      ed[j] = live ? (a.eid ? a.eid[p0 + j] : p0 + j) : 0;
      nn[j] = a.pos_lo + (uint32_t)((live && a.nidx) ? a.nidx[p0 + j] : p0 + j);
      ss[j] = (live && a.src_scale) ? a.src_scale[u[j]] : 1.0f;
      if (edge1 && live) {                               // [E, 1] parameters: in flight with the rows
        q0[j] = a.p0[ed[j]];
        q1[j] = a.p1[ed[j]];
        if (a.nflags & kFlagLogScale) q1[j] = exp_scale(q1[j]);
      }
    }
    for (int tile = 0; tile < ntile; ++tile) {
      const uint32_t chunk = tile * LPE + c;
      const int k0 = (int)chunk * 4;
      if (k0 >= D) continue;
      if (ntile > 1) load_g(k0);
      const uint32_t c1 = chunk | (a.pos_hi << 20);      // Philox counter word 1 (chunk_base = 0: the entry point)
      float xr[2][4], pa[2][4], pb[2][4], s0[2][4], s1[2][4];
      // what the K samples of an edge share, once per edge
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s0[j][q] = s1[j][q] = 0.f;
        if (p0 + j < end) {
          load4(a.x + (int64_t)u[j] * a.ldx, k0, D, xvec, xr[j]);
          if (edge1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { pa[j][q] = q0[j]; pb[j][q] = q1[j]; }
          } else {
            load4(a.p0 + ed[j] * D, k0, D, pvec, pa[j]);   // (rows D floats apart, as stag_agg_bwd_w takes them)
            load4(a.p1 + ed[j] * D, k0, D, pvec, pb[j]);
            if (a.nflags & kFlagLogScale) {
#pragma unroll
              for (int q = 0; q < 4; ++q) pb[j][q] = exp_scale(pb[j][q]);
            }
          }
          if (!fresh) {                                  // what the previous pass left for this edge
            load4(a.dw0 + ed[j] * a.ldw, k0, D, wvec, s0[j]);
            if (two) load4(a.dw1 + ed[j] * a.ldw, k0, D, wvec, s1[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (p0 + j < end) {
          float sx[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) sx[q] = ss[j] * xr[j][q];
#pragma unroll
          for (int s = 0; s < K; ++s) {                  // the draws: the one thing a sample does not share
            float w[4], d0[4], d1[4];
            draw4_grad<KIND>(nn[j], c1, key[s], pa[j], pb[j], dflags, w, d0, d1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float val = (k0 + q < D) ? sx[q] * gv[s][q] : 0.f;
              if (s == 0 && fresh) {
                s0[j][q] = d0[q] * val;
                s1[j][q] = d1[q] * val;
              } else {
                s0[j][q] = __builtin_fmaf(d0[q], val, s0[j][q]);
                s1[j][q] = __builtin_fmaf(d1[q], val, s1[j][q]);
              }
            }
          }
          if (!reduce_k) {
            store4(a.dw0 + ed[j] * a.ldw, k0, D, wvec, s0[j]);
            if (two) store4(a.dw1 + ed[j] * a.ldw, k0, D, wvec, s1[j]);
          } else {
            tot0[j] += (s0[j][0] + s0[j][1]) + (s0[j][2] + s0[j][3]);
            tot1[j] += (s1[j][0] + s1[j][1]) + (s1[j][2] + s1[j][3]);
          }
        }
      }
    }
    if (reduce_k) {                                      // agg_bwd_w_body's fixed-order team sum
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        tot0[j] = team_sum<LPE>(tot0[j]);
        if (two) tot1[j] = team_sum<LPE>(tot1[j]);
        if (p0 + j < end && c == 0) {
          float* o0 = a.dw0 + ed[j] * a.ldw;
          o0[0] = a.accumulate ? o0[0] + tot0[j] : tot0[j];
          if (two) {
            float* o1 = a.dw1 + ed[j] * a.ldw;
            o1[0] = a.accumulate ? o1[0] + tot1[j] : tot1[j];
          }
        }
      }
    }
  }
}

template <int KIND, int K>
void bwd_w_mc_kind(const BwdWMcArgs& a, int lpe, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4, 2, 1>(lpe, [&](auto L) {
    hipLaunchKernelGGL((agg_bwd_w_mc_kernel<KIND, K, decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace

hipError_t bwd_w_mc_launch(const BwdWMcArgs& a, int kind, int k, hipStream_t s) {
  const int lpe = lanes_for((a.D + 3) / 4, 1);
  const int T = 256 / lpe;
  const dim3 grid((unsigned)(((int64_t)a.n_units + T - 1) / T));
  pick<kNormal, kUniform>(kind, [&](auto KD) {
    pick<4, 2, 1>(k, [&](auto KS) { bwd_w_mc_kind<decltype(KD)::value, decltype(KS)::value>(a, lpe, grid, s); });
  });
  return hipGetLastError();
}

}  // namespace stag

using namespace stag;

extern "C" int stag_agg_bwd_w_mc(const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx,
                                 const float* g, int64_t ldg, int64_t g_sample_stride, int32_t D,
                                 const float* src_scale, const float* g_scale, const stag_noise_spec* spec,
                                 int32_t n_samples, int64_t offset_stride, int32_t reduce_k,
                                 float* dw0, float* dw1, int64_t ldw, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(csr);
  if (rc) return rc;
  if (!x || !g || !spec || !dw0) return STAG_EINVAL;
  if (D <= 0 || ldx < 0 || (ldx > 0 && ldx < D) || ldg < D || ldw < (reduce_k ? 1 : D)) return STAG_EINVAL;
  if (n_samples < 1 || offset_stride < 0) return STAG_EINVAL;
  if (n_samples > 1 && g_sample_stride < (int64_t)csr->n_dst * ldg) return STAG_EINVAL;
  if (spec->kind != STAG_NOISE_NORMAL && spec->kind != STAG_NOISE_UNIFORM) return STAG_EINVAL;   // no reparameterised draw
  if (spec->param_mode != (reduce_k ? STAG_PARAM_PER_EDGE1 : STAG_PARAM_PER_EDGE)) return STAG_EINVAL;   // SCALAR / PER_CHANNEL: stag_agg_bwd_dp's
  if (spec->deriv != 0) return STAG_EINVAL;
  BwdWMcArgs a{};
  if ((rc = fill_units(a, csr, plan))) return rc;       // a plan without units
  rc = check_spec(spec, csr->n_edges, D);               // a NULL p0 / p1 (a graph with edges), the counter bounds of stag_agg_fwd
  if (rc) return rc;
  // what the loop over stag_agg_bwd_w keeps
  if (spec->in_norm || ldx == 0 || spec->chunk_base != 0) return STAG_ENOSYS;
  if (ldx >= (1ll << 30) || ldg >= (1ll << 30)) return STAG_ENOSYS;
  rc = check_positions(spec, csr->n_edges, D, true);    // one 2^32 range of the global position per call
  if (rc) return rc;
  if (csr->n_dst == 0 || csr->n_edges == 0) return STAG_OK;

  a.indptr = csr->indptr; a.indices = csr->indices; a.eid = csr->eid; a.nidx = csr->nidx;
  a.n_rows = csr->n_dst; a.D = D;
  a.x = x; a.ldx = ldx; a.ldg = ldg; a.g_sample_stride = g_sample_stride;
  a.src_scale = src_scale; a.g_scale = g_scale;
  a.xvec = D % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  a.gvec = D % 4 == 0 && ldg % 4 == 0 && aligned16(g) && (n_samples == 1 || g_sample_stride % 4 == 0);
  a.pvec = D % 4 == 0 && aligned16(spec->p0) && aligned16(spec->p1);
  a.wvec = D % 4 == 0 && ldw % 4 == 0 && aligned16(dw0) && (!dw1 || aligned16(dw1));
  a.reduce_k = reduce_k ? 1 : 0;
  a.dw0 = dw0; a.dw1 = dw1; a.ldw = ldw; a.mc_stride = (uint64_t)offset_stride;
  // the largest built pass first (4, then 2, then 1 samples); every pass starts its own samples at the right offset
  stag_noise_spec sp = *spec;
  for (int32_t s0 = 0; s0 < n_samples;) {
    int k = kBwdWMcMaxK;
    while (k > n_samples - s0) k >>= 1;
    sp.offset = spec->offset + (uint64_t)s0 * (uint64_t)offset_stride;
    fill_spec(a, &sp, 0);   // (flags: relu and the log-scale; a derivative selector was refused above)
    a.g = g + (int64_t)s0 * g_sample_stride;
    a.accumulate = s0 > 0;
    if (bwd_w_mc_launch(a, spec->kind, k, (hipStream_t)stream) != hipSuccess) return STAG_EIO;
    s0 += k;
  }
  return STAG_OK;
}
