// edge_embed.hip — the wide edge embedding of an AmortizedDistribution(in, out > 1) in one pass each way (gfx950).
//
//   forward     h[e, k] = SiLU(ps[src[e], k] + pd[dst[e], k])                                 stag_edge_embed_fwd
//   backward    d_own[r, k] = sum_{p in row r} g[eid[p], k] * SiLU'(own[r, k] + other[indices[p], k])   stag_edge_embed_bwd
//     pre = ps + pd rounded to fp32,  sg = 1 / (1 + expf(-pre)),  SiLU = pre * sg,  SiLU' = sg * (1 + pre * (1 - sg))
//     (amort.hip's sigmoidf: the narrow and the wide form of the embedding compute the same function)
//
// The forward is edge-parallel by edge id, as stag_edge_mlp_fwd is: a team of LPE lanes (4 channels a lane) takes
// kEdgesPerTeam edges, requests the two rows of all of them, and only then forms and stores the first.  Channels past a
// team's width go to further channel tiles (grid.y).
// The backward is one kernel for both tables: on the destination-major view own = pd, other = ps gives d pd; on the
// source-major view own = ps, other = pd gives d ps.  The pre-activation is formed again from the two tables, so no
// [E, hidden] tensor is kept by the forward or formed here.  It walks the plan's units in plan order (unit_sum.hpp):
// one team per unit, the own row loaded once, the unit's edges in rounds of LPE (lane l loads indices and eid of the
// edge at r0 + l, coalesced across the team) and blocks of 4 positions — the block's 4 gathered rows and 4 gradient
// rows are all requested before the first is used; a block's terms are summed from +0 and folded into the unit's sum
// in order, Kahan-compensated past kKahanMinLen.  A segment of a long row leaves its partial in the plan's workspace
// and seg_merge adds them in a second small launch.  No atomics, no counters: two launches give the same bits.
#include "edge_embed.hpp"
#include "unit_sum.hpp"     // the unit walk, the block fold, the segment merge; agg_kernel.hpp's load4 / store4, u32x4_t

namespace stag {
namespace {

constexpr int kEdgesPerTeam = 4;   // edges whose rows a forward team has in flight together

__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int LPE>
__global__ __launch_bounds__(256) void edge_embed_fwd_kernel(const EmbedFwdArgs a) {
  constexpr int T = 256 / LPE;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);
  if (k0 >= a.D) return;
  // team t takes edges e0 + t, e0 + T + t, ...: neighbouring teams store neighbouring rows of h
  const int64_t e0 = (int64_t)blockIdx.x * (T * kEdgesPerTeam) + team;
  const bool pv = a.pvec != 0;
  int u[kEdgesPerTeam], v[kEdgesPerTeam];
#pragma unroll
  for (int j = 0; j < kEdgesPerTeam; ++j) {
    const int64_t e = e0 + (int64_t)j * T;
    const bool in = e < a.E;
    u[j] = in ? a.src[e] : 0;
    v[j] = in ? a.dst[e] : 0;
  }
  float s[kEdgesPerTeam][4], d[kEdgesPerTeam][4];
#pragma unroll
  for (int j = 0; j < kEdgesPerTeam; ++j) {
    if (e0 + (int64_t)j * T < a.E) {
      load4(a.ps + (int64_t)u[j] * a.ldps, k0, a.D, pv, s[j]);
      load4(a.pd + (int64_t)v[j] * a.ldpd, k0, a.D, pv, d[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kEdgesPerTeam; ++j) {
    const int64_t e = e0 + (int64_t)j * T;
    if (e < a.E) {
      float h[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float pre = s[j][c] + d[j][c];
        h[c] = pre * sigmoid_f(pre);
      }
      store4(a.h + e * a.ldh, k0, a.D, a.hvec != 0, h);
    }
  }
}

// 4 channels of row `idx` of a gathered table: 32-bit offsets behind the descriptor, or a 64-bit address
__device__ __forceinline__ void gather4(const float* base, __amdgpu_buffer_rsrc_t rsrc, bool narrow, bool vec, int idx,
                                        uint32_t ldb, int k0, int D, float (&v)[4]) {
  if (vec && narrow) {
    const u32x4_t t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24((uint32_t)idx, ldb) + (uint32_t)k0 * 4u), 0, 0);
    v[0] = __uint_as_float(t.x); v[1] = __uint_as_float(t.y);
    v[2] = __uint_as_float(t.z); v[3] = __uint_as_float(t.w);
  } else {
    const char* r = reinterpret_cast<const char*>(base) + (uint64_t)(uint32_t)idx * ldb;
    load4(reinterpret_cast<const float*>(r), k0, D, vec, v);
  }
}

template <int LPE>
__global__ __launch_bounds__(256) void edge_embed_bwd_kernel(const EmbedBwdArgs a) {
  const int lane = threadIdx.x % LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);        // the lane's 4 channels
  // (no early return for a lane without channels: it still loads the ids of its position in a round)
  const bool live = k0 < a.D;
  int row, start, len, slot;
  if (!unit_of<LPE>(a, row, start, len, slot)) return;
  const bool xv = a.xvec != 0, xn = a.x_bytes != 0, gn = a.g_bytes != 0;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g), 0, (int)a.g_bytes, 0x00020000);
  float own[4] = {0.f, 0.f, 0.f, 0.f};
  if (live && len > 0) load4(a.own + (int64_t)row * a.ld_own, k0, a.D, xv, own);   // once per unit
  const bool kahan = len > kKahanMinLen;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, comp[4] = {0.f, 0.f, 0.f, 0.f};
  const int end = start + len;
  for (int r0 = start; r0 < end; r0 += LPE) {
    // the round: lane l owns the ids of the edge at r0 + l
    const int n = min(LPE, end - r0);
    int u = 0, ed = 0;
    if (lane < n) {
      const int p = r0 + lane;
      u = a.indices[p];
      ed = a.eid ? a.eid[p] : p;
    }
    for (int j0 = 0; j0 < n; j0 += 4) {                  // n is uniform over the team
      float xr[4][4], gr[4][4];
      bool take[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int uq = __shfl(u, j0 + q, LPE), eq = __shfl(ed, j0 + q, LPE);
        take[q] = live && j0 + q < n;
        if (take[q]) {
          gather4(a.x, rx, xn, xv, uq, a.ldxb, k0, a.D, xr[q]);
          gather4(a.g, rg, gn, xv, eq, a.ldgb, k0, a.D, gr[q]);
        }
      }
      float t[4] = {0.f, 0.f, 0.f, 0.f};                 // a block: 4 consecutive positions, summed from +0
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (take[q]) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float pre = own[c] + xr[q][c];
            const float sg = sigmoid_f(pre);
            t[c] = __builtin_fmaf(gr[q][c], sg * (1.0f + pre * (1.0f - sg)), t[c]);
          }
        }
      }
      fold_block(kahan, t, acc, comp);
    }
  }
  if (!live) return;
  if (slot >= 0) {   // a segment: its partial, added by edge_embed_merge_kernel
    store4(a.ws + (int64_t)slot * a.D, k0, a.D, a.ovec != 0, acc);
    return;
  }
  store4(a.out + (int64_t)row * a.ldo, k0, a.D, a.ovec != 0, acc);
}

template <int LPE>
__global__ __launch_bounds__(256) void edge_embed_merge_kernel(const EmbedBwdArgs a) { seg_merge<4, LPE>(a); }

}  // namespace

hipError_t embed_fwd_launch(const EmbedFwdArgs& a, hipStream_t s) {
  const int nchunk = (a.D + 3) / 4;
  const int lpe = lanes_for(nchunk, 4);
  const int per_block = (256 / lpe) * kEdgesPerTeam;
  const dim3 grid((unsigned)((a.E + per_block - 1) / per_block), (nchunk + lpe - 1) / lpe);
  pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
    hipLaunchKernelGGL((edge_embed_fwd_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
  return hipGetLastError();
}

hipError_t embed_bwd_launch(const EmbedBwdArgs& a, int32_t n_seg, hipStream_t s) {
  return unit_sum_launch(a.D, 4, 4, a.n_units, a.n_long, n_seg,
      [&](int lpe, dim3 grid) {
        pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
          hipLaunchKernelGGL((edge_embed_bwd_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      },
      [&](int lpe, dim3 grid) {
        pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
          hipLaunchKernelGGL((edge_embed_merge_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      });
}

}  // namespace stag

using namespace stag;

extern "C" int stag_edge_embed_fwd(const int32_t* src, const int32_t* dst, int64_t n_edges, const float* ps, int64_t ldps,
                                   const float* pd, int64_t ldpd, int32_t hidden, float* h, int64_t ldh, void* stream) {
  // every decision below is taken before any device work
  if (n_edges < 0 || n_edges > 0x7FFFFFFFll || hidden <= 0) return STAG_EINVAL;
  if (ldps < hidden || ldpd < hidden || ldh < hidden) return STAG_EINVAL;
  if (n_edges == 0) return STAG_OK;
  if (!src || !dst || !ps || !pd || !h) return STAG_EINVAL;
  EmbedFwdArgs a{};
  a.src = src; a.dst = dst; a.E = n_edges;
  a.ps = ps; a.pd = pd; a.ldps = ldps; a.ldpd = ldpd; a.D = hidden;
  const bool v4 = hidden % 4 == 0;
  a.pvec = v4 && ldps % 4 == 0 && ldpd % 4 == 0 && aligned16(ps) && aligned16(pd);
  a.h = h; a.ldh = ldh;
  a.hvec = v4 && ldh % 4 == 0 && aligned16(h);
  return embed_fwd_launch(a, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_edge_embed_bwd(const stag_csr* view, const stag_plan* plan, const float* own, int64_t ld_own,
                                   const float* other, int64_t ld_other, int32_t hidden, const float* g, int64_t ldg,
                                   float* d_own, int64_t ldd, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(view);
  if (rc) return rc;
  if (hidden <= 0 || ld_own < hidden || ld_other < hidden || ldg < hidden || ldd < hidden) return STAG_EINVAL;
  if (view->n_edges > 0 && (!own || !other || !g || !d_own)) return STAG_EINVAL;
  const bool use_plan = plan_in_use(plan);
  if (use_plan && check_plan_units(plan, kPlanCounts)) return STAG_EINVAL;
  const int32_t n_seg = use_plan ? plan->n_seg : 0;
  if (use_plan && (rc = check_plan_segments(plan, kPlanSegPtr | kPlanWorkspace, stag_plan_workspace_bytes(n_seg, hidden, 0)))) return rc;
  if (view->n_dst == 0 || !d_own) return STAG_OK;   // (no edges: every row of d_own is written as zeros below)

  EmbedBwdArgs a{};
  a.indptr = view->indptr; a.indices = view->indices; a.eid = view->eid;
  a.D = hidden;
  a.own = own; a.ld_own = ld_own;
  a.x = other; a.ldxb = (uint32_t)(ld_other * 4);
  a.g = g; a.ldgb = (uint32_t)(ldg * 4);
  if ((rc = narrow_rows(view->n_src, ld_other, hidden, 4, a.x_bytes))) return rc;
  if ((rc = narrow_rows(view->n_edges, ldg, hidden, 4, a.g_bytes))) return rc;
  a.xvec = hidden % 4 == 0 && ld_own % 4 == 0 && ld_other % 4 == 0 && ldg % 4 == 0 && aligned16(own) && aligned16(other) &&
           aligned16(g);
  fill_plan(a, view, plan);   // plan->xcd_order is ignored: the units are walked in plan order
  a.out = d_own; a.ldo = ldd;
  a.ovec = hidden % 4 == 0 && aligned16(d_own) && ldd % 4 == 0 && (n_seg == 0 || aligned16(plan->workspace));
  return embed_bwd_launch(a, n_seg, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}
