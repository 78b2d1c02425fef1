// entry_args.hpp — host side only: how an entry point of include/stag_hip.h reads its stag_csr, stag_noise_spec and
// stag_plan.  One definition of every check and of the spec -> kernel-argument translation; api.hip, gat.hip and
// agg_half.hip compose them in the order that gives each entry point its return codes, and take every decision
// before any device work.  And how every source gets from a runtime lane count to a kernel's template argument: pick.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// How a kernel addresses n_src gathered rows of D elements of esize bytes, ldx elements apart.  x_bytes = the extent of
// x when 32-bit byte offsets and 24-bit multiplies (row < 2^24, stride < 2^24 bytes) reach all of it behind a buffer
// descriptor, else 0: 64-bit addresses, whose 32-bit row stride refuses one past 32 bits of bytes (STAG_ENOSYS).
// (gat.hip's narrow_extent is another rule: contiguous rows, no stride limit.)
inline int narrow_rows(int64_t n_src, int64_t ldx, int32_t D, uint32_t esize, uint32_t& x_bytes) {
  const uint64_t stride = (uint64_t)ldx * esize;
  const uint64_t xbytes = n_src > 0 ? ((uint64_t)(n_src - 1) * (uint64_t)ldx + (uint64_t)D) * esize : 0u;
  const bool narrow = xbytes > 0 && xbytes < (1ull << 32) && n_src < (1 << 24) && stride < (1u << 24);
  x_bytes = narrow ? (uint32_t)xbytes : 0u;
  return !narrow && stride >= (1ull << 32) ? STAG_ENOSYS : STAG_OK;
}

// The same decision for the kernels of agg_common (api.hip: stag_agg_fwd, stag_agg_fwd_mc, stag_agg_bwd, stag_agg_bwd_edge,
// stag_agg_bwd_dp), which also read per-edge rows of D floats ([E, D] weights or parameters, by edge id or CSR position):
//   wide bit 0: x takes 64-bit addresses (n_src >= 2^24 rows, a stride >= 2^24 bytes, or n_src * ldx * 4 >= 2^32 bytes)
//   wide bit 1: the per-edge rows do (n_edges >= 2^24, D * 4 >= 2^24, or n_edges * D * 4 >= 2^32; an upper bound when grouped)
//   x_bytes: the extent behind x's buffer descriptor in the narrow form (n_src rows of ldx floats; ldx == 0: the one
//            broadcast row of D floats), else 0
//   idx_bytes: the extent of the column ids behind theirs, 0 from 2^30 edges on
// The row stride travels as 32 bits of bytes in every form: one of 2^32 bytes or more is refused (STAG_ENOSYS), as
// narrow_rows refuses it.
struct AggForms {
  uint32_t wide, x_bytes, idx_bytes;
};
inline int agg_forms(int64_t n_src, int64_t n_edges, int64_t ldx, int32_t D, AggForms& f) {
  f = AggForms{};
  if (ldx >= (1ll << 30)) return STAG_ENOSYS;
  const uint64_t xbytes = (uint64_t)n_src * (uint64_t)ldx * 4u;
  const uint64_t wbytes = (uint64_t)n_edges * (uint64_t)D * 4u;
  const bool x_narrow = xbytes < (1ull << 32) && n_src < (1 << 24) && (uint64_t)ldx * 4u < (1u << 24);
  const bool w_narrow = wbytes < (1ull << 32) && n_edges < (1 << 24) && (uint64_t)D * 4u < (1u << 24);
  f.wide = (x_narrow ? 0u : 1u) | (w_narrow ? 0u : 2u);
  f.x_bytes = x_narrow ? (uint32_t)(ldx == 0 ? (uint64_t)D * 4u : xbytes) : 0u;
  f.idx_bytes = n_edges < (1 << 30) ? (uint32_t)n_edges * 4u : 0u;
  return STAG_OK;
}

// lanes per row: the smallest power of two >= min_lanes that covers nchunk chunks, capped at a wave
inline int lanes_for(int nchunk, int min_lanes) {
  int lpe = min_lanes;
  while (lpe < nchunk && lpe < 64) lpe <<= 1;
  return lpe;
}

// lanes per head of a row of heads of F channels: F / 4 rounded up to a power of two (any F: callers refuse after it)
inline int lanes_per_head(int F) {
  int l = 1;
  while ((int64_t)l * 4 < F) l <<= 1;
  return l;
}

// ---- from a runtime value to a template argument ---------------------------------------------------------------------
// The one ladder of every launch: f(std::integral_constant<int, V>{}) for the V of Vs... that equals v, the last of them
// when none does.  A launch site lists its kernel's instantiations, the default last, and launches from a generic lambda:
//   pick<64, 32, 16, 8, 4>(lpe, [&](auto L) { hipLaunchKernelGGL((kernel<decltype(L)::value>), grid, block, 0, s, a); });
template <int V0, int... Vs, class F>
inline void pick(int v, const F& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else pick<Vs...>(v, f);
}
// ... for kernels with a bool next to it (vec): f(std::integral_constant<int, V>{}, std::bool_constant<b>{})
template <int... Vs, class F>
inline void pick(int v, bool b, const F& f) {
  pick<Vs...>(v, [&](auto V) {
    if (b) f(V, std::true_type{});
    else f(V, std::false_type{});
  });
}

// ---- stag_csr ------------------------------------------------------------------------------------------------------
// What must hold before any other field of the csr is read.  The GAT entry points start with this much and run
// check_csr as their last refusal, so that every code they return above it stands.
inline int check_csr_header(const stag_csr* g) {
  return (!g || !g->indptr || g->n_dst < 0 || g->n_edges < 0) ? STAG_EINVAL : STAG_OK;
}

inline int check_csr(const stag_csr* g) {
  if (check_csr_header(g) || g->n_src < 0) return STAG_EINVAL;
  if (g->n_edges > 0x7FFFFFFFll) return STAG_EINVAL;   // int32 CSR positions
  if (g->n_edges > 0 && !g->indices) return STAG_EINVAL;
  return STAG_OK;
}

// ---- stag_noise_spec -----------------------------------------------------------------------------------------------
// n_edges: per-edge arrays (explicit weights, [E, 1 | Dn] parameters) of a graph without edges have no address.
// Dn: the noise width, whose chunks must fit the counter word's chunk field (0: not known here)
inline int check_spec(const stag_noise_spec* s, int64_t n_edges = 1, int32_t Dn = 0) {
  if (!s) return STAG_EINVAL;
  if (s->kind < STAG_NOISE_NONE || s->kind > STAG_NOISE_BERNOULLI) return STAG_EINVAL;
  if (s->kind == STAG_NOISE_EXPLICIT && !s->p0 && n_edges > 0) return STAG_EINVAL;
  if (s->deriv < 0 || s->deriv > 2 || s->chunk_base < 0 || s->chunk_base >= (1 << 20)) return STAG_EINVAL;
  if (s->deriv != 0 && (s->in_norm || (s->kind != STAG_NOISE_NORMAL && s->kind != STAG_NOISE_UNIFORM)))
    return STAG_EINVAL;   // only reparameterised draws have a derivative; in-norm is not differentiated here
  if (s->p1_log != 0 && (s->p1_log != 1 || s->kind != STAG_NOISE_NORMAL)) return STAG_EINVAL;   // a log-scale is a Normal's
  if (s->p1_log && s->param_mode == STAG_PARAM_PER_CHANNEL) return STAG_ENOSYS;   // exponentiate a [Dn] row yourself
  if (s->kind >= STAG_NOISE_NORMAL) {
    if (!counter_space_ok(s->pos_base, n_edges, s->chunk_base, ((int64_t)Dn + 3) / 4)) return STAG_EINVAL;
    if (s->param_mode < STAG_PARAM_SCALAR || s->param_mode > STAG_PARAM_PER_EDGE) return STAG_EINVAL;
    const bool per_edge = s->param_mode == STAG_PARAM_PER_EDGE1 || s->param_mode == STAG_PARAM_PER_EDGE;
    if (s->param_mode != STAG_PARAM_SCALAR && !(per_edge && n_edges == 0)) {
      if (!s->p0) return STAG_EINVAL;
      if (s->kind != STAG_NOISE_BERNOULLI && !s->p1) return STAG_EINVAL;
    }
  }
  return STAG_OK;
}

// The global positions of a launch that draws (edge weights, or an attention-dropout mask): STAG_EINVAL outside what
// the counter word names (counter_space_ok), STAG_ENOSYS across a 2^32 boundary: the kernels keep hi32 of the position
// fixed and add the local index (with or without nidx) to lo32 in 32 bits.  Shards are < 2^31 edges, so a caller splits
// the call at the boundary.
inline uint32_t pos_lo32(int64_t pos_base) { return (uint32_t)((uint64_t)pos_base & 0xFFFFFFFFull); }
inline int check_positions(const stag_noise_spec* s, int64_t n_edges, int32_t Dn, bool drawn) {
  if (!drawn) return STAG_OK;
  if (!counter_space_ok(s->pos_base, n_edges, s->chunk_base, ((int64_t)Dn + 3) / 4)) return STAG_EINVAL;
  if ((uint64_t)pos_lo32(s->pos_base) + (uint64_t)n_edges > (1ull << 32)) return STAG_ENOSYS;
  return STAG_OK;
}

inline PhiloxKey make_key(uint64_t seed, uint64_t offset, const uint64_t* epoch) {
  PhiloxKey k;
  k.k0 = (uint32_t)(seed & 0xFFFFFFFFull);
  k.k1 = (uint32_t)(seed >> 32);
  k.o0 = (uint32_t)(offset & 0xFFFFFFFFull);
  k.o1 = (uint32_t)(offset >> 32);
  k.epoch = epoch;
  return k;
}

// members that only some argument blocks have: a kernel family templated on the kind carries no `kind`, the GAT
// kernels no `chunk_base`, and the position is either one 64-bit `pos_base` or `pos_lo` / `pos_hi`
#define STAG_HAS_MEMBER(M)                                                                    \
  template <class A, class = void> struct has_##M : std::false_type {};                       \
  template <class A> struct has_##M<A, std::void_t<decltype(std::declval<A&>().M)>> : std::true_type {}
STAG_HAS_MEMBER(kind);
STAG_HAS_MEMBER(chunk_base);
STAG_HAS_MEMBER(pos_base);
#undef STAG_HAS_MEMBER

// The noise fields of a kernel's argument block from a checked spec.  `deriv`: the derivative selector of the flag
// word (spec->deriv, or 0 where the kernel returns both derivatives).  A scalar log-scale is exponentiated here.
template <class Args>
void fill_spec(Args& a, const stag_noise_spec* s, int32_t deriv) {
  const bool logs = s->kind == STAG_NOISE_NORMAL && s->p1_log;
  if constexpr (has_kind<Args>::value) a.kind = s->kind;
  a.pmode = s->kind >= STAG_NOISE_NORMAL ? s->param_mode : 0;
  a.nflags = (s->relu ? kFlagRelu : 0) | (deriv << kDerivShift) | (logs ? kFlagLogScale : 0);
  a.p0 = s->p0; a.p1 = s->p1;
  a.p0s = s->p0_scalar; a.p1s = logs ? expf(s->p1_scalar) : s->p1_scalar;
  a.key = make_key(s->seed, s->offset, s->epoch);
  if constexpr (has_pos_base<Args>::value) {
    a.pos_base = s->pos_base;
  } else {
    a.pos_lo = pos_lo32(s->pos_base);
    a.pos_hi = (uint32_t)((uint64_t)s->pos_base >> 32);
  }
  if constexpr (has_chunk_base<Args>::value) a.chunk_base = (uint32_t)s->chunk_base;
}

// ---- stag_plan -----------------------------------------------------------------------------------------------------
// what a launch needs of a plan beyond its units
enum : unsigned {
  kPlanCounts = 1,       // n_seg and n_long size a grid of their own: refuse negative ones
  kPlanHeavy = 2,        // units[0, n_heavy) is walked as a prefix of its own
  kPlanXcd = 4,          // the units are walked in the XCD-aware order when the plan has one
  kPlanSegPtr = 8,       // the segments of a long row are merged: long_seg_ptr next to long_rows
  kPlanWorkspace = 16,   // ... through ws_bytes of partials in plan->workspace
  kPlanNarrow = 32,      // ... which go through a 32-bit buffer descriptor
  kPlanCounters = 64,    // ... by the segment that arrives last: seg_counters
};

inline bool plan_in_use(const stag_plan* p) { return p && p->n_units > 0; }

inline int check_plan_units(const stag_plan* p, unsigned needs) {
  if (!p->units || !aligned16(p->units)) return STAG_EINVAL;
  if ((needs & kPlanCounts) && (p->n_seg < 0 || p->n_long < 0)) return STAG_EINVAL;
  return STAG_OK;
}

// the records of the XCD-aware order (stag_plan_xcd): 8 heavy stripes of sh of them, then 8 light ones of sl
inline const stag_unit* xcd_units(const stag_plan* p) {
  return reinterpret_cast<const stag_unit*>(p->xcd_order + STAG_XCD_HEADER);
}

inline int check_plan_segments(const stag_plan* p, unsigned needs, size_t ws_bytes = 0) {
  if (p->n_seg <= 0) return STAG_OK;
  if (!p->long_rows || ((needs & kPlanSegPtr) && !p->long_seg_ptr) || ((needs & kPlanWorkspace) && !p->workspace) ||
      ((needs & kPlanCounters) && !p->seg_counters))
    return STAG_EINVAL;
  if ((needs & kPlanWorkspace) && p->workspace_bytes < ws_bytes) return STAG_ENOMEM;
  if ((needs & kPlanNarrow) && ws_bytes >= (1ull << 32)) return STAG_ENOSYS;
  return STAG_OK;
}

// a plan that may be absent (NULL, or n_units <= 0: one unit per row): units, heavy prefix, XCD order, segments
inline int check_plan(const stag_plan* p, unsigned needs, size_t ws_bytes = 0) {
  if (!plan_in_use(p)) return STAG_OK;
  if (check_plan_units(p, needs)) return STAG_EINVAL;
  if ((needs & kPlanHeavy) && (p->n_heavy < 0 || p->n_heavy > p->n_units)) return STAG_EINVAL;
  const int64_t sh = p->xcd_stride_heavy, sl = p->xcd_stride_light;
  if ((needs & kPlanXcd) && p->xcd_order &&
      (!aligned16(p->xcd_order) || sh < 0 || sl < 0 || sh > p->n_heavy || sl > p->n_units ||     /* (sl may count heavy units: stag_plan_xcd_ranges with n_heavy = 0) */
       STAG_XCD_STRIPES * (sh + sl) < p->n_units || STAG_XCD_STRIPES * (sh + sl) > 0x7FFFFFFFll)) return STAG_EINVAL;
  return check_plan_segments(p, needs, ws_bytes);
}

// the units a launch walks (the plan's, or one per row) and, where the plan has segments, the long rows they merge
// into through the workspace
template <class Args>
void fill_plan(Args& a, const stag_csr* csr, const stag_plan* plan) {
  a.n_units = csr->n_dst;
  if (!plan_in_use(plan)) return;
  a.units = plan->units; a.n_units = plan->n_units;
  if (plan->n_seg <= 0) return;
  a.long_rows = plan->long_rows; a.long_seg_ptr = plan->long_seg_ptr; a.n_long = plan->n_long;
  a.ws = plan->workspace;
}

// ... for a kernel without a merge, which only looks the rows of its segments up; checked here
template <class Args>
int fill_units(Args& a, const stag_csr* csr, const stag_plan* plan) {
  if (check_plan(plan, 0)) return STAG_EINVAL;
  a.n_units = csr->n_dst;
  if (plan_in_use(plan)) { a.units = plan->units; a.long_rows = plan->long_rows; a.n_units = plan->n_units; }
  return STAG_OK;
}

}  // namespace stag
