// gat.hip — GAT edge attention with noisy logits, softmax and aggregation fused
// (stag/zoo/gat.py:114-126):
//     e[p,h]     = w[p,h] * leaky_relu(el[u_p,h] + er[v,h])
//     a[p,h]     = softmax_p(e[.,h])           (DGL edge_softmax: per dst, per head)
//     out[v,h,:] = sum_p a[p,h] * ft[u_p,h,:]
// Noise width is H (`sample_dimension`, stag/zoo/gat.py:11): one Philox block per
// (edge, 4 heads), so this path is gather-bound (an H*F*4-byte row per edge), not RNG-bound.
//
// Same decomposition as the aggregation kernel (agg_kernel.hpp): the launch walks the
// plan's UNITS (whole rows, or <= seg_len-edge segments of long rows, longest first); a
// TEAM of LPE = H*F/4 lanes owns one unit.  Per batch of LPE edges of the unit:
//   phase 1 (edge-parallel)    lane i draws the H weights of edge i, forms the H logits and
//                              parks them in LDS — no RNG work is repeated across lanes;
//   phase 2 (channel-parallel) lane c owns channels [4c, 4c+4) of head h_c: batch max, then
//                              p = exp(logit - max), running sum and weighted row sum.
// A unit ends with a softmax state (m, l, acc) per lane.  Whole rows normalise and store;
// segments publish their state (sc1 stores + ticket, as in agg_kernel) and the last arriver
// merges the states in segment order: m = max m_i, l = sum l_i e^(m_i-m), acc likewise.
#include "../../include/stag_hip.h"
#include "agg_kernel.hpp"
#include "entry_args.hpp"

using namespace stag;

namespace {

#ifndef STAG_GAT_MERGE_NF
#define STAG_GAT_MERGE_NF 12
#endif
constexpr int kGatMergeNF = STAG_GAT_MERGE_NF;   // segment states of a long row fetched per round trip by the row's merge

struct GatArgs {
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;
  const int32_t* nidx;
  int32_t n_rows;
  const float* el;
  const float* er;
  const float* ft;
  const float* nscale;   // [n_rows, H] in-norm factor (null: 1)
  int32_t H, F, HF;
  float neg_slope;
  int32_t kind;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  int32_t pmode, nflags;   // nflags: relu | log-scale << 3 (noise.hpp)
  PhiloxKey key;
  uint32_t pos_lo, pos_hi;
  float* out;
  float* attn;           // [E, H] by edge id, or null (gat_attn_kernel / backward by-product)
  float* stats;          // [n_rows, 2H] softmax statistics per row: m[H] then l[H], or null
  uint32_t ft_bytes;     // extent of ft when it fits a buffer descriptor, else 0
  // plan
  const stag_unit* units;
  int32_t n_units;
  const int32_t* long_rows;
  const int32_t* long_seg_ptr;
  int32_t n_long;
  int32_t* seg_counters;
  float* ws;             // [n_seg][HF + 2*H]: acc, then m[H], l[H]
  int32_t n_seg;         // units [0, n_seg) are the segments of long rows
  int32_t ws_stride;
  uint32_t ws_bytes;
  const int32_t* block_ptr;   // [n_blocks+1] unit batches of the workgroup-cooperative kernels
  int32_t hvec;               // el / er / nscale are 16-byte aligned (rows of H % 4 == 0 heads load as dwordx4)
  int32_t lphp;               // lanes per head in the cooperative kernels: F / 4 rounded up to a power of two
  // attention dropout (stag/zoo/gat.py:122): a[e,h] -> a[e,h] keep[e,h] / keep_prob, keep from its own Philox stream
  float drop_keep;            // keep probability; 0: no dropout
  float drop_scale;           // 1 / keep probability
  PhiloxKey drop_key;
};

// bit j = head 4c + j of the edge with noise index n survives the attention dropout
__device__ __forceinline__ uint32_t drop_keep4(const GatArgs& a, const PhiloxKey& dkey, uint32_t n, uint32_t chunk) {
  const float q[4] = {a.drop_keep, a.drop_keep, a.drop_keep, a.drop_keep};
  float k[4];
  draw4<kBernoulli>(n, chunk | (a.pos_hi << 20), dkey, q, q, 0, k);
  return (k[0] != 0.f ? 1u : 0u) | (k[1] != 0.f ? 2u : 0u) | (k[2] != 0.f ? 4u : 0u) | (k[3] != 0.f ? 8u : 0u);
}

// the 4 weights of heads [4c, 4c+4) of the edge with noise index n and edge id ed
__device__ __forceinline__ void head_w4(const GatArgs& a, const PhiloxKey& key, uint32_t n, int64_t ed,
                                        uint32_t chunk, float (&w)[4]) {
  const int h0 = (int)chunk * 4;
  float pa[4], pb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int h = h0 + j;
    const bool in = h < a.H;
    float q0 = a.p0s, q1 = a.p1s;
    if (a.pmode == STAG_PARAM_PER_CHANNEL) { q0 = in ? a.p0[h] : 0.f; q1 = (in && a.p1) ? a.p1[h] : 0.f; }
    else if (a.pmode == STAG_PARAM_PER_EDGE1) { q0 = a.p0[ed]; q1 = a.p1 ? a.p1[ed] : 0.f; }
    else if (a.pmode == STAG_PARAM_PER_EDGE) {
      q0 = in ? a.p0[ed * a.H + h] : 0.f;
      q1 = (in && a.p1) ? a.p1[ed * a.H + h] : 0.f;
    }
    if (a.pmode != STAG_PARAM_SCALAR && (a.nflags & kFlagLogScale)) q1 = exp_scale(q1);
    pa[j] = q0; pb[j] = q1;
  }
  const uint32_t c1 = chunk | (a.pos_hi << 20);
  switch (a.kind) {
    case kNormal: draw4<kNormal>(n, c1, key, pa, pb, a.nflags, w); break;
    case kUniform: draw4<kUniform>(n, c1, key, pa, pb, a.nflags, w); break;
    case kBernoulli: draw4<kBernoulli>(n, c1, key, pa, pb, a.nflags, w); break;
    case kExplicit:
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = (h0 + j < a.H) ? a.p0[ed * a.H + h0 + j] : 0.f;
        w[j] = (a.nflags & kFlagRelu) ? fmaxf(t, 0.f) : t;
      }
      break;
    default: w[0] = w[1] = w[2] = w[3] = 1.0f;
  }
}

// Lane L of a team -> its 4 channels.  A head takes lphp lanes (F / 4 rounded up to a power of two: the head sums
// are DPP butterflies); lanes past a head's F channels idle, so a width like F = 40 (lphp = 16) costs idle lanes but
// no padded bytes.  F / 4 a power of two: k0 = 4 L, the plain contiguous mapping.
__device__ __forceinline__ void lane_chunk(int L, int H, int F, int lphp, int& k0, bool& kin, int& hl) {
  const int head = L / lphp, j = L - head * lphp;
  kin = head < H && 4 * j < F;
  k0 = kin ? head * F + 4 * j : 0;
  hl = kin ? head : 0;
}

// The row output is written once and not read again by this launch: a non-temporal store keeps it from
// displacing ft in the 256 MB Infinity Cache (cfg5: ft 173 MB + out 173 MB do not fit together; measured
// 298 -> 289 us on the one-unit-per-team kernel).
__device__ __forceinline__ void store4_out(float* p, int k0, int D, bool vec, const float (&v)[4]) {
  if (vec) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p + k0));
    return;
  }
  store4(p, k0, D, vec, v);
}

// LDS hand-off between lanes of ONE wave: the LDS unit serves a wave's requests in
// order, so only the compiler has to be kept from reordering around the hand-off.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// LPE lanes per unit (H*F/4 rounded up to a power of two, 4..64); VEC: dwordx4 rows
template <int LPE, bool VEC>
__global__ __launch_bounds__(256) void gat_fwd_kernel(const GatArgs a) {
  extern __shared__ __align__(16) float lds[];
  const PhiloxKey key = resolve_epoch(a.key);
  constexpr int TEAMS_PER_BLOCK = 256 / LPE;
  const int H = a.H, F = a.F, HF = a.HF;
  const int team = threadIdx.x / LPE;
  const int c = threadIdx.x % LPE;
  const int team_lane0 = (int)(threadIdx.x & 63) - c;
  float* logit = lds + (size_t)team * (LPE * H);      // [LPE edges][H]
  const int unit = blockIdx.x * TEAMS_PER_BLOCK + team;
  if (unit >= a.n_units) return;   // teams are independent: no block-level barrier below

  int v, b, len, slot = -1;
  if (a.units) {
    const int4 q = *reinterpret_cast<const int4*>(a.units + unit);
    v = q.x; b = q.y; len = q.z; slot = q.w;
  } else {
    v = unit;
    b = a.indptr[v];
    len = a.indptr[v + 1] - b;
  }
  const int row = (slot >= 0) ? a.long_rows[v] : v;
  if (len > 24) __builtin_amdgcn_s_setprio(2);

  const int k0 = c * 4;                    // channels [k0, k0+4) of the H*F row
  const bool kin = k0 < HF;
  // head of each of the lane's 4 channels: all equal when F % 4 == 0 (the VEC path); with
  // an odd F a lane's channels can straddle two heads, so the softmax state is per channel
  int hq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) hq[q] = (k0 + q < HF) ? (k0 + q) / F : 0;
  const int hl = hq[0];
  const int nchunk = (H + 3) / 4;
  const __amdgpu_buffer_rsrc_t rft =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.ft), 0, (int)a.ft_bytes, 0x00020000);
  const bool ft_buf = VEC && a.ft_bytes != 0;

  constexpr int NS = VEC ? 1 : 4;          // softmax states per lane
  float m[NS], l[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) { m[q] = -INFINITY; l[q] = 0.f; }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};

  for (int i0 = 0; i0 < len; i0 += LPE) {
    const int nb = min(LPE, len - i0);
    // ---- phase 1: lane c computes the H logits of edge i0 + c ------------------------------
    wave_sync();
    int u = 0;
    if (c < nb) {
      const int p = b + i0 + c;
      u = a.indices[p];
      const int64_t ed = a.eid ? a.eid[p] : p;
      const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
      for (int cc = 0; cc < nchunk; ++cc) {
        float w[4];
        head_w4(a, key, n, ed, (uint32_t)cc, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = 4 * cc + j;
          if (h < H) {
            const float s = a.el[(int64_t)u * H + h] + a.er[(int64_t)row * H + h];
            const float lr = s > 0.f ? s : a.neg_slope * s;
            const float ns = a.nscale ? a.nscale[(int64_t)row * H + h] : 1.0f;
            const float lg = (w[j] * ns) * lr;
            logit[c * H + h] = lg;
          }
        }
      }
    }
    wave_sync();
    // ---- phase 2: fold the batch into this lane's head --------------------------------------
    if (kin) {
#pragma unroll
      for (int sI = 0; sI < NS; ++sI) {
        float bm = -INFINITY;
        for (int i = 0; i < nb; ++i) bm = fmaxf(bm, logit[i * H + hq[sI]]);
        const float mn = fmaxf(m[sI], bm);
        const float corr = __expf(m[sI] - mn);     // 0 on the first batch (m = -inf)
        l[sI] *= corr;
        if constexpr (VEC) {
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] *= corr;
        } else {
          acc[sI] *= corr;
        }
        m[sI] = mn;
      }
    }
    for (int i = 0; i < nb; i += 4) {
      int ui[4];
      float fv[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ui[j] = __builtin_amdgcn_ds_bpermute((team_lane0 + i + j) << 2, u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < nb && kin) {
          if (ft_buf) bufrow4(rft, ui[j], (uint32_t)HF * 4u, (uint32_t)k0 * 4u, fv[j]);
          else loadrow4(a.ft + (int64_t)ui[j] * HF + k0, k0, HF, VEC, fv[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < nb && kin) {
          if constexpr (VEC) {
            const float pe = __expf(logit[(i + j) * H + hl] - m[0]);
            l[0] += pe;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_fmaf(pe, fv[j][q], acc[q]);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float pe = __expf(logit[(i + j) * H + hq[q]] - m[q]);
              l[q] += pe;
              acc[q] = __builtin_fmaf(pe, fv[j][q], acc[q]);
            }
          }
        }
      }
    }
  }

  if (slot < 0) {
    // ---- whole row: normalise and store ------------------------------------------------------
    if (kin) {
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float lq = l[VEC ? 0 : q];
        o[q] = acc[q] * ((lq > 0.f) ? 1.0f / lq : 0.f);
      }
      store4_out(a.out + (int64_t)row * HF, k0, HF, VEC, o);
    }
    // the lane holding a head's first channel publishes that head's statistics: the attention
    // values and the backward pass are computed from them (no [E, H] tensor leaves this kernel)
    if (a.stats) {
#pragma unroll
      for (int q = 0; q < NS; ++q)
        if (k0 + q < HF && (k0 + q) % F == 0) {
          a.stats[(int64_t)row * 2 * H + hq[q]] = m[q];
          a.stats[(int64_t)row * 2 * H + H + hq[q]] = l[q];
        }
    }
  } else {
    // ---- segment: publish (acc, m, l) write-through, take a ticket ---------------------------
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(a.ws, 0, (int)a.ws_bytes, 0x00020000);
    const uint32_t base = (uint32_t)slot * ((uint32_t)a.ws_stride * 4u);
    if (kin) {
      store4_sc1(rws, base + (uint32_t)k0 * 4u, k0, HF, VEC, acc);
#pragma unroll
      for (int q = 0; q < NS; ++q)
        if (k0 + q < HF && (k0 + q) % F == 0) {
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m[q]), rws, (int)(base + (uint32_t)(HF + hq[q]) * 4u), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l[q]), rws, (int)(base + (uint32_t)(HF + H + hq[q]) * 4u), 0, 16);
        }
    }
    const int s0 = a.long_seg_ptr[v], s1 = a.long_seg_ptr[v + 1];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ticket = 0;
    if (c == 0)
      ticket = __hip_atomic_fetch_add(a.seg_counters + v, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_ds_bpermute(team_lane0 << 2, ticket);
    if (ticket != (s1 - s0) - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (c == 0) a.seg_counters[v] = 0;
    // merge the segment states in segment order
    float M[NS], L[NS];
    float A[4] = {0.f, 0.f, 0.f, 0.f};
    if (kin) {
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        M[q] = -INFINITY; L[q] = 0.f;
        for (int s = s0; s < s1; ++s) M[q] = fmaxf(M[q], a.ws[(int64_t)s * a.ws_stride + HF + hq[q]]);
      }
      for (int s = s0; s < s1; ++s) {
        const float* wr = a.ws + (int64_t)s * a.ws_stride;
        float t[4];
        load4(wr, k0, HF, VEC, t);
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const float sc = __expf(wr[HF + hq[q]] - M[q]);
          L[q] += wr[HF + H + hq[q]] * sc;
          if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 4; ++r) A[r] = __builtin_fmaf(t[r], sc, A[r]);
          } else {
            A[q] = __builtin_fmaf(t[q], sc, A[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float lq = L[VEC ? 0 : q];
        A[q] *= (lq > 0.f) ? 1.0f / lq : 0.f;
      }
      store4_out(a.out + (int64_t)row * HF, k0, HF, VEC, A);
    }
    if (a.stats && kin) {
#pragma unroll
      for (int q = 0; q < NS; ++q)
        if (k0 + q < HF && (k0 + q) % F == 0) {
          a.stats[(int64_t)row * 2 * H + hq[q]] = M[q];
          a.stats[(int64_t)row * 2 * H + H + hq[q]] = L[q];
        }
    }
  }
}

// ---- workgroup-cooperative forward (the default with a block plan, F % 4 == 0, H <= 16) --------
// gat_fwd_kernel gives a whole wave to one destination row: on a graph of mean in-degree 7 its
// edge-parallel phase runs 7 of 64 lanes through a chain of dependent round trips (unit -> ids -> el ->
// draw) while nothing is being gathered: 283 us at cfg5 for 1.5 GB, 5.4 TB/s, 5 waves per SIMD, each
// alive ~14 us for one row.  Here a WORKGROUP takes a batch of consecutive units of the plan (stag_plan
// block_ptr: <= 256 edges, <= 32 units):
//   phase 1  thread t <-> edge t of the batch: draws its H weights, forms its H noisy logits -> LDS
//            (every lane busy, one chain of round trips per batch instead of one per row);
//   phase 1b thread <-> (unit, head): max and sum of exp over the unit's logits in LDS; the logits are
//            replaced by p = exp(e - m) in place;
//   phase 2  a team of LPE lanes per unit (the block's units dealt round robin): a plain weighted gather
//            — ids and weights come from LDS, NR rows in flight — then normalise / publish.
// A unit's arithmetic does not depend on which batch it rides in: m = max over its edges, l = sum of
// exp in edge order, acc = fma(p_i, row_i, acc) in edge order — so shards reproduce the whole graph.
constexpr int kBlkEdges = STAG_BLOCK_EDGES, kBlkUnits = STAG_BLOCK_UNITS, kBlkMaxH = 16;
constexpr int kBlkThreads = STAG_BLOCK_EDGES;     // a thread per edge of the batch
static_assert(kBlkUnits <= 64 && kBlkThreads % 64 == 0 && kBlkThreads <= 1024, "the unit prefix is one wave's scan");
#ifndef STAG_GAT_DBG
#define STAG_GAT_DBG 0    // 16: per-stage timestamps into the stats buffer (tools/gat_trace.py)
#endif
#ifndef STAG_GAT_NR
#define STAG_GAT_NR 4     // rows in flight per team in phase 2
#endif
#ifndef STAG_GAT_BRANCHFREE
#define STAG_GAT_BRANCHFREE 1
#endif
// Rows in flight per team in the FORWARD's gather.  Round 3: with the loads of a round really issued together
// (STAG_GAT_BRANCHFREE) more of them is monotonically WORSE on cfg5 — 1: 222.2, 2: 238.1, 3: 249.6, 4: 252.8 us; the
// branchy form that serialised its "4 in flight" by accident: 228.5 us — and so is any other number of workgroups per CU
// than 4 (3: 246.9, 5: 239.0, 6: 253.9, 8: 255.8 us): a gather of 1-KB rows out of a 173 MB table wants ~16 rows in
// flight per CU and no more.  (128-thread workgroups over 128-edge batches, 4 / 6 / 8 / 12 per CU: 314.6 / 239.6 / 220.8 / 249.9 us —
// the same 16 waves per CU, the same time.)
#ifndef STAG_GAT_NR_FWD
#define STAG_GAT_NR_FWD 1
#endif
#ifndef STAG_GAT_NR_FWD_LOCAL
#define STAG_GAT_NR_FWD_LOCAL 2
#endif
// Round 4, re-measured on the kernel as it stands (three builds beside the shipped one in one call): on the one-GPU cfg5
// launch the count no longer matters — 1: 221.0-221.7, 2: 219.8-221.3, 3: 219.7, 4: 220.3 us — and on a SHARD-sized launch
// (an eighth of the graph: 900 batches, not fabric-bound: its time is the longest unit's chain of row round trips) it
// decides: 52.1 | 42.1 | 38.8 | 37.9 us for 1 | 2 | 3 | 4.  Rows of one chunk per lane (H * F <= 256: every BASELINE
// config) therefore keep 4 in flight; wider rows (2 or 4 chunks per lane: 4 rows would be 32-64 more registers) stay
// as they were.
#ifndef STAG_GAT_NR_FWD_NARROW
#define STAG_GAT_NR_FWD_NARROW 4
#endif
// (the one-gather backward keeps its branchy NR = 4 loop: branch-free loads there change nothing — cfg5 training step
//  632.5 against 632.1 us — and fewer rows per round cost it: NR = 2 640.5, NR = 1 658 us)

// (80 SGPRs: a CU admits 8 workgroups of 256 threads only up to that count — MI355X_MICROARCH.md,
//  "Residency"; the argument block alone would take ~100, the rest spill to lanes of a VGPR.)
#ifndef STAG_GAT_SGPR
#define STAG_GAT_SGPR 0
#endif
#if STAG_GAT_SGPR
#define STAG_GAT_SGPR_ATTR __attribute__((amdgpu_num_sgpr(STAG_GAT_SGPR)))
#else
#define STAG_GAT_SGPR_ATTR
#endif
#ifndef STAG_GAT_LDS_MIN
// Bytes of LDS a workgroup asks for at least: caps the workgroups a CU admits (160 KB / bytes).  The
// gather of 1-KB rows from a table beyond L2 is fastest with FEWER workgroups resident than registers
// and the kernel's own LDS would allow (cfg5, us per forward: 6 per CU 250, 5: 235, 4: 224.5, 3: 252,
// 2: 341; forward + backward with the two backward kernels at 4: 759, 5: 722, 6: 733).
#define STAG_GAT_LDS_MIN 40000      // forward: 4 workgroups per CU
#endif
#ifndef STAG_GAT_LDS_MIN_ONE
// the one-gather backward: no cap beyond its registers' (80 VGPRs: 6 waves per SIMD).  Round 4, 32000 | 16000 B: the
// one-GPU training step 621-628 | 618-624 us (no difference), the remote-rows source pass of a shard of eight 62.9 | 53.2 us
// (85 k rows of 1.5 edges: latency x concurrency, not the fabric); 48000: 689 us and 74.9 us.
#define STAG_GAT_LDS_MIN_ONE 16000
#endif
#ifndef STAG_GAT_LDS_MIN_BWD
#define STAG_GAT_LDS_MIN_BWD 32000  // backward passes: 5
#endif

// ---- half rows in the cooperative forward (stag_gat_fwd_half: DT = STAG_DTYPE_F16 / _BF16 of the kernel below) ------------
// a.ft points at fp16 / bf16 rows of H*F elements (a.ft_bytes: their extent in bytes when the descriptor reaches all
// of them); el, er, the in-norm factor, out, stats and the segment states are fp32 as before.  The gather — the one
// thing this launch waits for — is E x H*F*2 bytes.
// Rows in flight and workgroups per CU have knobs of their own (the fp32 values were tuned for 1-KB rows): none of
// them changes a bit of the result.  Round 10, cfg5 on bf16 rows, us per call (tools/ab_bench.py run --gat-half bf16,
// no noise): rows in flight 1 | 2 | 4 at 4 workgroups per CU 190.3 | 161.7 | 152.8; 4 | 5 | 6 workgroups per CU at 4
// rows 152.8 | 146.1 | 141.2 (6 needs <= 80 VGPRs: only with 4 merge states per round trip, which a shard-sized launch
// pays for — not taken).  Half-size rows out of a table that fits the Infinity Cache want MORE in flight, not fewer.
#ifndef STAG_GAT_HALF_NR
#define STAG_GAT_HALF_NR STAG_GAT_NR_FWD                 // rows of 2 or 4 chunks per lane, rows out of the Infinity Cache
#endif
#ifndef STAG_GAT_HALF_NR_LOCAL
#define STAG_GAT_HALF_NR_LOCAL STAG_GAT_NR_FWD_LOCAL     // ... XCD-local batches
#endif
#ifndef STAG_GAT_HALF_NR_NARROW
#define STAG_GAT_HALF_NR_NARROW STAG_GAT_NR_FWD_NARROW   // rows of one chunk per lane
#endif
#ifndef STAG_GAT_HALF_LDS_MIN
#define STAG_GAT_HALF_LDS_MIN 32000                      // bytes of LDS asked for at least: 160 KB / this = 5 workgroups per CU
#endif
#ifndef STAG_GAT_HALF_MERGE_NF
// Segment states of a long row fetched per round trip by the row's merge.  The fp32 kernel takes 12 (kGatMergeNF) in 121
// VGPRs; here 12 come to 143 (3 workgroups per CU instead of 4, and scratch when the allocator is held to 128), 8 to 93.
// The states are folded in segment order whatever the count: no bit depends on it.
#define STAG_GAT_HALF_MERGE_NF 8
#endif
constexpr int kGatHalfMergeNF = STAG_GAT_HALF_MERGE_NF;
constexpr int kGatRowF32 = 0;     // DT of fp32 rows: file-local, not a public dtype (stag_gat_fwd_half refuses ft_dtype 0)
static_assert(kGatRowF32 != STAG_DTYPE_F16 && kGatRowF32 != STAG_DTYPE_BF16, "the fp32 row type is none of the public half types");
typedef _Float16 gat_f16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int gat_u32x2_t __attribute__((ext_vector_type(2)));

// channels [k0, k0 + 4) of row u of ft: one 8-byte load (`buffer_load_dwordx2` behind the descriptor; a global load
// of 8 bytes past 2^24 rows or 4 GiB) widened exactly — bf16 by a shift / a mask, fp16 by
// v_cvt_f32_f16 (subnormals included: the conversion is an instruction, not arithmetic under the FP mode)
template <int DT>
__device__ __forceinline__ void gat_row4(const GatArgs& a, __amdgpu_buffer_rsrc_t rft, bool ft_buf, int u, int HF, int k0,
                                         float (&v)[4]) {
  static_assert(DT == STAG_DTYPE_F16 || DT == STAG_DTYPE_BF16, "half rows: fp16 or bf16");
  gat_u32x2_t t;
  if (ft_buf) {
    t = __builtin_amdgcn_raw_buffer_load_b64(rft, (int)(__umul24((uint32_t)u, (uint32_t)HF * 2u) + (uint32_t)k0 * 2u), 0, 0);
  } else {
    const char* p = reinterpret_cast<const char*>(a.ft) + ((int64_t)u * HF + k0) * 2;
    t = *reinterpret_cast<const gat_u32x2_t*>(p);
  }
  const uint32_t wd[2] = {t.x, t.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if constexpr (DT == STAG_DTYPE_BF16) {
      v[2 * i] = __uint_as_float(wd[i] << 16);
      v[2 * i + 1] = __uint_as_float(wd[i] & 0xFFFF0000u);
    } else {
      const gat_f16x2_t h = __builtin_bit_cast(gat_f16x2_t, wd[i]);
      v[2 * i] = (float)h.x;
      v[2 * i + 1] = (float)h.y;
    }
  }
}

// NRF: rows in flight per team in the gather — STAG_GAT_NR_FWD (1) when the rows come out of the Infinity Cache (cfg5: a
// 173 MB table, uniformly random sources), STAG_GAT_NR_FWD_LOCAL (2) when the batches are XCD-local (stag_plan_blocks_xcd*:
// the caller says so by a non-NULL plan->xcd_order) and the rows come out of an XCD's L2, where the gather is bound by
// latency, not by the fabric (round 4; tools/bench_configs.py --lib, us, 1 | 2 | 4 rows: PPI batch 4 x 256 356.6 | 334.2 |
// 337.3; cfg5 221.8 | 238.0 | 252.0).
// DT: the type of the ft rows — kGatRowF32 (stag_gat_fwd), STAG_DTYPE_F16 / STAG_DTYPE_BF16 (stag_gat_fwd_half).  It picks
// the row load (bufrow4 / loadrow4, or gat_row4<DT>) and the merge width (kGatMergeNF, or kGatHalfMergeNF) and nothing
// else: draws, logits, statistics, the fma chain in edge order, the padding of a round and the segment merge are ONE
// text, so the three agree bit for bit on rows that widen to the same floats.  The STAG_GAT_DBG & 16 trace and
// STAG_GAT_SGPR_ATTR apply to every DT; both are inert at their defaults (0: no trace code, no attribute).
// The body stays this __global__ function's own, with GatArgs its by-value parameter, and no part of it lives in a
// __device__ function, a macro or an included fragment.  This kernel is tuned to the VGPR, and every other way of
// sharing the text was tried and moved the register allocation (the DT parameter alone leaves all 27 instantiations'
// assembly and resource lines as they were when fp32 and half rows had a copy each; tools/device_code_diff.py):
//  - the body as a __device__ __forceinline__ gat_fwd_block_body<...>(a) under thin __global__ wrappers, GatArgs by
//    reference or by value: 12-15 of the 27 instantiations change — fp32 <64, 4, 2> 145 -> 147-149 VGPRs, fp32 <64, 2, 2>
//    78 -> 81 VGPRs and 6 -> 5 waves per SIMD, SGPR spills 34-36 -> 37-43;
//  - blk_prologue / blk_unit_of (the backward's helpers) for the batch prologue: the assembly of all 27 changes, their
//    resource lines do not;
//  - a gat_merge_row helper shared with gat_fwd_mc_block_kernel: the VGPR counts of 8 kernels move.
template <int DT, int LPE, int CPL, int NRF = STAG_GAT_NR_FWD>
__global__ __launch_bounds__(kBlkThreads) STAG_GAT_SGPR_ATTR void gat_fwd_block_kernel(const GatArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int H = a.H, F = a.F, HF = a.HF;
  float* s_w = lds;                                   // [kBlkEdges][H] logits, then p = exp(e - m)
  float* s_m = s_w + kBlkEdges * H;                   // [kBlkUnits][H]
  float* s_l = s_m + kBlkUnits * H;                   // [kBlkUnits][H]
  int* s_u = reinterpret_cast<int*>(s_l + kBlkUnits * H);   // [kBlkEdges] source row of each edge
  int* s_start = s_u + kBlkEdges;                     // [kBlkUnits + 1] first edge slot of each unit
  int4* s_unit = reinterpret_cast<int4*>(s_start + kBlkUnits + 4);   // [kBlkUnits] (row, start, len, slot); 16-B aligned
  const int t = threadIdx.x;
#if STAG_GAT_DBG & 16
  uint64_t* trace = reinterpret_cast<uint64_t*>(a.stats) + (int64_t)blockIdx.x * 8;
  if (t == 0) trace[0] = wall_clock64();
#define GAT_TS(i) if (t == 0) trace[i] = wall_clock64();
#else
#define GAT_TS(i)
#endif
  const int ub = a.block_ptr[blockIdx.x], nu = a.block_ptr[blockIdx.x + 1] - ub;

  // ---- the batch: unit records, edge-slot prefix -----------------------------------------------
  if (t < kBlkUnits) {
    int4 q = make_int4(0, 0, 0, -1);
    if (t < nu) q = *reinterpret_cast<const int4*>(a.units + ub + t);
    s_unit[t] = q;
    int incl = q.z;                                    // inclusive scan of the lengths over lanes 0..31
#pragma unroll
    for (int d = 1; d < kBlkUnits; d <<= 1) {
      const int up = __shfl_up(incl, d, kBlkUnits);          // lanes 0..kBlkUnits-1 of wave 0
      if (t >= d) incl += up;
    }
    s_start[t + 1] = incl;
    if (t == 0) s_start[0] = 0;
  }
  __syncthreads();
  GAT_TS(1)
  const int ne = s_start[nu];                          // edges of the batch (<= kBlkEdges by the plan)

  // ---- phase 1: thread t <-> edge slot t ---------------------------------------------------------
  uint32_t kmask = 0;                                  // attention dropout: bit h = head h of my edge survives
  if (t < ne) {
    int lo = 0, hi = nu;                               // unit j with s_start[j] <= t < s_start[j+1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_start[mid] <= t) lo = mid; else hi = mid;
    }
    const int4 q = s_unit[lo];
    const int row = (q.w >= 0) ? a.long_rows[q.x] : q.x;
    const int p = q.y + (t - s_start[lo]);
    const int u = a.indices[p];
    s_u[t] = u;
    const int64_t ed = a.eid ? a.eid[p] : p;
    const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
    const PhiloxKey key = resolve_epoch(a.key);
    const int nchunk = (H + 3) / 4;
    const bool h4 = (H & 3) == 0 && a.hvec;           // el / er / nscale rows as dwordx4 (one L1 lookup per 4 heads)
    for (int cc = 0; cc < nchunk; ++cc) {
      float w[4], sl4[4], sr4[4], ns4[4] = {1.f, 1.f, 1.f, 1.f};
      if (h4) {
        load4(a.el + (int64_t)u * H, 4 * cc, H, true, sl4);
        load4(a.er + (int64_t)row * H, 4 * cc, H, true, sr4);
        if (a.nscale) load4(a.nscale + (int64_t)row * H, 4 * cc, H, true, ns4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = 4 * cc + j;
          sl4[j] = h < H ? a.el[(int64_t)u * H + h] : 0.f;
          sr4[j] = h < H ? a.er[(int64_t)row * H + h] : 0.f;
          if (a.nscale && h < H) ns4[j] = a.nscale[(int64_t)row * H + h];
        }
      }
      head_w4(a, key, n, ed, (uint32_t)cc, w);
      if (a.drop_keep > 0.f) kmask |= drop_keep4(a, resolve_epoch(a.drop_key), n, (uint32_t)cc) << (4 * cc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int h = 4 * cc + j;
        if (h < H) {
          const float sL = sl4[j] + sr4[j];
          const float lr = sL > 0.f ? sL : a.neg_slope * sL;
          s_w[t * H + h] = (w[j] * ns4[j]) * lr;
        }
      }
    }
  }
  GAT_TS(2)
  __syncthreads();
  GAT_TS(3)

  // ---- phase 1b: thread <-> (unit, head): softmax statistics, logits -> p ---------------------------
  for (int i = t; i < nu * H; i += kBlkThreads) {
    const int j = i / H, h = i - j * H;
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float m = -INFINITY;
    for (int e = e0; e < e1; ++e) m = fmaxf(m, s_w[e * H + h]);
    float l = 0.f;
    for (int e = e0; e < e1; ++e) {
      const float pe = __expf(s_w[e * H + h] - m);
      s_w[e * H + h] = pe;
      l += pe;
    }
    s_m[i] = m;
    s_l[i] = l;
  }
  GAT_TS(4)
  __syncthreads();
  GAT_TS(5)
  if (a.drop_keep > 0.f) {       // (uniform) the softmax statistics saw every edge; the weighted sum sees the survivors
    if (t < ne) {
      for (int h = 0; h < H; ++h)
        s_w[t * H + h] = ((kmask >> h) & 1u) ? s_w[t * H + h] * a.drop_scale : 0.f;
    }
    __syncthreads();
  }

  // ---- phase 2: a team per unit, weighted gather -------------------------------------------------------
  // lane c owns CPL chunks of 4 channels: [4 (c + LPE j), +4), j < CPL  (H*F <= 256: one; up to 1024: 2 or 4)
  constexpr int TEAMS = kBlkThreads / LPE, NR = STAG_GAT_BRANCHFREE ? NRF : (CPL >= 4 ? 2 : STAG_GAT_NR);
  const int team = t / LPE, c = t % LPE;
  const int team_lane0 = (int)(t & 63) - c;
  int k0[CPL], hl[CPL];
  bool kin[CPL];
#pragma unroll
  for (int cj = 0; cj < CPL; ++cj) {
    lane_chunk(c + LPE * cj, H, F, a.lphp, k0[cj], kin[cj], hl[cj]);
  }
  const __amdgpu_buffer_rsrc_t rft =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.ft), 0, (int)a.ft_bytes, 0x00020000);
  const bool ft_buf = a.ft_bytes != 0;
  for (int j = team; j < nu; j += TEAMS) {
    const int4 q = s_unit[j];
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float acc[CPL][4];
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) acc[cj][0] = acc[cj][1] = acc[cj][2] = acc[cj][3] = 0.f;
#if STAG_GAT_BRANCHFREE
    // The NR gathers of a round are issued back to back with NO control flow between them: a round's source ids and
    // weights come out of LDS first (positions past the unit's end are clamped to its last edge and carry weight 0:
    // a repeated row, which the L1 serves), lanes without a chunk load chunk 0 and store nothing.  With the
    // `if (e + r < e1)` / `if (kin)` branches around each load the compiler could not count the loads in flight and put
    // `s_waitcnt vmcnt(0)` in front of every next LDS read: the "NR rows in flight" went out one at a time.
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4], pe[NR][CPL];
      int u[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int er = min(e + r, e1 - 1);
        u[r] = s_u[er];
#pragma unroll
        for (int cj = 0; cj < CPL; ++cj) {
          const float wv = s_w[er * H + (kin[cj] ? hl[cj] : 0)];
          pe[r][cj] = (e + r < e1) ? wv : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int cj = 0; cj < CPL; ++cj) {
          if constexpr (DT == kGatRowF32) {
            if (ft_buf) bufrow4(rft, u[r], (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
            else loadrow4(a.ft + (int64_t)u[r] * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
          } else {
            gat_row4<DT>(a, rft, ft_buf, u[r], HF, k0[cj], fv[r][cj]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int cj = 0; cj < CPL; ++cj) {
#pragma unroll
          for (int x = 0; x < 4; ++x) acc[cj][x] = __builtin_fmaf(pe[r][cj], fv[r][cj][x], acc[cj][x]);
        }
      }
    }
#else
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
          const int u = s_u[e + r];
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              if constexpr (DT == kGatRowF32) {
                if (ft_buf) bufrow4(rft, u, (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
                else loadrow4(a.ft + (int64_t)u * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
              } else {
                gat_row4<DT>(a, rft, ft_buf, u, HF, k0[cj], fv[r][cj]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              const float pe = s_w[(e + r) * H + hl[cj]];
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[cj][x] = __builtin_fmaf(pe, fv[r][cj][x], acc[cj][x]);
            }
          }
        }
      }
    }
#endif
    if (q.w < 0) {
      // ---- whole row: normalise and store --------------------------------------------------------
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) {
        if (!kin[cj]) continue;
        const float m = s_m[j * H + hl[cj]], l = s_l[j * H + hl[cj]];
        const float inv = (l > 0.f) ? 1.0f / l : 0.f;
        float o[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) o[x] = acc[cj][x] * inv;
        store4_out(a.out + (int64_t)q.x * HF, k0[cj], HF, true, o);
        if (a.stats && k0[cj] % F == 0 && !(STAG_GAT_DBG & 16)) {
          a.stats[(int64_t)q.x * 2 * H + hl[cj]] = m;
          a.stats[(int64_t)q.x * 2 * H + H + hl[cj]] = l;
        }
      }
      continue;
    }
    // ---- segment: publish (acc, m, l) write-through, take a ticket; the last arriver merges ----------
    const int v = q.x, slot = q.w, row = a.long_rows[v];
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(a.ws, 0, (int)a.ws_bytes, 0x00020000);
    const uint32_t base = (uint32_t)slot * ((uint32_t)a.ws_stride * 4u);
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      if (!kin[cj]) continue;
      store4_sc1(rws, base + (uint32_t)k0[cj] * 4u, k0[cj], HF, true, acc[cj]);
      if (k0[cj] % F == 0) {
        const float m = s_m[j * H + hl[cj]], l = s_l[j * H + hl[cj]];
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), rws, (int)(base + (uint32_t)(HF + hl[cj]) * 4u), 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l), rws, (int)(base + (uint32_t)(HF + H + hl[cj]) * 4u), 0, 16);
      }
    }
    const int s0 = a.long_seg_ptr[v], s1 = a.long_seg_ptr[v + 1];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ticket = 0;
    if (c == 0)
      ticket = __hip_atomic_fetch_add(a.seg_counters + v, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_ds_bpermute(team_lane0 << 2, ticket);
    if (ticket != (s1 - s0) - 1) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (c == 0) a.seg_counters[v] = 0;
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      if (!kin[cj]) continue;
      float M = -INFINITY, L = 0.f;
      float A[4] = {0.f, 0.f, 0.f, 0.f};
      // The merge is a chain on the launch's critical path when the launch is small (a shard of an 8-way partition: the
      // 13k-edge hub's 205 segment states, one L2 round trip each, were 97 of the shard's 145 us).  The states are fetched
      // kGatMergeNF (12; half rows kGatHalfMergeNF, 8) at a time — independent loads, clamped to the last segment instead of
      // branching — and folded in segment order as before, so the row's bits do not change.  12 states are 121 VGPRs on fp32
      // rows: free, because the kernel's LDS request (STAG_GAT_LDS_MIN) caps a SIMD at 4 waves, which registers allow up to
      // 128 (one-GPU cfg5 with 4 | 8 | 12 at a time: 223.8 | 223.5 | 223.1 us; the hub's shard of eight: 70.2 | 57.4 | 53.0 us).
      // (wider rows, CPL chunks per lane: their register budget has no room, one state at a time as before)
      constexpr int NFM = CPL == 1 ? (DT == kGatRowF32 ? kGatMergeNF : kGatHalfMergeNF) : 1;
      // the row's maximum per head.  Where the team's lanes are exactly H heads x F/4 lanes (cfg5: 8 x 8 = 64), the F/4
      // lanes of a head take every (F/4)-th segment each and exchange their maxima: 205 states in 4 round trips
      // instead of 26 (a maximum does not care about the order)
      const int lph = a.lphp;
      if (CPL == 1 && lph >= 2 && lph * 4 == F && H * lph == LPE) {
        const int g = c & (lph - 1);
        for (int sg = s0 + g; sg < s1; sg += 2 * NFM * lph) {
          float mm[2 * NFM];
#pragma unroll
          for (int i = 0; i < 2 * NFM; ++i)
            mm[i] = a.ws[(int64_t)min(sg + i * lph, s1 - 1) * a.ws_stride + HF + hl[cj]];
#pragma unroll
          for (int i = 0; i < 2 * NFM; ++i) M = fmaxf(M, mm[i]);
        }
        for (int d = 1; d < lph; d <<= 1) M = fmaxf(M, __shfl_xor(M, d));
      } else {
        for (int sg = s0; sg < s1; sg += 2 * NFM) {
          float mm[2 * NFM];
#pragma unroll
          for (int i = 0; i < 2 * NFM; ++i)
            mm[i] = a.ws[(int64_t)min(sg + i, s1 - 1) * a.ws_stride + HF + hl[cj]];
#pragma unroll
          for (int i = 0; i < 2 * NFM; ++i) M = fmaxf(M, mm[i]);
        }
      }
      for (int sg = s0; sg < s1; sg += NFM) {
        float tt[NFM][4], ms[NFM], ls[NFM];
#pragma unroll
        for (int i = 0; i < NFM; ++i) {
          const float* wr = a.ws + (int64_t)min(sg + i, s1 - 1) * a.ws_stride;
          load4(wr, k0[cj], HF, true, tt[i]);
          ms[i] = wr[HF + hl[cj]];
          ls[i] = wr[HF + H + hl[cj]];
        }
#pragma unroll
        for (int i = 0; i < NFM; ++i) {
          if (sg + i < s1) {
            const float sc = __expf(ms[i] - M);
            L += ls[i] * sc;
#pragma unroll
            for (int x = 0; x < 4; ++x) A[x] = __builtin_fmaf(tt[i][x], sc, A[x]);
          }
        }
      }
      const float inv = (L > 0.f) ? 1.0f / L : 0.f;
#pragma unroll
      for (int x = 0; x < 4; ++x) A[x] *= inv;
      store4_out(a.out + (int64_t)row * HF, k0[cj], HF, true, A);
      if (a.stats && k0[cj] % F == 0 && !(STAG_GAT_DBG & 16)) {
        a.stats[(int64_t)row * 2 * H + hl[cj]] = M;
        a.stats[(int64_t)row * 2 * H + H + hl[cj]] = L;
      }
    }
  }
  GAT_TS(6)
}

// ---- Monte-Carlo form of the cooperative forward (stag_gat_fwd_mc) -------------------------------------------------
// The reference's models average S noisy passes (stag/models.py:45-55, :67-68); on a first layer every pass gathers the
// same ft rows and only the H-wide draws differ.  gat_fwd_mc_block_kernel is gat_fwd_block_kernel<kGatRowF32, ...> carrying `ns` <= SP
// samples per launch: phase 1 draws the H weights of every sample from one load of el / er / the source id (sample s
// at the key advanced by s * stride), phase 1b forms each sample's softmax statistics, phase 2 gathers each row ONCE
// and folds it into SP accumulator sets.  Per sample the arithmetic, its order and the padding of a round are those of
// gat_fwd_block_kernel<kGatRowF32, LPE, CPL, NRF> — sample s is the single-sample launch at offset + s * stride, bit for bit.
// LDS: ns x (256 H + 64 H) floats of logits and statistics + the batch records, padded to STAG_GAT_LDS_MIN as the
// single-sample kernel is.  Segment states: [slot][wsp][ws_stride], one ticket per segment for all its samples; the last
// arriver merges sample by sample (the merge's registers are the single-sample kernel's, not SP times them).
#ifndef STAG_GAT_MC_SP
#define STAG_GAT_MC_SP 4          // samples per pass, rows of 1 or 2 chunks per lane (H * lanes_per_head <= 128)
#endif
#ifndef STAG_GAT_MC_SP_WIDE
#define STAG_GAT_MC_SP_WIDE 2     // samples per pass, rows of 4 chunks per lane (PPI's 4 x 256): 16 accumulators each
#endif
constexpr int kGatMcMaxSP = 4;    // the workspace is sized for this many samples (stag_gat_fwd_mc_workspace_bytes)
static_assert(STAG_GAT_MC_SP >= 1 && STAG_GAT_MC_SP <= kGatMcMaxSP && STAG_GAT_MC_SP_WIDE >= 1 &&
              STAG_GAT_MC_SP_WIDE <= kGatMcMaxSP, "samples per pass: 1..4");

struct GatMcArgs {
  GatArgs a;               // a.key: sample 0 of this pass; a.out / a.stats: sample 0's rows
  uint64_t stride;         // offset step between consecutive samples
  int64_t out_stride;      // floats between two samples' out
  int64_t stats_stride;    // floats between two samples' stats
  int32_t ns;              // samples of this pass, 1..SP
  int32_t wsp;             // segment states per slot of the workspace: min(n_samples, SP)
};

template <int LPE, int CPL, int NRF, int SP>
__global__ __launch_bounds__(kBlkThreads) void gat_fwd_mc_block_kernel(const GatMcArgs g) {
  extern __shared__ __align__(16) float lds[];
  const GatArgs& a = g.a;
  const int H = a.H, F = a.F, HF = a.HF, ns = g.ns;
  const int EH = kBlkEdges * H, UH = kBlkUnits * H;   // floats per sample: logits, statistics
  float* s_w = lds;                                   // [ns][kBlkEdges][H] logits, then p = exp(e - m)
  float* s_m = s_w + ns * EH;                         // [ns][kBlkUnits][H]
  float* s_l = s_m + ns * UH;                         // [ns][kBlkUnits][H]
  int* s_u = reinterpret_cast<int*>(s_l + ns * UH);   // [kBlkEdges] source row of each edge
  int* s_start = s_u + kBlkEdges;                     // [kBlkUnits + 1] first edge slot of each unit
  int4* s_unit = reinterpret_cast<int4*>(s_start + kBlkUnits + 4);   // [kBlkUnits] (row, start, len, slot); 16-B aligned
  const int t = threadIdx.x;
  const int ub = a.block_ptr[blockIdx.x], nu = a.block_ptr[blockIdx.x + 1] - ub;

  // ---- the batch: unit records, edge-slot prefix -----------------------------------------------
  if (t < kBlkUnits) {
    int4 q = make_int4(0, 0, 0, -1);
    if (t < nu) q = *reinterpret_cast<const int4*>(a.units + ub + t);
    s_unit[t] = q;
    int incl = q.z;
#pragma unroll
    for (int d = 1; d < kBlkUnits; d <<= 1) {
      const int up = __shfl_up(incl, d, kBlkUnits);
      if (t >= d) incl += up;
    }
    s_start[t + 1] = incl;
    if (t == 0) s_start[0] = 0;
  }
  __syncthreads();
  const int ne = s_start[nu];

  // ---- phase 1: thread t <-> edge slot t; el / er / the source id once, the draws of every sample --------------
  if (t < ne) {
    int lo = 0, hi = nu;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_start[mid] <= t) lo = mid; else hi = mid;
    }
    const int4 q = s_unit[lo];
    const int row = (q.w >= 0) ? a.long_rows[q.x] : q.x;
    const int p = q.y + (t - s_start[lo]);
    const int u = a.indices[p];
    s_u[t] = u;
    const int64_t ed = a.eid ? a.eid[p] : p;
    const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
    const PhiloxKey key = resolve_epoch(a.key);
    const int nchunk = (H + 3) / 4;
    const bool h4 = (H & 3) == 0 && a.hvec;
    for (int cc = 0; cc < nchunk; ++cc) {
      float sl4[4], sr4[4];
      if (h4) {
        load4(a.el + (int64_t)u * H, 4 * cc, H, true, sl4);
        load4(a.er + (int64_t)row * H, 4 * cc, H, true, sr4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = 4 * cc + j;
          sl4[j] = h < H ? a.el[(int64_t)u * H + h] : 0.f;
          sr4[j] = h < H ? a.er[(int64_t)row * H + h] : 0.f;
        }
      }
      for (int s = 0; s < ns; ++s) {
        float w[4];
        head_w4(a, key_plus(key, (uint64_t)s * g.stride), n, ed, (uint32_t)cc, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = 4 * cc + j;
          if (h < H) {
            const float sL = sl4[j] + sr4[j];
            const float lr = sL > 0.f ? sL : a.neg_slope * sL;
            s_w[s * EH + t * H + h] = (w[j] * 1.0f) * lr;    // (the single-sample form with no in-norm factor)
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 1b: thread <-> (sample, unit, head): softmax statistics, logits -> p -----------------------------
  for (int i = t; i < ns * nu * H; i += kBlkThreads) {
    const int s = i / (nu * H), jh = i - s * (nu * H);
    const int j = jh / H, h = jh - j * H;
    float* w = s_w + s * EH;
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float m = -INFINITY;
    for (int e = e0; e < e1; ++e) m = fmaxf(m, w[e * H + h]);
    float l = 0.f;
    for (int e = e0; e < e1; ++e) {
      const float pe = __expf(w[e * H + h] - m);
      w[e * H + h] = pe;
      l += pe;
    }
    s_m[s * UH + jh] = m;
    s_l[s * UH + jh] = l;
  }
  __syncthreads();

  // ---- phase 2: a team per unit; each row gathered once, folded into SP accumulator sets ------------------------
  constexpr int TEAMS = kBlkThreads / LPE, NR = NRF;
  const int team = t / LPE, c = t % LPE;
  const int team_lane0 = (int)(t & 63) - c;
  int k0[CPL], hl[CPL];
  bool kin[CPL];
#pragma unroll
  for (int cj = 0; cj < CPL; ++cj) lane_chunk(c + LPE * cj, H, F, a.lphp, k0[cj], kin[cj], hl[cj]);
  const __amdgpu_buffer_rsrc_t rft =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.ft), 0, (int)a.ft_bytes, 0x00020000);
  const bool ft_buf = a.ft_bytes != 0;
  for (int j = team; j < nu; j += TEAMS) {
    const int4 q = s_unit[j];
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float acc[SP][CPL][4];
#pragma unroll
    for (int s = 0; s < SP; ++s)
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) acc[s][cj][0] = acc[s][cj][1] = acc[s][cj][2] = acc[s][cj][3] = 0.f;
    // (the round of gat_fwd_block_kernel's branch-free form: NR loads issued back to back, positions past the unit's
    //  end clamped to its last edge with weight 0; samples past ns carry weight 0 and are never stored)
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4], pe[NR][SP][CPL];
      int u[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int er = min(e + r, e1 - 1);
        u[r] = s_u[er];
#pragma unroll
        for (int s = 0; s < SP; ++s) {
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            const float wv = (s < ns) ? s_w[s * EH + er * H + (kin[cj] ? hl[cj] : 0)] : 0.f;
            pe[r][s][cj] = (e + r < e1) ? wv : 0.f;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int cj = 0; cj < CPL; ++cj) {
          if (ft_buf) bufrow4(rft, u[r], (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
          else loadrow4(a.ft + (int64_t)u[r] * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int s = 0; s < SP; ++s) {
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
#pragma unroll
            for (int x = 0; x < 4; ++x) acc[s][cj][x] = __builtin_fmaf(pe[r][s][cj], fv[r][cj][x], acc[s][cj][x]);
          }
        }
      }
    }
    if (q.w < 0) {
      // ---- whole row: normalise and store every sample ---------------------------------------------------------
#pragma unroll
      for (int s = 0; s < SP; ++s) {
        if (s >= ns) break;
        float* out_s = a.out + (int64_t)s * g.out_stride;
#pragma unroll
        for (int cj = 0; cj < CPL; ++cj) {
          if (!kin[cj]) continue;
          const float m = s_m[s * UH + j * H + hl[cj]], l = s_l[s * UH + j * H + hl[cj]];
          const float inv = (l > 0.f) ? 1.0f / l : 0.f;
          float o[4];
#pragma unroll
          for (int x = 0; x < 4; ++x) o[x] = acc[s][cj][x] * inv;
          store4_out(out_s + (int64_t)q.x * HF, k0[cj], HF, true, o);
          if (a.stats && k0[cj] % F == 0) {
            float* st = a.stats + (int64_t)s * g.stats_stride;
            st[(int64_t)q.x * 2 * H + hl[cj]] = m;
            st[(int64_t)q.x * 2 * H + H + hl[cj]] = l;
          }
        }
      }
      continue;
    }
    // ---- segment: publish (acc, m, l) of every sample write-through, take ONE ticket; the last arriver merges ------
    const int v = q.x, slot = q.w, row = a.long_rows[v];
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(a.ws, 0, (int)a.ws_bytes, 0x00020000);
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      if (s >= ns) break;
      const uint32_t base = ((uint32_t)slot * (uint32_t)g.wsp + (uint32_t)s) * ((uint32_t)a.ws_stride * 4u);
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) {
        if (!kin[cj]) continue;
        store4_sc1(rws, base + (uint32_t)k0[cj] * 4u, k0[cj], HF, true, acc[s][cj]);
        if (k0[cj] % F == 0) {
          const float m = s_m[s * UH + j * H + hl[cj]], l = s_l[s * UH + j * H + hl[cj]];
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), rws, (int)(base + (uint32_t)(HF + hl[cj]) * 4u), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l), rws, (int)(base + (uint32_t)(HF + H + hl[cj]) * 4u), 0, 16);
        }
      }
    }
    const int s0 = a.long_seg_ptr[v], s1 = a.long_seg_ptr[v + 1];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ticket = 0;
    if (c == 0)
      ticket = __hip_atomic_fetch_add(a.seg_counters + v, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_ds_bpermute(team_lane0 << 2, ticket);
    if (ticket != (s1 - s0) - 1) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (c == 0) a.seg_counters[v] = 0;
    // the merge of gat_fwd_block_kernel<kGatRowF32, LPE, CPL, NRF> (fp32 rows: kGatMergeNF states per round trip), one sample
    // at a time: segment sg of sample s is state sg * wsp + s
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const float* ws = a.ws + (int64_t)s * a.ws_stride;
      const int64_t wst = (int64_t)g.wsp * a.ws_stride;
      float* out_s = a.out + (int64_t)s * g.out_stride;
#pragma unroll
      for (int cj = 0; cj < CPL; ++cj) {
        if (!kin[cj]) continue;
        float M = -INFINITY, L = 0.f;
        float A[4] = {0.f, 0.f, 0.f, 0.f};
        constexpr int NFM = CPL == 1 ? kGatMergeNF : 1;
        const int lph = a.lphp;
        if (CPL == 1 && lph >= 2 && lph * 4 == F && H * lph == LPE) {
          const int gq = c & (lph - 1);
          for (int sg = s0 + gq; sg < s1; sg += 2 * NFM * lph) {
            float mm[2 * NFM];
#pragma unroll
            for (int i = 0; i < 2 * NFM; ++i) mm[i] = ws[(int64_t)min(sg + i * lph, s1 - 1) * wst + HF + hl[cj]];
#pragma unroll
            for (int i = 0; i < 2 * NFM; ++i) M = fmaxf(M, mm[i]);
          }
          for (int d = 1; d < lph; d <<= 1) M = fmaxf(M, __shfl_xor(M, d));
        } else {
          for (int sg = s0; sg < s1; sg += 2 * NFM) {
            float mm[2 * NFM];
#pragma unroll
            for (int i = 0; i < 2 * NFM; ++i) mm[i] = ws[(int64_t)min(sg + i, s1 - 1) * wst + HF + hl[cj]];
#pragma unroll
            for (int i = 0; i < 2 * NFM; ++i) M = fmaxf(M, mm[i]);
          }
        }
        for (int sg = s0; sg < s1; sg += NFM) {
          float tt[NFM][4], ms[NFM], ls[NFM];
#pragma unroll
          for (int i = 0; i < NFM; ++i) {
            const float* wr = ws + (int64_t)min(sg + i, s1 - 1) * wst;
            load4(wr, k0[cj], HF, true, tt[i]);
            ms[i] = wr[HF + hl[cj]];
            ls[i] = wr[HF + H + hl[cj]];
          }
#pragma unroll
          for (int i = 0; i < NFM; ++i) {
            if (sg + i < s1) {
              const float sc = __expf(ms[i] - M);
              L += ls[i] * sc;
#pragma unroll
              for (int x = 0; x < 4; ++x) A[x] = __builtin_fmaf(tt[i][x], sc, A[x]);
            }
          }
        }
        const float inv = (L > 0.f) ? 1.0f / L : 0.f;
#pragma unroll
        for (int x = 0; x < 4; ++x) A[x] *= inv;
        store4_out(out_s + (int64_t)row * HF, k0[cj], HF, true, A);
        if (a.stats && k0[cj] % F == 0) {
          float* st = a.stats + (int64_t)s * g.stats_stride;
          st[(int64_t)row * 2 * H + hl[cj]] = M;
          st[(int64_t)row * 2 * H + H + hl[cj]] = L;
        }
      }
    }
  }
}

// Attention values a[eid, h] = exp(logit - m[v,h]) / l[v,h] (get_attention=True,
// stag/zoo/gat.py:146-147) from the row statistics of gat_fwd_kernel: 8 lanes per unit of the
// plan, a lane per edge; the noisy logit is redrawn from its counters.
__global__ __launch_bounds__(256) void gat_attn_kernel(const GatArgs a) {
  const PhiloxKey key = resolve_epoch(a.key);
  const int c = threadIdx.x & 7;
  const int unit = blockIdx.x * 32 + (threadIdx.x >> 3);
  if (unit >= a.n_units) return;
  int v, b, len, slot = -1;
  if (a.units) {
    const int4 q = *reinterpret_cast<const int4*>(a.units + unit);
    v = q.x; b = q.y; len = q.z; slot = q.w;
  } else {
    v = unit; b = a.indptr[v]; len = a.indptr[v + 1] - b;
  }
  const int row = (slot >= 0) ? a.long_rows[v] : v;
  const int H = a.H, nchunk = (H + 3) / 4;
  const float* st = a.stats + (int64_t)row * 2 * H;
  for (int p = b + c; p < b + len; p += 8) {
    const int u = a.indices[p];
    const int64_t ed = a.eid ? a.eid[p] : p;
    const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
    for (int cc = 0; cc < nchunk; ++cc) {
      float w[4], at[4];
      head_w4(a, key, n, ed, (uint32_t)cc, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int h = 4 * cc + j;
        at[j] = 0.f;
        if (h < H) {
          const float e = a.el[(int64_t)u * H + h] + a.er[(int64_t)row * H + h];
          const float lr = e > 0.f ? e : a.neg_slope * e;
          const float ns = a.nscale ? a.nscale[(int64_t)row * H + h] : 1.0f;
          at[j] = __expf((w[j] * ns) * lr - st[h]) / st[H + h];
        }
      }
      if ((H & 3) == 0) {       // one 16-byte store per head chunk
        *reinterpret_cast<float4*>(a.attn + ed * H + 4 * cc) = make_float4(at[0], at[1], at[2], at[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * cc + j < H) a.attn[ed * H + 4 * cc + j] = at[j];
      }
    }
  }
}

// ---- backward, per-edge part ---------------------------------------------------------------
// Given G = dL/dout[v,h,:] and gdo[v,h] = <G[v,h,:], out[v,h,:]>:
//     da[p,h] = <G[v,h,:], ft[u_p,h,:]>
//     ds[p,h] = a[p,h] * (da[p,h] - gdo[v,h])                      softmax backward
//     de[p,h] = ds[p,h] * w[p,h] * lrelu'(el[u_p,h] + er[v,h])     -> d el / d er by segment sums
//     dw[p,h] = ds[p,h] * lrelu(el[u_p,h] + er[v,h]) * nscale      (explicit / materialised w)
// Edges are independent, so segments need no merge.  Phase 1 (edge-parallel) regenerates the
// weights and parks a, w*lrelu', lrelu in LDS; phase 2 (channel-parallel) gathers ft rows,
// takes the dot with G, reduces it over the F/4 lanes of a head and lets the head's first
// lane write.  Requires F % 4 == 0 and F/4 a power of two.
struct GatBwdArgs {
  GatArgs f;
  const float* g;      // [n_rows, H*F]
  const float* gdo;    // [n_rows, H] = <g[v,h,:], out[v,h,:]>, or null: computed here from `out`
  const float* out;    // [n_rows, H*F] forward output (used when gdo is null)
  float* de;           // [E, H] by edge id
  float* dw;           // [E, H] by edge id, or null
};

template <int LPE>
__global__ __launch_bounds__(256) void gat_bwd_edge_kernel(const GatBwdArgs ba) {
  extern __shared__ __align__(16) float lds[];
  const GatArgs& a = ba.f;
  const PhiloxKey key = resolve_epoch(a.key);
  constexpr int TEAMS_PER_BLOCK = 256 / LPE;
  const int H = a.H, F = a.F, HF = a.HF;
  const int team = threadIdx.x / LPE;
  const int c = threadIdx.x % LPE;
  const int team_lane0 = (int)(threadIdx.x & 63) - c;
  float* sa = lds + (size_t)team * (3 * LPE * H);   // [LPE][H] attention
  float* sc1 = sa + LPE * H;                         // [LPE][H] w * nscale * lrelu'
  float* sc2 = sc1 + LPE * H;                        // [LPE][H] lrelu * nscale
  const int unit = blockIdx.x * TEAMS_PER_BLOCK + team;
  if (unit >= a.n_units) return;

  int v, b, len, slot = -1;
  if (a.units) {
    const int4 q = *reinterpret_cast<const int4*>(a.units + unit);
    v = q.x; b = q.y; len = q.z; slot = q.w;
  } else {
    v = unit;
    b = a.indptr[v];
    len = a.indptr[v + 1] - b;
  }
  const int row = (slot >= 0) ? a.long_rows[v] : v;
  const int k0 = c * 4;
  const bool kin = k0 < HF;
  const int hl = kin ? k0 / F : 0;
  const int nchunk = (H + 3) / 4;
  const int lanes_per_head = F / 4;

  // sum over the F/4 lanes of a head: DPP inside a row of 16 lanes, bpermute only beyond
  auto head_sum = [&](float x) {
    if (lanes_per_head >= 2) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
    if (lanes_per_head >= 4) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));
    if (lanes_per_head >= 8) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, true));
    if (lanes_per_head >= 16) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xF, 0xF, true));
    if (lanes_per_head >= 32) x += __shfl_xor(x, 16);
    if (lanes_per_head >= 64) x += __shfl_xor(x, 32);
    return x;
  };
  float gv[4] = {0.f, 0.f, 0.f, 0.f};
  float gdo = 0.f;
  if (kin) load4(ba.g + (int64_t)row * HF, k0, HF, true, gv);
  if (ba.gdo) {
    if (kin) gdo = ba.gdo[(int64_t)row * H + hl];
  } else {                      // <g[v,h,:], out[v,h,:]> of the unit's own row
    float ov[4] = {0.f, 0.f, 0.f, 0.f};
    if (kin) load4(ba.out + (int64_t)row * HF, k0, HF, true, ov);
    gdo = head_sum((gv[0] * ov[0] + gv[1] * ov[1]) + (gv[2] * ov[2] + gv[3] * ov[3]));
  }

  for (int i0 = 0; i0 < len; i0 += LPE) {
    const int nb = min(LPE, len - i0);
    wave_sync();
    int u = 0, edl = 0;
    if (c < nb) {
      const int p = b + i0 + c;
      u = a.indices[p];
      const int64_t ed = a.eid ? a.eid[p] : p;
      edl = (int)ed;
      const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
      for (int cc = 0; cc < nchunk; ++cc) {
        float w[4], at4[4] = {0.f, 0.f, 0.f, 0.f};
        head_w4(a, key, n, ed, (uint32_t)cc, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int h = 4 * cc + j;
          if (h < H) {
            const float e = a.el[(int64_t)u * H + h] + a.er[(int64_t)row * H + h];
            const float ns = a.nscale ? a.nscale[(int64_t)row * H + h] : 1.0f;
            const float lr = e > 0.f ? e : a.neg_slope * e;
            // the attention value, from the row statistics of the forward pass
            const float at = __expf((w[j] * ns) * lr - a.stats[(int64_t)row * 2 * H + h]) /
                             a.stats[(int64_t)row * 2 * H + H + h];
            sa[c * H + h] = at;
            at4[j] = at;
            sc1[c * H + h] = (w[j] * ns) * (e > 0.f ? 1.0f : a.neg_slope);
            sc2[c * H + h] = lr * ns;
          }
        }
        if (a.attn) {      // by-product: the weights of the d ft aggregation, 16 bytes per head chunk
          if ((H & 3) == 0) {
            *reinterpret_cast<float4*>(a.attn + ed * H + 4 * cc) = make_float4(at4[0], at4[1], at4[2], at4[3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * cc + j < H) a.attn[ed * H + 4 * cc + j] = at4[j];
          }
        }
      }
    }
    wave_sync();
    for (int i = 0; i < nb; i += 4) {      // four rows in flight
      int ui[4], ei[4];
      float fv[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ui[j] = __builtin_amdgcn_ds_bpermute((team_lane0 + i + j) << 2, u);
        ei[j] = __builtin_amdgcn_ds_bpermute((team_lane0 + i + j) << 2, edl);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < nb && kin) load4(a.ft + (int64_t)ui[j] * HF, k0, HF, true, fv[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float dot = 0.f;
        if (i + j < nb && kin)
          dot = (gv[0] * fv[j][0] + gv[1] * fv[j][1]) + (gv[2] * fv[j][2] + gv[3] * fv[j][3]);
        dot = head_sum(dot);
        if (i + j < nb && kin && (k0 % F) == 0) {
          const float ds = sa[(i + j) * H + hl] * (dot - gdo);
          ba.de[(int64_t)ei[j] * H + hl] = ds * sc1[(i + j) * H + hl];
          if (ba.dw) ba.dw[(int64_t)ei[j] * H + hl] = ds * sc2[(i + j) * H + hl];
        }
      }
    }
  }
}

// ---- workgroup-cooperative backward (stag_gat_bwd) -------------------------------------------------
// Two passes over batches of units, each shaped like gat_fwd_block_kernel:
//   edge pass (destination-major batches): phase 1, thread <-> edge: the weight redrawn from its
//     counters, a = exp(e - m[v]) / l[v] from the forward's statistics, c1 = w ns lrelu'(s),
//     (c2 = lrelu(s) ns) -> LDS; phase 2, a team per unit: G[v] and gdo[v] = <G[v], out[v]> in registers,
//     per in-edge the ft row, <G[v,h,:], ft[u,h,:]> reduced over the head's lanes, ds = a (da - gdo),
//     de = ds c1 -> LDS; phase 3, thread <-> edge: (a, de) written BY FORWARD POSITION, [E, 2H], coalesced;
//     thread <-> (unit, head): d er[v,h] = sum of de over the unit (segments: a partial per segment).
//   source pass (source-major batches of the transposed CSR): phase 1, thread <-> out-edge: (a, de) of
//     its forward position (csr_t.nidx) -> LDS; d el[u,h] = sum of de; phase 2: d ft[u] = sum a G[v],
//     the forward kernel's weighted gather with G in the place of ft.
// Long rows (segments) leave partial sums in the plan's workspace; gat_seg_finish_kernel adds them in
// segment order (deterministic; nothing is accumulated with atomics).
struct GatBwdBlkArgs {
  GatArgs f;             // edge pass: the forward's arguments (graph, el, er, ft, noise, stats, plan batches)
  const float* g;        // [n_rows, H*F]
  const float* out;      // [n_rows, H*F] forward output
  float* ade;            // [E, 2H] by forward position: a[H] then de[H]
  float* d_er;           // [n_rows, H]
  float* dw;             // [E, H] by edge id, or null
  float* ws;             // segment partials of d er: [n_seg][H]
};

// the batch a workgroup owns: unit records and the edge-slot prefix in LDS; returns the unit count
__device__ __forceinline__ int blk_prologue(const stag_unit* units, const int32_t* block_ptr, int4* s_unit,
                                            int* s_start) {
  const int t = threadIdx.x;
  const int ub = block_ptr[blockIdx.x], nu = block_ptr[blockIdx.x + 1] - ub;
  if (t < kBlkUnits) {
    int4 q = make_int4(0, 0, 0, -1);
    if (t < nu) q = *reinterpret_cast<const int4*>(units + ub + t);
    s_unit[t] = q;
    int incl = q.z;
#pragma unroll
    for (int d = 1; d < kBlkUnits; d <<= 1) {
      const int up = __shfl_up(incl, d, kBlkUnits);          // lanes 0..kBlkUnits-1 of wave 0
      if (t >= d) incl += up;
    }
    s_start[t + 1] = incl;
    if (t == 0) s_start[0] = 0;
  }
  __syncthreads();
  return nu;
}

__device__ __forceinline__ int blk_unit_of(const int* s_start, int nu, int t) {
  int lo = 0, hi = nu;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s_start[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// sum over the F/4 lanes of a head (lanes_per_head a power of two): DPP inside a row of 16 lanes
__device__ __forceinline__ float gat_head_sum(float x, int lanes_per_head) {
  if (lanes_per_head >= 2) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
  if (lanes_per_head >= 4) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));
  if (lanes_per_head >= 8) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, true));
  if (lanes_per_head >= 16) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xF, 0xF, true));
  if (lanes_per_head >= 32) x += __shfl_xor(x, 16);
  if (lanes_per_head >= 64) x += __shfl_xor(x, 32);
  return x;
}

template <int LPE, int CPL>
__global__ __launch_bounds__(kBlkThreads) void gat_bwd_edge_block_kernel(const GatBwdBlkArgs ba) {
  extern __shared__ __align__(16) float lds[];
  const GatArgs& a = ba.f;
  const int H = a.H, F = a.F, HF = a.HF;
  float* s_a = lds;                                   // [kBlkEdges][H] attention
  float* s_c1 = s_a + kBlkEdges * H;                  // [kBlkEdges][H] w ns lrelu'(s), then de
  float* s_c2 = s_c1 + kBlkEdges * H;                 // [kBlkEdges][H] lrelu(s) ns, then dw (only when wanted)
  int* s_u = reinterpret_cast<int*>(s_c2 + (ba.dw ? kBlkEdges * H : 0));
  int* s_start = s_u + kBlkEdges;
  int4* s_unit = reinterpret_cast<int4*>(s_start + kBlkUnits + 4);
  const int t = threadIdx.x;
  const int nu = blk_prologue(a.units, a.block_ptr, s_unit, s_start);
  const int ne = s_start[nu];

  // ---- phase 1: thread <-> edge slot -------------------------------------------------------------
  int my_p = 0;
  int64_t my_ed = 0;
  if (t < ne) {
    const int j = blk_unit_of(s_start, nu, t);
    const int4 q = s_unit[j];
    const int row = (q.w >= 0) ? a.long_rows[q.x] : q.x;
    const int p = q.y + (t - s_start[j]);
    my_p = p;
    const int u = a.indices[p];
    s_u[t] = u;
    const int64_t ed = a.eid ? a.eid[p] : p;
    my_ed = ed;
    const uint32_t n = a.pos_lo + (a.nidx ? (uint32_t)a.nidx[p] : (uint32_t)p);
    const PhiloxKey key = resolve_epoch(a.key);
    const int nchunk = (H + 3) / 4;
    const bool h4 = (H & 3) == 0 && a.hvec;
    for (int cc = 0; cc < nchunk; ++cc) {
      float w[4], sl4[4], sr4[4], ns4[4] = {1.f, 1.f, 1.f, 1.f}, m4[4], l4[4];
      if (h4) {
        load4(a.el + (int64_t)u * H, 4 * cc, H, true, sl4);
        load4(a.er + (int64_t)row * H, 4 * cc, H, true, sr4);
        if (a.nscale) load4(a.nscale + (int64_t)row * H, 4 * cc, H, true, ns4);
        load4(a.stats + (int64_t)row * 2 * H, 4 * cc, H, true, m4);
        load4(a.stats + (int64_t)row * 2 * H + H, 4 * cc, H, true, l4);
      } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int h = 4 * cc + jj;
          const bool in = h < H;
          sl4[jj] = in ? a.el[(int64_t)u * H + h] : 0.f;
          sr4[jj] = in ? a.er[(int64_t)row * H + h] : 0.f;
          if (a.nscale && in) ns4[jj] = a.nscale[(int64_t)row * H + h];
          m4[jj] = in ? a.stats[(int64_t)row * 2 * H + h] : 0.f;
          l4[jj] = in ? a.stats[(int64_t)row * 2 * H + H + h] : 1.f;
        }
      }
      head_w4(a, key, n, ed, (uint32_t)cc, w);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int h = 4 * cc + jj;
        if (h < H) {
          const float sL = sl4[jj] + sr4[jj];
          const float lr = sL > 0.f ? sL : a.neg_slope * sL;
          const float wn = w[jj] * ns4[jj];
          s_a[t * H + h] = __expf(wn * lr - m4[jj]) / l4[jj];
          s_c1[t * H + h] = wn * (sL > 0.f ? 1.0f : a.neg_slope);
          if (ba.dw) s_c2[t * H + h] = lr * ns4[jj];
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: a team per unit: <G[v,h,:], ft[u,h,:]> per in-edge -> ds -> de ---------------------------
  constexpr int TEAMS = kBlkThreads / LPE, NR = CPL >= 4 ? 2 : STAG_GAT_NR;
  const int team = t / LPE, c = t % LPE;
  const int lph = a.lphp;
  int k0[CPL], hl[CPL];
  bool kin[CPL];
#pragma unroll
  for (int cj = 0; cj < CPL; ++cj) {
    lane_chunk(c + LPE * cj, H, F, a.lphp, k0[cj], kin[cj], hl[cj]);
  }
  const __amdgpu_buffer_rsrc_t rft =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.ft), 0, (int)a.ft_bytes, 0x00020000);
  const bool ft_buf = a.ft_bytes != 0;
  for (int j = team; j < nu; j += TEAMS) {
    const int4 q = s_unit[j];
    const int row = (q.w >= 0) ? a.long_rows[q.x] : q.x;
    const int e0 = s_start[j], e1 = s_start[j + 1];
    if (e0 == e1) continue;
    float gv[CPL][4], gdo[CPL];
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      float ov[4] = {0.f, 0.f, 0.f, 0.f};
      gv[cj][0] = gv[cj][1] = gv[cj][2] = gv[cj][3] = 0.f;
      if (kin[cj]) {
        load4(ba.g + (int64_t)row * HF, k0[cj], HF, true, gv[cj]);
        load4(ba.out + (int64_t)row * HF, k0[cj], HF, true, ov);
      }
      gdo[cj] = gat_head_sum((gv[cj][0] * ov[0] + gv[cj][1] * ov[1]) + (gv[cj][2] * ov[2] + gv[cj][3] * ov[3]), lph);
    }
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
          const int u = s_u[e + r];
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              if (ft_buf) bufrow4(rft, u, (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
              else loadrow4(a.ft + (int64_t)u * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {                              // uniform over the team
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            float dot = 0.f;
            if (kin[cj])
              dot = (gv[cj][0] * fv[r][cj][0] + gv[cj][1] * fv[r][cj][1]) + (gv[cj][2] * fv[r][cj][2] + gv[cj][3] * fv[r][cj][3]);
            dot = gat_head_sum(dot, lph);
            if (kin[cj] && (k0[cj] % F) == 0) {
              const float ds = s_a[(e + r) * H + hl[cj]] * (dot - gdo[cj]);
              s_c1[(e + r) * H + hl[cj]] = ds * s_c1[(e + r) * H + hl[cj]];
              if (ba.dw) s_c2[(e + r) * H + hl[cj]] = ds * s_c2[(e + r) * H + hl[cj]];
            }
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 3: per-edge results by forward position (coalesced); d er per unit ------------------------
  if (t < ne) {
    float* dst = ba.ade + (int64_t)my_p * 2 * H;
    if ((H & 3) == 0) {
      for (int h = 0; h < H; h += 4) {
        *reinterpret_cast<float4*>(dst + h) = *reinterpret_cast<const float4*>(s_a + t * H + h);
        *reinterpret_cast<float4*>(dst + H + h) = *reinterpret_cast<const float4*>(s_c1 + t * H + h);
      }
    } else {
      for (int h = 0; h < H; ++h) { dst[h] = s_a[t * H + h]; dst[H + h] = s_c1[t * H + h]; }
    }
    if (ba.dw)
      for (int h = 0; h < H; ++h) ba.dw[my_ed * H + h] = s_c2[t * H + h];
  }
  for (int i = t; i < nu * H; i += kBlkThreads) {
    const int j = i / H, h = i - j * H;
    const int4 q = s_unit[j];
    float sum = 0.f;
    for (int e = s_start[j]; e < s_start[j + 1]; ++e) sum += s_c1[e * H + h];
    if (q.w < 0) ba.d_er[(int64_t)q.x * H + h] = sum;
    else ba.ws[(int64_t)q.w * H + h] = sum;            // a segment's share; gat_seg_finish_kernel adds them
  }
}

struct GatSrcBlkArgs {
  const int32_t* indices;      // csr_t: destination row of each transposed position
  const int32_t* nidx;         // csr_t: forward position of each transposed position
  const stag_unit* units;
  const int32_t* block_ptr;
  const int32_t* long_rows;
  const float* ade;            // [E, 2H] by forward position
  const float* g;              // [n_dst rows of the forward, H*F]
  int32_t H, F, HF;
  uint32_t g_bytes;
  float* d_ft;                 // [n_src, H*F]
  float* d_el;                 // [n_src, H]
  float* ws;                   // segment partials: [n_seg_t][HF + H]
};

template <int LPE, int CPL>
__global__ __launch_bounds__(kBlkThreads) void gat_bwd_src_block_kernel(const GatSrcBlkArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int H = a.H, F = a.F, HF = a.HF;
  float* s_a = lds;                                   // [kBlkEdges][H]
  float* s_de = s_a + kBlkEdges * H;                  // [kBlkEdges][H]
  int* s_v = reinterpret_cast<int*>(s_de + kBlkEdges * H);
  int* s_start = s_v + kBlkEdges;
  int4* s_unit = reinterpret_cast<int4*>(s_start + kBlkUnits + 4);
  const int t = threadIdx.x;
  const int nu = blk_prologue(a.units, a.block_ptr, s_unit, s_start);
  const int ne = s_start[nu];
  if (t < ne) {
    const int j = blk_unit_of(s_start, nu, t);
    const int4 q = s_unit[j];
    const int qq = q.y + (t - s_start[j]);
    s_v[t] = a.indices[qq];
    const float* src = a.ade + (int64_t)a.nidx[qq] * 2 * H;
    if ((H & 3) == 0) {
      for (int h = 0; h < H; h += 4) {
        *reinterpret_cast<float4*>(s_a + t * H + h) = *reinterpret_cast<const float4*>(src + h);
        *reinterpret_cast<float4*>(s_de + t * H + h) = *reinterpret_cast<const float4*>(src + H + h);
      }
    } else {
      for (int h = 0; h < H; ++h) { s_a[t * H + h] = src[h]; s_de[t * H + h] = src[H + h]; }
    }
  }
  __syncthreads();
  // d el[u,h] = sum of de over the out-edges, in transposed-position order
  for (int i = t; i < nu * H; i += kBlkThreads) {
    const int j = i / H, h = i - j * H;
    const int4 q = s_unit[j];
    float sum = 0.f;
    for (int e = s_start[j]; e < s_start[j + 1]; ++e) sum += s_de[e * H + h];
    if (q.w < 0) a.d_el[(int64_t)q.x * H + h] = sum;
    else a.ws[(int64_t)q.w * (HF + H) + HF + h] = sum;
  }
  // d ft[u,h,:] = sum over out-edges of a[e,h] G[v,h,:]
  constexpr int TEAMS = kBlkThreads / LPE, NR = CPL >= 4 ? 2 : STAG_GAT_NR;
  const int team = t / LPE, c = t % LPE;
  int k0[CPL], hl[CPL];
  bool kin[CPL];
#pragma unroll
  for (int cj = 0; cj < CPL; ++cj) {
    k0[cj] = (c + LPE * cj) * 4;
    kin[cj] = k0[cj] < HF;
    hl[cj] = kin[cj] ? k0[cj] / F : 0;
  }
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g), 0, (int)a.g_bytes, 0x00020000);
  const bool g_buf = a.g_bytes != 0;
  for (int j = team; j < nu; j += TEAMS) {
    const int4 q = s_unit[j];
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float acc[CPL][4];
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) acc[cj][0] = acc[cj][1] = acc[cj][2] = acc[cj][3] = 0.f;
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
          const int v = s_v[e + r];
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              if (g_buf) bufrow4(rg, v, (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
              else loadrow4(a.g + (int64_t)v * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              const float w = s_a[(e + r) * H + hl[cj]];
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[cj][x] = __builtin_fmaf(w, fv[r][cj][x], acc[cj][x]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      if (!kin[cj]) continue;
      if (q.w < 0) store4_out(a.d_ft + (int64_t)q.x * HF, k0[cj], HF, true, acc[cj]);
      else store4(a.ws + (int64_t)q.w * (HF + H), k0[cj], HF, true, acc[cj]);
    }
  }
}

// ---- backward with ONE gather of [H*F] rows ---------------------------------------------------------------
// The two kernels above gather 1-KB rows twice: ft[u] by destination (for <G[v], ft[u]>) and G[v] by source (for
// d ft[u] = sum a G[v]).  The dot product is symmetric in where it is formed: on the SOURCE-major CSR ft[u] is the
// unit's own row and G[v] is the row the d ft sum gathers anyway.  What the source-major side lacks is the softmax
// correction sum_e' a[e',h] <G[v,h], ft[u',h]> = <G[v,h], out[v,h]> of the destination row — a per-node quantity,
// sdot [N, H], that one streaming pass over G and out provides (gat_rowdot_kernel) — and d er[v], whose terms it
// leaves in dsl [E, H] by forward position, where the in-edges of v are contiguous (gat_der_kernel).
//   gat_rowdot_kernel       sdot[v,h] = sum_f G[v,h,f] out[v,h,f]                       (2 N H F floats read)
//   gat_bwd_one_kernel      per batch of the source-major plan: phase 1 (thread per edge) a[e,h], the leaky-relu /
//                           noise factors and sdot[v,h] into LDS; phase 2 (team per source row) gathers G[v], forms
//                           the per-head dot with the own ft row, d s[e,h] = a (dot - sdot) c1, and d ft[u] += a G[v];
//                           phase 3 writes dsl (by forward position), dw (by edge id), d el[u]
//   gat_der_kernel          d er[v,h] = sum of dsl over the row's positions
struct GatBwd1Args {
  GatArgs f;             // graph fields: the SOURCE-major CSR (indices = destination, eid, nidx) and its block plan
  const float* g;        // [n_dst of the forward, H*F]
  uint32_t g_bytes;
  const float* pack;     // [n_dst of the forward, 4H]: er | m | l | sdot per destination (gat_rowdot_kernel)
  float* d_ft;           // [n_src, H*F]
  float* d_el;           // [n_src, H]
  float* dsl;            // [E, H] by forward position
  float* dw;             // [E, H] by edge id, or null
  float* ws;             // segment partials: [n_seg_t][HF + H]
  int32_t eid_is_pos;    // the forward CSR has no eid: edge id = forward position
  float* dp_part;        // [n_blocks][2][H] or null: this batch's share of the gradients of scalar / per-head noise
                         // parameters, sum_e dw[e,h] * dw/dp_i[e,h] (stag_gat_bwd_dp; vi=True, stag/layers.py:123-124)
};

constexpr int kRowdotRows = 4;
// sdot goes into a per-node record next to the other per-destination inputs of the edge phase — er, the softmax
// statistics m and l — so that an edge fetches ONE line of 4H floats instead of three separate rows:
// pack[v] = er[H] | m[H] | l[H] | sdot[H]
template <int LPE>
__global__ __launch_bounds__(256) void gat_rowdot_kernel(const float* g, const float* out, int n, int H, int F, int HF,
                                                         int lphp, const float* er, const float* stats, float* pack) {
  constexpr int R = kRowdotRows;
  const int c = threadIdx.x % LPE;
  const int row0 = (blockIdx.x * (256 / LPE) + threadIdx.x / LPE) * R;
  const int lph = lphp;
  for (int L0 = 0; L0 < H * lphp; L0 += LPE) {          // every lane makes every trip (the head sums are DPP)
    int k0, hd;
    bool in;
    lane_chunk(L0 + c, H, F, lphp, k0, in, hd);
    float gv[R][4], ov[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      gv[r][0] = gv[r][1] = gv[r][2] = gv[r][3] = 0.f;
      ov[r][0] = ov[r][1] = ov[r][2] = ov[r][3] = 0.f;
      if (in && row0 + r < n) {
        load4(g + (int64_t)(row0 + r) * HF, k0, HF, true, gv[r]);
        load4(out + (int64_t)(row0 + r) * HF, k0, HF, true, ov[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float d = gat_head_sum((gv[r][0] * ov[r][0] + gv[r][1] * ov[r][1]) + (gv[r][2] * ov[r][2] + gv[r][3] * ov[r][3]), lph);
      if (in && row0 + r < n && (k0 % F) == 0) {
        const int64_t row = row0 + r;
        const int h = k0 / F;
        float* rec = pack + row * 4 * H;
        rec[h] = er[row * H + h];
        rec[H + h] = stats[row * 2 * H + h];
        rec[2 * H + h] = stats[row * 2 * H + H + h];
        rec[3 * H + h] = d;
      }
    }
  }
}

template <int LPE, int CPL>
__global__ __launch_bounds__(kBlkThreads) void gat_bwd_one_kernel(const GatBwd1Args ba) {
  extern __shared__ __align__(16) float lds[];
  const GatArgs& a = ba.f;
  const int H = a.H, F = a.F, HF = a.HF;
  float* s_a = lds;                                   // [kBlkEdges][H] attention
  float* s_c1 = s_a + kBlkEdges * H;                  // [kBlkEdges][H] w ns lrelu'(s), then d s
  float* s_sd = s_c1 + kBlkEdges * H;                 // [kBlkEdges][H] sdot of the edge's destination
  float* s_c2 = s_sd + kBlkEdges * H;                 // [kBlkEdges][H] lrelu(s) ns, then dw (only when wanted)
  const bool want_dw = ba.dw != nullptr || ba.dp_part != nullptr;
  int* s_v = reinterpret_cast<int*>(s_c2 + (want_dw ? kBlkEdges * H : 0));
  int* s_start = s_v + kBlkEdges;
  int4* s_unit = reinterpret_cast<int4*>(s_start + kBlkUnits + 4);
  const int t = threadIdx.x;
  const int nu = blk_prologue(a.units, a.block_ptr, s_unit, s_start);
  const int ne = s_start[nu];

  // ---- phase 1: thread <-> out-edge slot -----------------------------------------------------------------
  int my_fp = 0;
  int64_t my_ed = 0;
  if (t < ne) {
    const int j = blk_unit_of(s_start, nu, t);
    const int4 q = s_unit[j];
    const int u = (q.w >= 0) ? a.long_rows[q.x] : q.x;          // the source node: this unit's row
    const int qq = q.y + (t - s_start[j]);
    const int v = a.indices[qq];
    s_v[t] = v;
    const int fp = a.nidx[qq];                                  // forward position: the noise index, the dsl slot
    my_fp = fp;
    const int64_t ed = (ba.eid_is_pos || !a.eid) ? (int64_t)fp : (int64_t)a.eid[qq];
    my_ed = ed;
    const uint32_t n = a.pos_lo + (uint32_t)fp;
    const PhiloxKey key = resolve_epoch(a.key);
    const int nchunk = (H + 3) / 4;
    const bool h4 = (H & 3) == 0 && a.hvec;
    for (int cc = 0; cc < nchunk; ++cc) {
      float w[4], sl4[4], sr4[4], ns4[4] = {1.f, 1.f, 1.f, 1.f}, m4[4], l4[4], sd4[4];
      const float* rec = ba.pack + (int64_t)v * 4 * H;          // er | m | l | sdot of the destination
      if (h4) {
        load4(a.el + (int64_t)u * H, 4 * cc, H, true, sl4);
        if (a.nscale) load4(a.nscale + (int64_t)v * H, 4 * cc, H, true, ns4);
        load4(rec, 4 * cc, H, true, sr4);
        load4(rec + H, 4 * cc, H, true, m4);
        load4(rec + 2 * H, 4 * cc, H, true, l4);
        load4(rec + 3 * H, 4 * cc, H, true, sd4);
      } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int h = 4 * cc + jj;
          const bool in = h < H;
          sl4[jj] = in ? a.el[(int64_t)u * H + h] : 0.f;
          if (a.nscale && in) ns4[jj] = a.nscale[(int64_t)v * H + h];
          sr4[jj] = in ? rec[h] : 0.f;
          m4[jj] = in ? rec[H + h] : 0.f;
          l4[jj] = in ? rec[2 * H + h] : 1.f;
          sd4[jj] = in ? rec[3 * H + h] : 0.f;
        }
      }
      head_w4(a, key, n, ed, (uint32_t)cc, w);
      const uint32_t kbits = a.drop_keep > 0.f ? drop_keep4(a, resolve_epoch(a.drop_key), n, (uint32_t)cc) : 15u;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int h = 4 * cc + jj;
        if (h < H) {
          const float sL = sl4[jj] + sr4[jj];
          const float lr = sL > 0.f ? sL : a.neg_slope * sL;
          const float wn = w[jj] * ns4[jj];
          const float av = __expf(wn * lr - m4[jj]) / l4[jj];
          // attention dropout: the sign carries the keep bit (a > 0): dropped edges are stored as -a
          s_a[t * H + h] = (a.drop_keep > 0.f && !((kbits >> jj) & 1u)) ? -av : av;
          s_c1[t * H + h] = wn * (sL > 0.f ? 1.0f : a.neg_slope);
          s_sd[t * H + h] = sd4[jj];
          if (want_dw) s_c2[t * H + h] = lr * ns4[jj];
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: a team per source row: gather G[v]; <G[v,h,:], ft[u,h,:]> -> d s; d ft[u] += a G[v] ----------
  constexpr int TEAMS = kBlkThreads / LPE, NR = CPL >= 4 ? 2 : STAG_GAT_NR;
  const int team = t / LPE, c = t % LPE;
  const int lph = a.lphp;
  int k0[CPL], hl[CPL];
  bool kin[CPL];
#pragma unroll
  for (int cj = 0; cj < CPL; ++cj) {
    lane_chunk(c + LPE * cj, H, F, a.lphp, k0[cj], kin[cj], hl[cj]);
  }
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ba.g), 0, (int)ba.g_bytes, 0x00020000);
  const bool g_buf = ba.g_bytes != 0;
  for (int j = team; j < nu; j += TEAMS) {
    const int4 q = s_unit[j];
    const int u = (q.w >= 0) ? a.long_rows[q.x] : q.x;
    const int e0 = s_start[j], e1 = s_start[j + 1];
    float fu[CPL][4], acc[CPL][4];
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      fu[cj][0] = fu[cj][1] = fu[cj][2] = fu[cj][3] = 0.f;
      acc[cj][0] = acc[cj][1] = acc[cj][2] = acc[cj][3] = 0.f;
      if (kin[cj] && e0 < e1) load4(a.ft + (int64_t)u * HF, k0[cj], HF, true, fu[cj]);
    }
    for (int e = e0; e < e1; e += NR) {
      float fv[NR][CPL][4];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {
          const int v = s_v[e + r];
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            if (kin[cj]) {
              if (g_buf) bufrow4(rg, v, (uint32_t)HF * 4u, (uint32_t)k0[cj] * 4u, fv[r][cj]);
              else loadrow4(ba.g + (int64_t)v * HF + k0[cj], k0[cj], HF, true, fv[r][cj]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (e + r < e1) {                              // uniform over the team
#pragma unroll
          for (int cj = 0; cj < CPL; ++cj) {
            float dot = 0.f;
            if (kin[cj])
              dot = (fu[cj][0] * fv[r][cj][0] + fu[cj][1] * fv[r][cj][1]) + (fu[cj][2] * fv[r][cj][2] + fu[cj][3] * fv[r][cj][3]);
            dot = gat_head_sum(dot, lph);
            if (kin[cj]) {
              float w = s_a[(e + r) * H + hl[cj]];
              float ds;
              if (a.drop_keep > 0.f) {        // a' = a keep / q feeds d ft and <G, ft>; the correction stays with a
                const float aa = fabsf(w);
                w = w > 0.f ? w * a.drop_scale : 0.f;
                ds = w * dot - aa * s_sd[(e + r) * H + hl[cj]];
              } else {
                ds = w * (dot - s_sd[(e + r) * H + hl[cj]]);
              }
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[cj][x] = __builtin_fmaf(w, fv[r][cj][x], acc[cj][x]);
              if ((k0[cj] % F) == 0) {
                s_c1[(e + r) * H + hl[cj]] = ds * s_c1[(e + r) * H + hl[cj]];
                if (want_dw) s_c2[(e + r) * H + hl[cj]] = ds * s_c2[(e + r) * H + hl[cj]];
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int cj = 0; cj < CPL; ++cj) {
      if (!kin[cj]) continue;
      if (q.w < 0) store4_out(ba.d_ft + (int64_t)q.x * HF, k0[cj], HF, true, acc[cj]);
      else store4(ba.ws + (int64_t)q.w * (HF + H), k0[cj], HF, true, acc[cj]);
    }
  }
  __syncthreads();

  // ---- gradients of scalar / per-head noise parameters (vi=True): dw[e,h] is in LDS, the draw is redone with its
  //      derivatives (same counters), the products go where a and sdot were (both consumed), and 2H threads add the
  //      batch's edges in order: one [2][H] partial per batch, summed by two fixed-order launches (dp_stage*)
  if (ba.dp_part) {
    if (t < ne) {
      const uint32_t n = a.pos_lo + (uint32_t)my_fp;
      const PhiloxKey key = resolve_epoch(a.key);
      const uint32_t c1hi = a.pos_hi << 20;
      for (int cc = 0; cc < (H + 3) / 4; ++cc) {
        float pa[4], pb[4], w[4], d0[4], d1[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int h = 4 * cc + jj;
          const bool in = h < H;
          float q0 = a.p0s, q1 = a.p1s;
          if (a.pmode == STAG_PARAM_PER_CHANNEL) { q0 = in ? a.p0[h] : 0.f; q1 = (in && a.p1) ? a.p1[h] : 0.f; }
          if (a.pmode != STAG_PARAM_SCALAR && (a.nflags & kFlagLogScale)) q1 = exp_scale(q1);
          pa[jj] = q0; pb[jj] = q1;
        }
        if (a.kind == kNormal) draw4_grad<kNormal>(n, (uint32_t)cc | c1hi, key, pa, pb, a.nflags, w, d0, d1);
        else draw4_grad<kUniform>(n, (uint32_t)cc | c1hi, key, pa, pb, a.nflags, w, d0, d1);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int h = 4 * cc + jj;
          if (h < H) {
            s_a[t * H + h] = s_c2[t * H + h] * d0[jj];
            s_sd[t * H + h] = s_c2[t * H + h] * d1[jj];
          }
        }
      }
    }
    __syncthreads();
    if (t < 2 * H) {
      const float* src = t < H ? s_a : s_sd;
      const int h = t < H ? t : t - H;
      float sum = 0.f;
      for (int e = 0; e < ne; ++e) sum += src[e * H + h];
      ba.dp_part[(int64_t)blockIdx.x * 2 * H + t] = sum;
    }
  }

  // ---- phase 3: d s by forward position, dw by edge id; d el per unit ---------------------------------------
  if (t < ne) {
    float* dst = ba.dsl + (int64_t)my_fp * H;
    if ((H & 3) == 0) {
      for (int h = 0; h < H; h += 4)
        *reinterpret_cast<float4*>(dst + h) = *reinterpret_cast<const float4*>(s_c1 + t * H + h);
    } else {
      for (int h = 0; h < H; ++h) dst[h] = s_c1[t * H + h];
    }
    if (ba.dw)
      for (int h = 0; h < H; ++h) ba.dw[my_ed * H + h] = s_c2[t * H + h];
  }
  for (int i = t; i < nu * H; i += kBlkThreads) {
    const int j = i / H, h = i - j * H;
    const int4 q = s_unit[j];
    float sum = 0.f;
    for (int e = s_start[j]; e < s_start[j + 1]; ++e) sum += s_c1[e * H + h];
    if (q.w < 0) ba.d_el[(int64_t)q.x * H + h] = sum;
    else ba.ws[(int64_t)q.w * (HF + H) + HF + h] = sum;
  }
}

// d er[v,h] = sum over the positions of row v of dsl[p,h]: a thread per (unit of the forward plan, head), the
// unit's <= seg_len positions in order; segments leave partials for gat_seg_finish_kernel
__global__ __launch_bounds__(256) void gat_der_kernel(const stag_unit* units, int n_units, const int32_t* indptr,
                                                      const float* dsl, int H, float* d_er, float* ws) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t unit = i / H;
  const int h = (int)(i - unit * H);
  if (unit >= n_units) return;
  int row, b, len, slot = -1;
  if (units) {
    const int4 q = *reinterpret_cast<const int4*>(units + unit);
    row = q.x; b = q.y; len = q.z; slot = q.w;
  } else {
    row = (int)unit; b = indptr[row]; len = indptr[row + 1] - b;
  }
  float sum = 0.f;
  for (int p = b; p < b + len; ++p) sum += dsl[(int64_t)p * H + h];
  if (slot < 0) d_er[(int64_t)row * H + h] = sum;
  else ws[(int64_t)slot * H + h] = sum;
}

// out[long_rows[r]][k] = sum over the row's segments of ws[s][ws_off + k], k < width.  A workgroup per
// (long row, 16 columns): 16 slices of the segment list are summed side by side (slice i takes segments
// i, i+16, ... in order, Kahan), then the 16 slice sums in slice order — a fixed order, and a hub row
// of 200 segments costs 13 dependent loads instead of 200.
__global__ __launch_bounds__(256) void gat_seg_finish_kernel(const float* ws, int ws_stride, int ws_off, int width,
                                                             const int32_t* long_rows, const int32_t* long_seg_ptr,
                                                             float* out, int ld_out) {
  __shared__ float red[16][17];
  const int r = blockIdx.x, kx = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int k = blockIdx.y * 16 + kx;
  const int s0 = long_seg_ptr[r], s1 = long_seg_ptr[r + 1];
  float sum = 0.f, comp = 0.f;
  if (k < width) {
    for (int s = s0 + slice; s < s1; s += 16) {
      const float y = ws[(int64_t)s * ws_stride + ws_off + k] - comp;
      const float n = sum + y;
      comp = (n - sum) - y;
      sum = n;
    }
  }
  red[slice][kx] = sum;
  __syncthreads();
  if (slice == 0 && k < width) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i][kx];
    out[(int64_t)long_rows[r] * ld_out + k] = tot;
  }
}

}  // namespace

// The shape rule of the cooperative kernels: a head takes lphp = lanes_per_head(F) lanes (the backward's head sums are
// DPP butterflies, and the forward keeps the backward's mapping; lanes past a head's channels idle), a row H * lphp of
// them, at most 256.  Returns lphp, or 0 where they have no shape for (H, F): F % 4 != 0, H > 16 or a wider row.
static int gat_blk_lphp(int H, int F) {
  const int lphp = (F % 4 == 0) ? lanes_per_head(F) : 0;
  return (lphp == 0 || H > kBlkMaxH || lphp > 64 || H * lphp > 256) ? 0 : lphp;
}

// what a narrow (32-bit) buffer descriptor takes as the extent of `rows` rows of row_bytes each: 0 where it cannot
// name them all, and the kernel reads through plain addresses
static uint32_t narrow_extent(int64_t rows, uint64_t row_bytes) {
  const uint64_t bytes = (uint64_t)rows * row_bytes;
  return (bytes < (1ull << 32) && rows < (1 << 24)) ? (uint32_t)bytes : 0u;
}

// attention dropout of a call: 0 = none / set, STAG_EINVAL for a bad probability
static int fill_drop(GatArgs& a, const stag_gat_drop* drop) {
  a.drop_keep = 0.f; a.drop_scale = 1.f;
  if (!drop || drop->keep_prob >= 1.0f) return STAG_OK;
  if (!(drop->keep_prob > 0.0f)) return STAG_EINVAL;
  a.drop_keep = drop->keep_prob;
  a.drop_scale = 1.0f / drop->keep_prob;
  a.drop_key = make_key(drop->seed, drop->offset, drop->epoch);
  return STAG_OK;
}
static bool drop_on(const stag_gat_drop* drop) { return drop && drop->keep_prob < 1.0f; }

// the forward's segment states: merged by the segment that arrives last, through a 32-bit buffer descriptor
constexpr unsigned kGatFwdPlan = kPlanSegPtr | kPlanWorkspace | kPlanNarrow | kPlanCounters;

// what every GAT argument block takes from the graph, the scores and the spec (the noise width is H)
static void fill_gat_args(GatArgs& a, const stag_csr* csr, const float* el, const float* er, int32_t H, float neg_slope,
                          const stag_noise_spec* spec, const float* norm_scale) {
  a.indptr = csr->indptr; a.indices = csr->indices; a.eid = csr->eid; a.nidx = csr->nidx;
  a.n_rows = csr->n_dst; a.el = el; a.er = er;
  a.nscale = spec->in_norm ? norm_scale : nullptr;
  a.H = H; a.neg_slope = neg_slope;
  fill_spec(a, spec, 0);
}

extern "C" size_t stag_gat_workspace_bytes(int32_t n_seg, int32_t H, int32_t F) {
  if (n_seg <= 0 || H <= 0 || F <= 0) return 0;
  return (size_t)n_seg * (size_t)((H * F + 2 * H + 3) & ~3) * sizeof(float);   // rows padded to 16 bytes
}

// ---- the forward entries: stag_gat_fwd, stag_gat_fwd_half, stag_gat_fwd_mc -------------------------------------------
constexpr int kGatGo = 1;   // gat_fwd_begin: no return code, the entry goes on
// What stag_gat_fwd and stag_gat_fwd_half check and fill alike, in the order that gives both their return codes, up to
// the extent of ft (rows of ft_esize-byte elements).  ft_type_ok: the half entry's ft_dtype check, at its place among
// the others.  Returns kGatGo, or what the entry returns (STAG_OK: a graph without rows).
static int gat_fwd_begin(GatArgs& a, const stag_csr* csr, const float* el, const float* er, const void* ft,
                         uint32_t ft_esize, bool ft_type_ok, int32_t H, int32_t F, float neg_slope,
                         const stag_noise_spec* spec, const float* norm_scale, const stag_gat_drop* drop, float* out,
                         float* stats_out) {
  if (check_csr_header(csr)) return STAG_EINVAL;
  if (!spec || spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI) return STAG_EINVAL;
  if (!out || H <= 0 || F <= 0) return STAG_EINVAL;
  if (!ft_type_ok) return STAG_EINVAL;
  const int64_t HF64 = (int64_t)H * F;
  // one team spans the H*F row: 256 channels on the one-unit-per-team kernel, 1024 (4 chunks per lane) on the
  // workgroup-cooperative one (which also wants H <= 16, F % 4 == 0 and a block plan: checked by the entry)
  if (H > 64 || HF64 > 1024) return STAG_ENOSYS;
  if (spec->chunk_base != 0) return STAG_ENOSYS;  // heads are not channel-sharded
  if (spec->in_norm && !norm_scale) return STAG_EINVAL;   // the caller runs the row-sum pass first
  if (csr->n_dst == 0) return STAG_OK;
  if (csr->n_edges > 0 && (!csr->indices || !el || !er || !ft)) return STAG_EINVAL;
  if (spec->kind == STAG_NOISE_EXPLICIT && !spec->p0 && csr->n_edges > 0) return STAG_EINVAL;
  if (spec->kind >= STAG_NOISE_NORMAL && spec->param_mode != STAG_PARAM_SCALAR && csr->n_edges > 0 &&
      (!spec->p0 || (spec->kind != STAG_NOISE_BERNOULLI && !spec->p1)))
    return STAG_EINVAL;
  if (spec->deriv != 0) return STAG_EINVAL;
  fill_gat_args(a, csr, el, er, H, neg_slope, spec, norm_scale);
  a.ft = static_cast<const float*>(ft);     // (half rows: gat_row4<DT> reads them as what they are)
  a.F = F; a.HF = (int)HF64;
  const int prc = check_positions(spec, csr->n_edges, H, spec->kind >= STAG_NOISE_NORMAL || drop_on(drop));
  if (prc) return prc;
  a.out = out; a.stats = stats_out;
  if (fill_drop(a, drop)) return STAG_EINVAL;
  a.ft_bytes = narrow_extent(csr->n_src, (uint64_t)a.HF * ft_esize);
  return kGatGo;
}

// the plan of a forward launch, which may be absent: checked, its units and, where it has segments, their states
static int gat_fwd_plan(GatArgs& a, const stag_csr* csr, const stag_plan* plan) {
  const bool use_plan = plan_in_use(plan);
  const size_t need = use_plan ? stag_gat_workspace_bytes(plan->n_seg, a.H, a.F) : 0;
  const int plrc = check_plan(plan, kGatFwdPlan, need);
  if (plrc) return plrc;
  fill_plan(a, csr, plan);
  if (use_plan && plan->n_seg > 0) {
    a.seg_counters = plan->seg_counters; a.n_seg = plan->n_seg;
    a.ws_stride = (a.HF + 2 * a.H + 3) & ~3; a.ws_bytes = (uint32_t)need;
  }
  return STAG_OK;
}

// The workgroup-cooperative form of a launch (batches of units: stag_plan_blocks with STAG_BLOCK_EDGES / _UNITS): the
// fields only it reads, and what picks its kernel.  A head takes lphp lanes, a row H * lphp: lpe lanes per unit with cpl
// chunks of 4 channels each.  local: the batches are XCD-local, the rows come out of an L2.
struct GatBlkShape { int lpe, cpl; bool local; };
static GatBlkShape gat_blk_lanes(int H, int lphp, const stag_plan* plan) {
  const int nchunk = H * lphp;
  return {lanes_for(nchunk, 4), nchunk <= 64 ? 1 : (nchunk <= 128 ? 2 : 4), plan->xcd_order != nullptr};
}
// ... and the block fields of a filled argument block.  hvec: every [n, H] array the kernel reads takes dwordx4 loads:
// el and nscale, and the rest the pass reads (er; the backward's stats or pack), whose alignment the caller states.
static GatBlkShape gat_blk_shape(GatArgs& a, const stag_plan* plan, int lphp, bool rest_aligned) {
  a.block_ptr = plan->block_ptr;
  a.lphp = lphp;
  a.hvec = aligned16(a.el) && (!a.nscale || aligned16(a.nscale)) && rest_aligned;
  return gat_blk_lanes(a.H, lphp, plan);
}
// bytes of LDS of a cooperative workgroup: `floats` floats ahead of the batch records, at least `floor`
static size_t gat_lds(size_t floats, size_t floor) {
  const size_t lds = floats * sizeof(float) + (size_t)(kBlkEdges + kBlkUnits + 4) * sizeof(int) +
                     (size_t)kBlkUnits * sizeof(int4);
  return lds < floor ? floor : lds;
}
// ... of a forward workgroup that carries ns samples: logits and statistics per sample
static size_t gat_blk_lds(int H, int ns, size_t floor) {
  return gat_lds((size_t)ns * (kBlkEdges * H + 2 * kBlkUnits * H), floor);
}

// The instantiation of a cooperative kernel for a shape, forward or backward: launch(LPE, CPL, rows) with
// std::integral_constants, rows the class of rows in flight, which each forward entry maps to a knob of its own and
// the backward ignores — rows of one chunk per lane (at most 256 floats) are kGatRowsNarrow whatever the launch; wider
// ones are kGatRowsWide, or kGatRowsWideLocal on XCD-local batches.  stag_gat_fwd_mc goes through the same ladder as
// stag_gat_fwd: the same rounds, so the same bits per sample.
enum { kGatRowsWide, kGatRowsWideLocal, kGatRowsNarrow };
constexpr int gat_rows(int rows, int wide, int wide_local, int narrow) {
  return rows == kGatRowsWide ? wide : (rows == kGatRowsWideLocal ? wide_local : narrow);
}
template <int V> using gat_int = std::integral_constant<int, V>;
template <class Launch>
static void gat_blk_dispatch(const GatBlkShape& sh, const Launch& launch) {
  pick<4, 2, 1>(sh.cpl, [&](auto Cc) {
    if constexpr (decltype(Cc)::value == 1)
      pick<64, 32, 16, 8, 4>(sh.lpe, [&](auto L) { launch(L, Cc, gat_int<kGatRowsNarrow>{}); });
    else if (sh.local) launch(gat_int<64>{}, Cc, gat_int<kGatRowsWideLocal>{});
    else launch(gat_int<64>{}, Cc, gat_int<kGatRowsWide>{});
  });
}

extern "C" int stag_gat_fwd(const stag_csr* csr, const stag_plan* plan, const float* el,
                            const float* er, const float* ft, int32_t H, int32_t F, float neg_slope,
                            const stag_noise_spec* spec, const float* norm_scale, const stag_gat_drop* drop,
                            float* out, float* stats_out, void* stream) {
  GatArgs a{};
  const int rc = gat_fwd_begin(a, csr, el, er, ft, 4u, true, H, F, neg_slope, spec, norm_scale, drop, out, stats_out);
  if (rc != kGatGo) return rc;
  const int HF = a.HF;
  const bool use_plan = plan_in_use(plan);
  const int plrc = gat_fwd_plan(a, csr, plan);
  if (plrc) return plrc;
  bool vec = (F % 4 == 0) && aligned16(ft) && aligned16(out);
  if (a.ws) vec = vec && aligned16(a.ws) && (a.ws_stride % 4 == 0);

  const int nchunk = (HF + 3) / 4;
  const int lpe = lanes_for(nchunk, 4);
  const int tpb = 256 / lpe;
  const dim3 grid((a.n_units + tpb - 1) / tpb);
  const size_t lds_bytes = (size_t)256 * H * sizeof(float);   // [teams][LPE][H]
  hipStream_t s = (hipStream_t)stream;
  const int lphp = gat_blk_lphp(H, F);
  const bool blk_ok = use_plan && plan->block_ptr && plan->n_blocks > 0 && vec && plan->seg_len <= kBlkEdges && lphp > 0;
  if (HF > 256 && !blk_ok) return STAG_ENOSYS;
  if (a.drop_keep > 0.f && !blk_ok) return STAG_ENOSYS;      // attention dropout lives in the cooperative kernels
  if (check_csr(csr)) return STAG_EINVAL;
  if (blk_ok) {
    const GatBlkShape sh = gat_blk_shape(a, plan, lphp, aligned16(er));
    const size_t lds_blk = gat_blk_lds(H, 1, STAG_GAT_LDS_MIN);
    const dim3 gb(plan->n_blocks);
    gat_blk_dispatch(sh, [&](auto L, auto Cc, auto rows) {
      constexpr int NRF = gat_rows(decltype(rows)::value, STAG_GAT_NR_FWD, STAG_GAT_NR_FWD_LOCAL, STAG_GAT_NR_FWD_NARROW);
      hipLaunchKernelGGL((gat_fwd_block_kernel<kGatRowF32, decltype(L)::value, decltype(Cc)::value, NRF>), gb,
                         dim3(kBlkThreads), lds_blk, s, a);
    });
    return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
  }
  pick<64, 32, 16, 8, 4>(lpe, vec, [&](auto L, auto V) {
    hipLaunchKernelGGL((gat_fwd_kernel<decltype(L)::value, decltype(V)::value>), grid, dim3(256), lds_bytes, s, a);
  });
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// stag_gat_fwd on fp16 / bf16 ft rows, the workgroup-cooperative form only (gat_fwd_block_kernel<DT, ...>).  The checks
// run in stag_gat_fwd's order; what that entry would hand to gat_fwd_kernel is STAG_ENOSYS here (the caller widens ft
// and calls stag_gat_fwd).  Every refusal comes before any device work.
extern "C" int stag_gat_fwd_half(const stag_csr* csr, const stag_plan* plan, const float* el, const float* er,
                                 const void* ft, int32_t ft_dtype, int32_t H, int32_t F, float neg_slope,
                                 const stag_noise_spec* spec, const float* norm_scale, const stag_gat_drop* drop,
                                 float* out, float* stats_out, void* stream) {
  GatArgs a{};
  const int rc = gat_fwd_begin(a, csr, el, er, ft, 2u, ft_dtype == STAG_DTYPE_F16 || ft_dtype == STAG_DTYPE_BF16, H, F,
                               neg_slope, spec, norm_scale, drop, out, stats_out);
  if (rc != kGatGo) return rc;
  // the cooperative form: F % 4 == 0, H <= 16, a row within 256 lanes, a block plan whose segments fit a batch
  const int lphp = gat_blk_lphp(H, F);
  if (lphp == 0) return STAG_ENOSYS;
  if (!plan_in_use(plan) || !plan->block_ptr || plan->n_blocks <= 0 || plan->seg_len > kBlkEdges) return STAG_ENOSYS;
  const int plrc = gat_fwd_plan(a, csr, plan);
  if (plrc) return plrc;
  // a lane loads 8 bytes of a row and stores 16 of out / of a segment state
  if ((reinterpret_cast<uintptr_t>(ft) & 7u) != 0 || !aligned16(out) || (a.ws && !aligned16(a.ws))) return STAG_ENOSYS;
  if (check_csr(csr)) return STAG_EINVAL;

  const GatBlkShape sh = gat_blk_shape(a, plan, lphp, aligned16(er));
  const size_t lds_blk = gat_blk_lds(H, 1, STAG_GAT_HALF_LDS_MIN);
  const dim3 gb(plan->n_blocks);
  hipStream_t s = (hipStream_t)stream;
  pick<STAG_DTYPE_BF16, STAG_DTYPE_F16>(ft_dtype, [&](auto DT) {
    gat_blk_dispatch(sh, [&](auto L, auto Cc, auto rows) {
      constexpr int NRF = gat_rows(decltype(rows)::value, STAG_GAT_HALF_NR, STAG_GAT_HALF_NR_LOCAL, STAG_GAT_HALF_NR_NARROW);
      hipLaunchKernelGGL((gat_fwd_block_kernel<decltype(DT)::value, decltype(L)::value, decltype(Cc)::value, NRF>), gb,
                         dim3(kBlkThreads), lds_blk, s, a);
    });
  });
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" size_t stag_gat_fwd_mc_workspace_bytes(int32_t n_seg, int32_t H, int32_t F, int32_t n_samples) {
  if (n_samples <= 0) return 0;
  return stag_gat_workspace_bytes(n_seg, H, F) * (size_t)(n_samples < kGatMcMaxSP ? n_samples : kGatMcMaxSP);
}

// n_samples draws of stag_gat_fwd from one gather of the ft rows per pass of SP samples (gat_fwd_mc_block_kernel).
// Every argument is checked before anything is launched.
extern "C" int stag_gat_fwd_mc(const stag_csr* csr, const stag_plan* plan, const float* el, const float* er,
                               const float* ft, int32_t H, int32_t F, float neg_slope, const stag_noise_spec* spec,
                               int32_t n_samples, int64_t offset_stride, float* out, int64_t out_stride,
                               float* stats_out, int64_t stats_stride, void* stream) {
  if (check_csr_header(csr) || csr->n_src < 0) return STAG_EINVAL;
  if (!spec || !out || !el || !er || !ft || (csr->n_edges > 0 && !csr->indices)) return STAG_EINVAL;
  if (H <= 0 || F <= 0 || n_samples < 1 || offset_stride < 0) return STAG_EINVAL;
  const int64_t HF64 = (int64_t)H * F;
  if (n_samples > 1 && (out_stride < (int64_t)csr->n_dst * HF64 || (stats_out && stats_stride < (int64_t)csr->n_dst * 2 * H)))
    return STAG_EINVAL;
  if (spec->kind != STAG_NOISE_NORMAL && spec->kind != STAG_NOISE_UNIFORM && spec->kind != STAG_NOISE_BERNOULLI)
    return STAG_EINVAL;
  if (spec->param_mode != STAG_PARAM_SCALAR && spec->param_mode != STAG_PARAM_PER_CHANNEL) return STAG_EINVAL;
  if (spec->param_mode == STAG_PARAM_PER_CHANNEL && (!spec->p0 || (spec->kind != STAG_NOISE_BERNOULLI && !spec->p1)))
    return STAG_EINVAL;
  if (spec->in_norm || spec->deriv) return STAG_EINVAL;
  const int prc = check_positions(spec, csr->n_edges, H, true);
  if (prc) return prc;
  if (spec->chunk_base != 0) return STAG_ENOSYS;   // heads are not channel-sharded
  // the cooperative form only: a block plan, F % 4 == 0, H <= 16, H * F <= 1024, a row within 256 lanes, 16-B rows
  const int lphp = gat_blk_lphp(H, F);
  if (!plan || plan->n_units <= 0 || !plan->units || !plan->block_ptr || plan->n_blocks <= 0) return STAG_ENOSYS;
  if (lphp == 0 || HF64 > 1024 || plan->seg_len > kBlkEdges) return STAG_ENOSYS;
  if (!aligned16(plan->units) || !aligned16(ft) || !aligned16(out) || (n_samples > 1 && out_stride % 4 != 0))
    return STAG_ENOSYS;
  const int HF = (int)HF64;

  GatMcArgs g{};
  GatArgs& a = g.a;
  fill_gat_args(a, csr, el, er, H, neg_slope, spec, nullptr);   // (every pass sets its own offset in the key)
  const GatBlkShape sh = gat_blk_shape(a, plan, lphp, aligned16(er));
  const int sp = sh.cpl == 4 ? STAG_GAT_MC_SP_WIDE : STAG_GAT_MC_SP;
  const int wsp = n_samples < sp ? n_samples : sp;
  a.ft = ft; a.F = F; a.HF = HF;
  a.ft_bytes = narrow_extent(csr->n_src, (uint64_t)HF * 4u);
  fill_plan(a, csr, plan);
  a.ws_stride = (HF + 2 * H + 3) & ~3;
  const size_t need = stag_gat_workspace_bytes(plan->n_seg, H, F) * (size_t)wsp;
  const int plrc = check_plan_segments(plan, kGatFwdPlan, need);
  if (plrc) return plrc;
  if (plan->n_seg > 0) {
    if (!aligned16(plan->workspace)) return STAG_ENOSYS;
    a.seg_counters = plan->seg_counters; a.ws_bytes = (uint32_t)need; a.n_seg = plan->n_seg;
  }
  if (csr->n_dst == 0) return STAG_OK;
  if (check_csr(csr)) return STAG_EINVAL;
  g.stride = (uint64_t)offset_stride;
  g.out_stride = out_stride; g.stats_stride = stats_stride;
  g.wsp = wsp;
  const dim3 gb(plan->n_blocks);
  hipStream_t s = (hipStream_t)stream;
  for (int32_t s0 = 0; s0 < n_samples; s0 += sp) {
    g.ns = (n_samples - s0 < sp) ? n_samples - s0 : sp;
    const uint64_t off = spec->offset + (uint64_t)s0 * (uint64_t)offset_stride;
    a.key = make_key(spec->seed, off, spec->epoch);
    a.out = out + (int64_t)s0 * out_stride;
    a.stats = stats_out ? stats_out + (int64_t)s0 * stats_stride : nullptr;
    const size_t lds = gat_blk_lds(H, g.ns, STAG_GAT_LDS_MIN);
    gat_blk_dispatch(sh, [&](auto L, auto Cc, auto rows) {
      constexpr int NRF = gat_rows(decltype(rows)::value, STAG_GAT_NR_FWD, STAG_GAT_NR_FWD_LOCAL, STAG_GAT_NR_FWD_NARROW);
      constexpr int SP = decltype(Cc)::value == 4 ? STAG_GAT_MC_SP_WIDE : STAG_GAT_MC_SP;
      hipLaunchKernelGGL((gat_fwd_mc_block_kernel<decltype(L)::value, decltype(Cc)::value, NRF, SP>), gb,
                         dim3(kBlkThreads), lds, s, g);
    });
    if (hipGetLastError() != hipSuccess) return STAG_EIO;
  }
  return STAG_OK;
}

// the argument block the attention / backward kernels share with the forward
static int fill_edge_args(GatArgs& a, const stag_csr* csr, const stag_plan* plan, const float* el,
                          const float* er, int32_t H, float neg_slope, const stag_noise_spec* spec,
                          const float* norm_scale, const float* stats) {
  fill_gat_args(a, csr, el, er, H, neg_slope, spec, norm_scale);
  // (a caller with attention dropout checks the positions itself, before it launches anything)
  const int prc = check_positions(spec, csr->n_edges, H, spec->kind >= STAG_NOISE_NORMAL);
  if (prc) return prc;
  a.stats = const_cast<float*>(stats);
  return fill_units(a, csr, plan);
}

extern "C" int stag_gat_attn(const stag_csr* csr, const stag_plan* plan, const float* el,
                             const float* er, int32_t H, float neg_slope, const stag_noise_spec* spec,
                             const float* norm_scale, const float* stats, float* attn_out,
                             void* stream) {
  if (check_csr_header(csr)) return STAG_EINVAL;
  if (!spec || spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI || spec->deriv) return STAG_EINVAL;
  if (!attn_out || !stats || H <= 0 || H > 64) return STAG_EINVAL;
  if (spec->chunk_base != 0) return STAG_ENOSYS;
  if (spec->in_norm && !norm_scale) return STAG_EINVAL;
  if (csr->n_dst == 0 || csr->n_edges == 0) return STAG_OK;
  if (!csr->indices || !el || !er) return STAG_EINVAL;
  if (spec->kind == STAG_NOISE_EXPLICIT && !spec->p0 && csr->n_edges > 0) return STAG_EINVAL;
  GatArgs a{};
  const int rc = fill_edge_args(a, csr, plan, el, er, H, neg_slope, spec, norm_scale, stats);
  if (rc) return rc;
  if (check_csr(csr)) return STAG_EINVAL;
  a.attn = attn_out;
  hipLaunchKernelGGL(gat_attn_kernel, dim3((a.n_units + 31) / 32), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_gat_bwd_edge(const stag_csr* csr, const stag_plan* plan, const float* el,
                                 const float* er, const float* ft, const float* stats, const float* g,
                                 const float* out, int32_t H, int32_t F, float neg_slope,
                                 const stag_noise_spec* spec, const float* norm_scale, float* de,
                                 float* dw, float* attn_out, void* stream) {
  if (check_csr_header(csr)) return STAG_EINVAL;
  if (!spec || spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI || spec->deriv) return STAG_EINVAL;
  if (!de || H <= 0 || F <= 0) return STAG_EINVAL;
  const int64_t HF64 = (int64_t)H * F;
  const int lph = F / 4;
  if (H > 64 || HF64 > 256 || F % 4 != 0 || (lph & (lph - 1)) != 0) return STAG_ENOSYS;
  if (spec->chunk_base != 0) return STAG_ENOSYS;
  if (spec->in_norm && !norm_scale) return STAG_EINVAL;
  if (csr->n_dst == 0 || csr->n_edges == 0) return STAG_OK;
  if (!csr->indices || !el || !er || !ft || !stats || !g || !out) return STAG_EINVAL;
  if (!aligned16(ft) || !aligned16(g) || !aligned16(out)) return STAG_EINVAL;
  if (spec->kind == STAG_NOISE_EXPLICIT && !spec->p0 && csr->n_edges > 0) return STAG_EINVAL;
  const int HF = (int)HF64;
  GatBwdArgs ba{};
  GatArgs& a = ba.f;
  const int rc = fill_edge_args(a, csr, plan, el, er, H, neg_slope, spec, norm_scale, stats);
  if (rc) return rc;
  if (check_csr(csr)) return STAG_EINVAL;
  a.ft = ft; a.F = F; a.HF = HF; a.attn = attn_out;
  ba.g = g; ba.gdo = nullptr; ba.out = out; ba.de = de; ba.dw = dw;
  const int lpe = lanes_for((HF + 3) / 4, 4);   // (H * F <= 256: at most a wave)
  const int tpb = 256 / lpe;
  const dim3 grid((a.n_units + tpb - 1) / tpb);
  const size_t lds_bytes = (size_t)3 * 256 * H * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  pick<64, 32, 16, 8, 4>(lpe, [&](auto L) {
    hipLaunchKernelGGL(gat_bwd_edge_kernel<decltype(L)::value>, grid, dim3(256), lds_bytes, s, ba);
  });
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// One call = the whole backward of stag_gat_fwd w.r.t. el, er, ft (and explicit weights): the edge pass
// over the forward CSR and the source pass over its transpose (see gat_bwd_edge_block_kernel).
extern "C" size_t stag_gat_bwd_workspace_bytes(int32_t n_seg, int32_t n_seg_t, int32_t H, int32_t F) {
  if (H <= 0 || F <= 0) return 0;
  const size_t a = n_seg > 0 ? (size_t)n_seg * (size_t)H : 0;
  const size_t b = n_seg_t > 0 ? (size_t)n_seg_t * (size_t)(H * F + H) : 0;
  return (a > b ? a : b) * sizeof(float);
}

// the end of a source pass: d_ft and d_el of the long source rows, from their segments' partials ws [n_seg_t][HF + H]
static void gat_src_finish(const stag_plan* plan_t, const float* ws, int H, int HF, float* d_ft, float* d_el, hipStream_t s) {
  if (plan_t->n_long <= 0) return;
  hipLaunchKernelGGL(gat_seg_finish_kernel, dim3(plan_t->n_long, (HF + 15) / 16), dim3(256), 0, s, ws, HF + H, 0, HF,
                     plan_t->long_rows, plan_t->long_seg_ptr, d_ft, HF);
  hipLaunchKernelGGL(gat_seg_finish_kernel, dim3(plan_t->n_long, (H + 15) / 16), dim3(256), 0, s, ws, HF + H, HF, H,
                     plan_t->long_rows, plan_t->long_seg_ptr, d_el, H);
}

extern "C" int stag_gat_bwd_two_pass(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                                     const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                                     const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                                     float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                                     const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft, float* dw,
                                     float* ade_ws, void* stream) {
  if (drop_on(drop)) return STAG_ENOSYS;               // attention dropout: stag_gat_bwd
  if (check_csr_header(csr) || !csr_t || !csr_t->indptr) return STAG_EINVAL;
  if (csr_t->n_edges != csr->n_edges || csr_t->n_dst != csr->n_src || csr_t->n_src != csr->n_dst) return STAG_EINVAL;
  if (!spec || spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI || spec->deriv) return STAG_EINVAL;
  if (!d_el || !d_er || !d_ft || !ade_ws || H <= 0 || F <= 0) return STAG_EINVAL;
  const int64_t HF64 = (int64_t)H * F;
  const int lphp = gat_blk_lphp(H, F);
  if (lphp == 0 || HF64 > 1024 || lphp != F / 4) return STAG_ENOSYS;   // this form: F / 4 a power of two, no idle lanes
  if (spec->chunk_base != 0) return STAG_ENOSYS;
  if (!plan || !plan_t || !plan->block_ptr || !plan_t->block_ptr || plan->n_blocks <= 0 || plan_t->n_blocks <= 0 ||
      plan->seg_len > kBlkEdges || plan_t->seg_len > kBlkEdges)
    return STAG_ENOSYS;                                   // needs the batch plans of both orientations
  if (spec->in_norm && !norm_scale) return STAG_EINVAL;
  if (csr->n_dst == 0 || csr->n_edges == 0) return STAG_OK;   // the caller zero-fills (no edge, no gradient)
  if (!csr->indices || !csr_t->indices || !csr_t->nidx || !el || !er || !ft || !stats || !g || !out) return STAG_EINVAL;
  if (!aligned16(ft) || !aligned16(g) || !aligned16(out) || !aligned16(d_ft) || !aligned16(ade_ws)) return STAG_EINVAL;
  if (spec->kind == STAG_NOISE_EXPLICIT && !spec->p0 && csr->n_edges > 0) return STAG_EINVAL;
  const int prc = check_positions(spec, csr->n_edges, H, spec->kind >= STAG_NOISE_NORMAL);
  if (prc) return prc;
  const int HF = (int)HF64;
  const size_t need = stag_gat_bwd_workspace_bytes(plan->n_seg, plan_t->n_seg, H, F);
  if (need > 0 && (!plan->workspace || plan->workspace_bytes < need)) return STAG_ENOMEM;
  hipStream_t s = (hipStream_t)stream;

  GatBwdBlkArgs ba{};
  GatArgs& a = ba.f;
  int rc = fill_edge_args(a, csr, plan, el, er, H, neg_slope, spec, norm_scale, stats);
  if (rc) return rc;
  // the source pass's plan too, before the edge pass is enqueued
  if (check_plan_units(plan_t, 0) || check_plan_segments(plan_t, kPlanSegPtr)) return STAG_EINVAL;
  if (check_csr(csr) || check_csr(csr_t)) return STAG_EINVAL;
  a.ft = ft; a.F = F; a.HF = HF;
  a.ft_bytes = narrow_extent(csr->n_src, (uint64_t)HF * 4u);
  const GatBlkShape sh = gat_blk_shape(a, plan, lphp, aligned16(er) && aligned16(stats));
  ba.g = g; ba.out = out; ba.ade = ade_ws; ba.d_er = d_er; ba.dw = dw; ba.ws = plan->workspace;
  const size_t lds_e = gat_lds((size_t)kBlkEdges * H * (dw ? 3 : 2), STAG_GAT_LDS_MIN_BWD);
  const dim3 ge(plan->n_blocks);
  gat_blk_dispatch(sh, [&](auto L, auto Cc, auto) {
    hipLaunchKernelGGL((gat_bwd_edge_block_kernel<decltype(L)::value, decltype(Cc)::value>), ge, dim3(kBlkThreads), lds_e,
                       s, ba);
  });
  if (plan->n_long > 0)
    hipLaunchKernelGGL(gat_seg_finish_kernel, dim3(plan->n_long, (H + 15) / 16), dim3(256), 0, s,
                       plan->workspace, H, 0, H, plan->long_rows, plan->long_seg_ptr, d_er, H);

  GatSrcBlkArgs sa{};
  sa.indices = csr_t->indices; sa.nidx = csr_t->nidx;
  sa.units = plan_t->units; sa.block_ptr = plan_t->block_ptr; sa.long_rows = plan_t->long_rows;
  sa.ade = ade_ws; sa.g = g; sa.H = H; sa.F = F; sa.HF = HF;
  sa.g_bytes = narrow_extent(csr->n_dst, (uint64_t)HF * 4u);
  sa.d_ft = d_ft; sa.d_el = d_el; sa.ws = plan->workspace;   // the edge pass's partials are consumed by now (stream order)
  const size_t lds_s = gat_lds((size_t)kBlkEdges * H * 2, STAG_GAT_LDS_MIN_BWD);
  const dim3 gs(plan_t->n_blocks);
  gat_blk_dispatch(sh, [&](auto L, auto Cc, auto) {
    hipLaunchKernelGGL((gat_bwd_src_block_kernel<decltype(L)::value, decltype(Cc)::value>), gs, dim3(kBlkThreads), lds_s,
                       s, sa);
  });
  gat_src_finish(plan_t, sa.ws, H, HF, d_ft, d_el, s);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" size_t stag_gat_bwd_scratch_bytes(int64_t n_dst, int64_t n_edges, int32_t H) {
  if (n_dst < 0 || n_edges < 0 || H <= 0) return 0;
  // two-pass form: a and de by forward position [E, 2H]; one-gather form: dsl [E, H] then the per-destination
  // records [n_dst, 4H]
  return ((size_t)2 * (size_t)n_edges + (size_t)4 * (size_t)n_dst) * (size_t)H * sizeof(float);
}

// the fixed-order reduction of per-block partials [gx][2][D] -> dp0 [D], dp1 [D] (api.hip: stag_agg_bwd_dp's stages)
namespace stag { int dp_reduce_partials(const float* part, int64_t gx, int32_t D, float* part2, float* dp0, float* dp1, hipStream_t s); }

static int gat_bwd_impl(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                        const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                        const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                        float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                        const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft, float* dw,
                        float* scratch, void* stream, float* dp0, float* dp1, float* dp_ws, int stages = 7);

extern "C" int stag_gat_bwd(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                            const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                            const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                            float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                            const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft, float* dw,
                            float* scratch, void* stream) {
  return gat_bwd_impl(csr, plan, csr_t, plan_t, el, er, ft, stats, g, out, H, F, neg_slope, spec, norm_scale, drop,
                      d_el, d_er, d_ft, dw, scratch, stream, nullptr, nullptr, nullptr);
}

extern "C" int stag_gat_bwd_stages(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                                   const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                                   const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                                   float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                                   const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft, float* scratch,
                                   int32_t stages, void* stream) {
  if (stages <= 0 || (stages & ~(STAG_GAT_BWD_ROWDOT | STAG_GAT_BWD_SOURCE | STAG_GAT_BWD_DER))) return STAG_EINVAL;
  return gat_bwd_impl(csr, plan, csr_t, plan_t, el, er, ft, stats, g, out, H, F, neg_slope, spec, norm_scale, drop,
                      d_el, d_er, d_ft, nullptr, scratch, stream, nullptr, nullptr, nullptr, stages);
}

extern "C" size_t stag_gat_bwd_dp_workspace_bytes(int32_t n_blocks_t, int32_t H) {
  if (n_blocks_t <= 0 || H <= 0) return 0;
  return ((size_t)n_blocks_t * 2u * (size_t)H + (size_t)256 * 2u * (size_t)H) * sizeof(float);
}

extern "C" int stag_gat_bwd_dp(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                               const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                               const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                               float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                               const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft,
                               float* dp0, float* dp1, float* scratch, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!spec || !dp0 || !dp1 || !plan_t) return STAG_EINVAL;
  if (spec->kind != STAG_NOISE_NORMAL && spec->kind != STAG_NOISE_UNIFORM) return STAG_EINVAL;
  if (spec->param_mode != STAG_PARAM_SCALAR && spec->param_mode != STAG_PARAM_PER_CHANNEL) return STAG_EINVAL;
  if (spec->in_norm) return STAG_EINVAL;          // the in-norm factor is not differentiated here
  if (csr && (csr->n_dst == 0 || csr->n_edges == 0)) {
    if (hipMemsetAsync(dp0, 0, sizeof(float) * H, (hipStream_t)stream) != hipSuccess) return STAG_EIO;
    if (hipMemsetAsync(dp1, 0, sizeof(float) * H, (hipStream_t)stream) != hipSuccess) return STAG_EIO;
    return STAG_OK;
  }
  if (!workspace || workspace_bytes < stag_gat_bwd_dp_workspace_bytes(plan_t->n_blocks, H)) return STAG_ENOMEM;
  return gat_bwd_impl(csr, plan, csr_t, plan_t, el, er, ft, stats, g, out, H, F, neg_slope, spec, norm_scale, drop,
                      d_el, d_er, d_ft, nullptr, scratch, stream, dp0, dp1, static_cast<float*>(workspace));
}

static int gat_bwd_impl(const stag_csr* csr, const stag_plan* plan, const stag_csr* csr_t,
                        const stag_plan* plan_t, const float* el, const float* er, const float* ft,
                        const float* stats, const float* g, const float* out, int32_t H, int32_t F,
                        float neg_slope, const stag_noise_spec* spec, const float* norm_scale,
                        const stag_gat_drop* drop, float* d_el, float* d_er, float* d_ft, float* dw,
                        float* scratch, void* stream, float* dp0, float* dp1, float* dp_ws, int stages) {
  if (check_csr_header(csr) || !csr_t || !csr_t->indptr) return STAG_EINVAL;
  if (csr_t->n_edges != csr->n_edges || csr_t->n_dst != csr->n_src || csr_t->n_src != csr->n_dst) return STAG_EINVAL;
  if (!spec || spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI || spec->deriv) return STAG_EINVAL;
  if (!d_el || !d_er || !d_ft || !scratch || H <= 0 || F <= 0) return STAG_EINVAL;
  const int64_t HF64 = (int64_t)H * F;
  const int lphp = gat_blk_lphp(H, F);                  // any F % 4 == 0: lanes past a head's channels idle
  if (lphp == 0 || HF64 > 1024) return STAG_ENOSYS;
  if (spec->chunk_base != 0) return STAG_ENOSYS;
  if (!plan_t || !plan_t->block_ptr || plan_t->n_blocks <= 0 || plan_t->seg_len > kBlkEdges) return STAG_ENOSYS;
  if (spec->in_norm && !norm_scale) return STAG_EINVAL;
  if (csr->n_dst == 0 || csr->n_edges == 0) return STAG_OK;   // the caller zero-fills (no edge, no gradient)
  if (!csr->indices || !csr_t->indices || !csr_t->nidx || !el || !er || !ft || !stats || !g || !out) return STAG_EINVAL;
  if (csr->eid && !csr_t->eid) return STAG_EINVAL;            // edge ids of the transposed positions
  if (!aligned16(ft) || !aligned16(g) || !aligned16(out) || !aligned16(d_ft) || !aligned16(scratch)) return STAG_EINVAL;
  if (spec->kind == STAG_NOISE_EXPLICIT && !spec->p0 && csr->n_edges > 0) return STAG_EINVAL;
  const int prc = check_positions(spec, csr->n_edges, H, spec->kind >= STAG_NOISE_NORMAL || drop_on(drop));
  if (prc) return prc;
  if (check_plan_units(plan_t, 0) || check_plan_segments(plan_t, kPlanSegPtr)) return STAG_EINVAL;
  const bool fplan = plan_in_use(plan);
  if (check_plan(plan, kPlanSegPtr)) return STAG_EINVAL;
  const int HF = (int)HF64;
  const size_t need = stag_gat_bwd_workspace_bytes(fplan ? plan->n_seg : 0, plan_t->n_seg, H, F);
  // segment partials of BOTH orientations live in the forward plan's workspace, one after the other
  if (need > 0 && (!plan || !plan->workspace || plan->workspace_bytes < need)) return STAG_ENOMEM;
  hipStream_t s = (hipStream_t)stream;
  float* dsl = scratch;
  float* pack = scratch + (size_t)csr->n_edges * H;        // 16-byte aligned whenever H % 4 == 0 (the vector form)

  // the source pass's arguments: its refusals come before the first launch too
  GatBwd1Args ba{};
  GatArgs& a = ba.f;
  const GatBlkShape sh = gat_blk_lanes(H, lphp, plan_t);
  if (stages & STAG_GAT_BWD_SOURCE) {
    const int rc = fill_edge_args(a, csr_t, plan_t, el, er, H, neg_slope, spec, norm_scale, stats);
    if (rc) return rc;
    if (fill_drop(a, drop)) return STAG_EINVAL;
  }
  if (check_csr(csr) || check_csr(csr_t)) return STAG_EINVAL;

  // 1. sdot[v,h] = <G[v,h,:], out[v,h,:]>
  if (stages & STAG_GAT_BWD_ROWDOT) {
    const int rl = sh.lpe < lphp ? lphp : sh.lpe;               // a head's lanes inside one team
    const int64_t rpb = (int64_t)(256 / rl) * kRowdotRows;
    const dim3 gr((unsigned)((csr->n_dst + rpb - 1) / rpb));
    pick<64, 32, 16, 8, 4>(rl, [&](auto L) {
      hipLaunchKernelGGL((gat_rowdot_kernel<decltype(L)::value>), gr, dim3(256), 0, s, g, out, csr->n_dst, H, F, HF, lphp,
                         er, stats, pack);
    });
  }

  // 2. the source-major pass
  if (stages & STAG_GAT_BWD_SOURCE) {
  a.ft = ft; a.F = F; a.HF = HF;
  gat_blk_shape(a, plan_t, lphp, aligned16(pack));     // (er and the statistics travel in pack)
  ba.g = g; ba.pack = pack; ba.d_ft = d_ft; ba.d_el = d_el; ba.dsl = dsl; ba.dw = dw;
  ba.dp_part = dp_ws;
  ba.ws = plan ? plan->workspace : nullptr;
  ba.eid_is_pos = csr->eid ? 0 : 1;
  ba.g_bytes = narrow_extent(csr->n_dst, (uint64_t)HF * 4u);
  const size_t lds_s = gat_lds((size_t)kBlkEdges * H * ((dw || dp_ws) ? 4 : 3), STAG_GAT_LDS_MIN_ONE);
  const dim3 gs(plan_t->n_blocks);
  gat_blk_dispatch(sh, [&](auto L, auto Cc, auto) {
    hipLaunchKernelGGL((gat_bwd_one_kernel<decltype(L)::value, decltype(Cc)::value>), gs, dim3(kBlkThreads), lds_s, s, ba);
  });
  gat_src_finish(plan_t, ba.ws, H, HF, d_ft, d_el, s);
  }

  // 3. d er: the in-edges of a row are contiguous in dsl (the source pass's partials are consumed by now)
  if (stages & STAG_GAT_BWD_DER) {
  const int n_units_f = fplan ? plan->n_units : csr->n_dst;
  const int64_t nth = (int64_t)n_units_f * H;
  hipLaunchKernelGGL(gat_der_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s,
                     fplan ? static_cast<const stag_unit*>(plan->units) : nullptr, n_units_f, csr->indptr, dsl, H, d_er,
                     plan ? plan->workspace : nullptr);
  if (fplan && plan->n_long > 0)
    hipLaunchKernelGGL(gat_seg_finish_kernel, dim3(plan->n_long, (H + 15) / 16), dim3(256), 0, s,
                       plan->workspace, H, 0, H, plan->long_rows, plan->long_seg_ptr, d_er, H);
  }
  if (dp_ws) {
    const int rc2 = stag::dp_reduce_partials(dp_ws, plan_t->n_blocks, H, dp_ws + (size_t)plan_t->n_blocks * 2u * (size_t)H, dp0, dp1, s);
    if (rc2) return rc2;
  }
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}
