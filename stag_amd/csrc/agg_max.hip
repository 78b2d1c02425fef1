// agg_max.hip — the max reducer (DGL's fn.max; GraphSAGE 'pool', stag/zoo/graph_sage.py:90-93) as fused passes.
//
//   m[e, c]   = w[e, c] * x[src_e, c]                     one fp32 multiply; w drawn in the kernel as stag_agg_fwd does
//   out[v, c] = max_e m[e, c] over the in-edges of v      +0.0 for a row without in-edges
//   cnt[v, c] = #{e : m[e, c] == out[v, c]}
//
// Forward: the units of the launch plan (whole rows, <= seg_len segments of long rows), LPE lanes per unit, four
// channels per lane; per channel a running maximum and a tie count.  The comparisons are explicit (`>` then `==`,
// then NaN), never v_max / fmaxf: those would drop a NaN message and could turn a -0.0 maximum into +0.0.  A segment
// leaves its (max, count) pair in the plan's workspace; a second small launch merges the segments of every long row
// in segment order (strict `>` keeps the earlier segment's bits, equal maxima add their counts).  Max and count are
// exact, so both outputs are bit-identical for every seg_len, unit order and channel tiling.
//
// Backward: a prep launch interleaves (out, g / cnt) per four channels into one [n_dst][ceil(D/4)][8] array, then one
// pass over the source-major CSR: a unit's own row is x[u], every out-edge fetches 32 contiguous bytes of the
// destination's record, redraws w from the forward position (nidx), recomputes m bit for bit and sends g / cnt
// where m equals the maximum.  Sums run in edge order inside a unit and in segment order across segments.
#include "agg_max.hpp"
#include "entry_args.hpp"

namespace stag {
namespace {

constexpr int kMaxBlk = 4;   // out-edges fetched together by a team

__device__ __forceinline__ void max_step(float m, float& best, int& n) {
  if (m > best) { best = m; n = 1; }
  else if (m == best) { n += 1; }
  else if (m != m && best == best) { best = m; n = 0; }   // the first NaN wins and stays: it equals nothing
}

// merge a later partial (b, nb) into (best, n)
__device__ __forceinline__ void max_merge(float b, int nb, float& best, int& n) {
  if (best != best) return;
  if (b != b) { best = b; n = 0; }
  else if (b > best) { best = b; n = nb; }
  else if (b == best) { n += nb; }
}

// a row without messages (count 0 and not NaN) is +0.0
__device__ __forceinline__ float max_final(float best, int n) { return (n == 0 && best == best) ? 0.0f : best; }

// the unit a team serves: false when there is none (past the end, or a null record of the XCD-aware order)
template <int LPE>
__device__ __forceinline__ bool max_unit(const MaxArgs& a, int& row, int& start, int& len, int& slot) {
  constexpr int T = 256 / LPE;
  const int team = threadIdx.x / LPE;
  int64_t rec;
  if (a.xcd) {
    const int s = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int jh = (a.sh + T - 1) / T;
    if (j < jh) {
      const int i = j * T + team;
      if (i >= a.sh) return false;
      rec = (int64_t)s * a.sh + i;
    } else {
      const int i = (j - jh) * T + team;
      if (i >= a.sl) return false;
      rec = (int64_t)STAG_XCD_STRIPES * a.sh + (int64_t)s * a.sl + i;
    }
  } else {
    rec = (int64_t)blockIdx.x * T + team;
    if (rec >= a.n_units) return false;
  }
  if (a.units) {
    const int4 q = *reinterpret_cast<const int4*>(a.units + rec);
    if (q.x < 0 && q.w < 0) return false;
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

template <bool VEC>
__device__ __forceinline__ void ld4(const float* p, int k0, int D, float (&v)[4]) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p + k0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (k0 + q < D) ? p[k0 + q] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void st4(float* p, int k0, int D, const float (&v)[4]) {
  if (VEC) {
    *reinterpret_cast<float4*>(p + k0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k0 + q < D) p[k0 + q] = v[q];
  }
}

// the parameters of channels k0..k0+3 of edge `ed` (stag_noise_materialize's edge_w4, field for field)
__device__ __forceinline__ void params4(const MaxArgs& a, int64_t ed, int k0, float (&pa)[4], float (&pb)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + j;
    const bool in = k < a.D;
    float q0 = a.p0s, q1 = a.p1s;
    if (a.pmode == STAG_PARAM_PER_CHANNEL) { q0 = in ? a.p0[k] : 0.f; q1 = (in && a.p1) ? a.p1[k] : 0.f; }
    else if (a.pmode == STAG_PARAM_PER_EDGE1) { q0 = a.p0[ed]; q1 = a.p1 ? a.p1[ed] : 0.f; }
    else if (a.pmode == STAG_PARAM_PER_EDGE) {
      q0 = in ? a.p0[ed * a.D + k] : 0.f;
      q1 = (in && a.p1) ? a.p1[ed * a.D + k] : 0.f;
    }
    if (a.pmode != STAG_PARAM_SCALAR && (a.nflags & kFlagLogScale)) q1 = exp_scale(q1);   // scalar: on the host
    pa[j] = q0; pb[j] = q1;
  }
}

// w of channels k0..k0+3 of the edge at CSR position p (forward position fp, edge id ed); GRAD: and dw/dp0, dw/dp1
template <int KIND, bool GRAD>
__device__ __forceinline__ void weight4(const MaxArgs& a, const PhiloxKey& key, int64_t fp, int64_t ed, int k0,
                                        uint32_t chunk, const float (&pc)[4], const float (&qc)[4], float (&w)[4],
                                        float (&d0)[4], float (&d1)[4]) {
  if constexpr (KIND == kNone) {
    w[0] = w[1] = w[2] = w[3] = 1.0f;
  } else if constexpr (KIND == kExplicit) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t = (k0 + q < a.D) ? a.p0[ed * a.D + k0 + q] : 0.f;
      w[q] = (a.nflags & kFlagRelu) ? fmaxf(t, 0.f) : t;
    }
  } else {
    float pa[4], pb[4];
    if (a.pmode >= STAG_PARAM_PER_EDGE1) {
      params4(a, ed, k0, pa, pb);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) { pa[q] = pc[q]; pb[q] = qc[q]; }
    }
    const int64_t gpos = a.pos_base + fp;
    if constexpr (GRAD) draw4_grad<KIND>((uint32_t)gpos, ctr1_of(gpos, chunk), key, pa, pb, a.nflags, w, d0, d1);
    else draw4<KIND>((uint32_t)gpos, ctr1_of(gpos, chunk), key, pa, pb, a.nflags, w);
  }
}

template <int KIND, int LPE, bool VEC>
__global__ __launch_bounds__(256) void agg_max_fwd_kernel(const MaxArgs a) {
  const int c = blockIdx.y * LPE + threadIdx.x % LPE;
  const int k0 = 4 * c;
  int row, start, len, slot;
  if (k0 >= a.D || !max_unit<LPE>(a, row, start, len, slot)) return;
  const PhiloxKey key = resolve_epoch(a.key);
  const uint32_t chunk = a.chunk_base + (uint32_t)c;
  float pc[4] = {0.f, 0.f, 0.f, 0.f}, qc[4] = {0.f, 0.f, 0.f, 0.f};
  if (KIND >= kNormal && a.pmode <= STAG_PARAM_PER_CHANNEL) params4(a, 0, k0, pc, qc);
  float best[4];
  int n[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) best[q] = -__builtin_inff();
  const int end = start + len;
  for (int p0 = start; p0 < end; p0 += kMaxBlk) {
    int u[kMaxBlk];
    int64_t ed[kMaxBlk], fp[kMaxBlk];
    float xv[kMaxBlk][4];
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j) {
      const int p = p0 + j;
      if (p < end) {
        u[j] = a.indices[p];
        ed[j] = a.eid ? a.eid[p] : p;
        fp[j] = a.nidx ? a.nidx[p] : p;
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j)
      if (p0 + j < end) ld4<VEC>(a.x + (int64_t)u[j] * a.ldx, k0, a.D, xv[j]);
    // one edge at a time in CSR order: draw (while the block's rows are in flight), multiply, compare
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j) {
      if (p0 + j < end) {
        float w[4], d0[4], d1[4];
        weight4<KIND, false>(a, key, fp[j], ed[j], k0, chunk, pc, qc, w, d0, d1);
#pragma unroll
        for (int q = 0; q < 4; ++q) max_step(KIND == kNone ? xv[j][q] : w[q] * xv[j][q], best[q], n[q]);
      }
    }
  }
  if (slot >= 0) {   // a segment: its partial, merged by agg_max_merge_kernel
    float* ws = a.ws + (int64_t)slot * 2 * a.D;
    float nf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) nf[q] = __int_as_float(n[q]);
    st4<VEC>(ws, k0, a.D, best);
    st4<VEC>(ws + a.D, k0, a.D, nf);
    return;
  }
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = max_final(best[q], n[q]);
  st4<VEC>(a.out + (int64_t)row * a.ldo, k0, a.D, o);
  if (a.cnt) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k0 + q < a.D) a.cnt[(int64_t)row * a.ldc + k0 + q] = n[q];
  }
}

// one team per long row: its segments' (max, count) pairs in segment order, eight segments' pairs in flight
template <int LPE, bool VEC>
__global__ __launch_bounds__(256) void agg_max_merge_kernel(const MaxArgs a) {
  constexpr int kAhead = 8;
  const int r = blockIdx.x * (256 / LPE) + threadIdx.x / LPE;
  const int k0 = 4 * (blockIdx.y * LPE + threadIdx.x % LPE);
  if (r >= a.n_long || k0 >= a.D) return;
  const int row = a.long_rows[r];
  const int s0 = a.long_seg_ptr[r], s1 = a.long_seg_ptr[r + 1];
  float best[4];
  int n[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) best[q] = -__builtin_inff();
  for (int s = s0; s < s1; s += kAhead) {
    float bv[kAhead][4], nv[kAhead][4];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (s + j < s1) {
        const float* ws = a.ws + (int64_t)(s + j) * 2 * a.D;
        ld4<VEC>(ws, k0, a.D, bv[j]);
        ld4<VEC>(ws + a.D, k0, a.D, nv[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (s + j < s1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) max_merge(bv[j][q], __float_as_int(nv[j][q]), best[q], n[q]);
      }
    }
  }
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = max_final(best[q], n[q]);
  st4<VEC>(a.out + (int64_t)row * a.ldo, k0, a.D, o);
  if (a.cnt) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k0 + q < a.D) a.cnt[(int64_t)row * a.ldc + k0 + q] = n[q];
  }
}

// og[v][c][0..3] = out[v, 4c..4c+3], og[v][c][4..7] = g / cnt there (0 where cnt is 0 and past D)
__global__ __launch_bounds__(256) void agg_max_prep_kernel(const MaxArgs a) {
  const int nchunk = (a.D + 3) / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.n_og_rows * nchunk) return;
  const int64_t v = i / nchunk;
  const int k0 = 4 * (int)(i - v * nchunk);
  float o[4], gq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + q;
    o[q] = 0.f;
    gq[q] = 0.f;
    if (k < a.D) {
      const int64_t at = v * a.ldf + k;
      const int n = a.cnt_in[at];
      o[q] = a.out_in[at];
      gq[q] = n > 0 ? a.g[at] / (float)n : 0.f;
    }
  }
  float4* dst = reinterpret_cast<float4*>(a.og + i * 8);
  dst[0] = make_float4(o[0], o[1], o[2], o[3]);
  dst[1] = make_float4(gq[0], gq[1], gq[2], gq[3]);
}

// NO = 1: dx; 3: dx and the two parameter-derivative aggregates
template <int KIND, int LPE, bool VEC, int NO>
__global__ __launch_bounds__(256) void agg_max_bwd_kernel(const MaxArgs a) {
  constexpr bool GRAD = NO == 3;
  const int c = blockIdx.y * LPE + threadIdx.x % LPE;
  const int k0 = 4 * c;
  int row, start, len, slot;
  if (k0 >= a.D || !max_unit<LPE>(a, row, start, len, slot)) return;
  const PhiloxKey key = resolve_epoch(a.key);
  const uint32_t chunk = a.chunk_base + (uint32_t)c;
  const int nchunk = (a.D + 3) / 4;
  float pc[4] = {0.f, 0.f, 0.f, 0.f}, qc[4] = {0.f, 0.f, 0.f, 0.f};
  if (KIND >= kNormal && a.pmode <= STAG_PARAM_PER_CHANNEL) params4(a, 0, k0, pc, qc);
  float xo[4];
  ld4<VEC>(a.x + (int64_t)row * a.ldx, k0, a.D, xo);
  float acc[NO][4];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[o][q] = 0.f;
  const int end = start + len;
  for (int p0 = start; p0 < end; p0 += kMaxBlk) {
    int v[kMaxBlk];
    int64_t ed[kMaxBlk], fp[kMaxBlk];
    float ov[kMaxBlk][4], gv[kMaxBlk][4];
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j) {
      const int p = p0 + j;
      if (p < end) {
        v[j] = a.indices[p];
        ed[j] = a.eid ? a.eid[p] : p;
        fp[j] = a.nidx ? a.nidx[p] : p;
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j) {
      if (p0 + j < end) {
        const float4* rec = reinterpret_cast<const float4*>(a.og + ((int64_t)v[j] * nchunk + c) * 8);
        const float4 t0 = rec[0], t1 = rec[1];
        ov[j][0] = t0.x; ov[j][1] = t0.y; ov[j][2] = t0.z; ov[j][3] = t0.w;
        gv[j][0] = t1.x; gv[j][1] = t1.y; gv[j][2] = t1.z; gv[j][3] = t1.w;
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxBlk; ++j) {
      if (p0 + j < end) {
        float w[4], d0[4], d1[4];
        weight4<KIND, GRAD>(a, key, fp[j], ed[j], k0, chunk, pc, qc, w, d0, d1);
        float t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float m = KIND == kNone ? xo[q] : w[q] * xo[q];
          t[q] = (m == ov[j][q]) ? gv[j][q] : 0.0f;
          acc[0][q] = KIND == kNone ? acc[0][q] + t[q] : __builtin_fmaf(w[q], t[q], acc[0][q]);
          if constexpr (GRAD) {
            acc[1][q] = __builtin_fmaf(d0[q], t[q], acc[1][q]);
            acc[2][q] = __builtin_fmaf(d1[q], t[q], acc[2][q]);
          }
        }
        if (KIND == kExplicit && a.dw) {
          float dwv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) dwv[q] = xo[q] * t[q];
          st4<false>(a.dw + ed[j] * a.ldw, k0, a.D, dwv);
        }
      }
    }
  }
  if (slot >= 0) {   // a segment of a long source row: partial sums, added by agg_max_bwd_merge_kernel
    float* ws = a.ws + (int64_t)slot * NO * a.D;
#pragma unroll
    for (int o = 0; o < NO; ++o) st4<VEC>(ws + o * a.D, k0, a.D, acc[o]);
    return;
  }
  if (a.dx) st4<VEC>(a.dx + (int64_t)row * a.ldd, k0, a.D, acc[0]);
  if constexpr (GRAD) {
    st4<VEC>(a.dp0 + (int64_t)row * a.ldd, k0, a.D, acc[1]);
    st4<VEC>(a.dp1 + (int64_t)row * a.ldd, k0, a.D, acc[2]);
  }
}

// one team per long source row: its segments' sums added in segment order
template <int LPE>
__global__ __launch_bounds__(256) void agg_max_bwd_merge_kernel(const MaxArgs a) {
  const int r = blockIdx.x * (256 / LPE) + threadIdx.x / LPE;
  const int k0 = 4 * (blockIdx.y * LPE + threadIdx.x % LPE);
  if (r >= a.n_long || k0 >= a.D) return;
  const int row = a.long_rows[r];
  const int s0 = a.long_seg_ptr[r], s1 = a.long_seg_ptr[r + 1];
  float* outs[3] = {a.dx, a.dp0, a.dp1};
  for (int o = 0; o < a.nws; ++o) {
    if (!outs[o]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + q;
      if (k >= a.D) break;
      float sum = 0.f;
      for (int s = s0; s < s1; ++s) sum += a.ws[((int64_t)s * a.nws + o) * a.D + k];
      outs[o][(int64_t)row * a.ldd + k] = sum;
    }
  }
}

dim3 unit_grid(const MaxArgs& a, int lpe) {
  const int T = 256 / lpe;
  const int tiles = ((a.D + 3) / 4 + lpe - 1) / lpe;
  if (a.xcd) {
    const int64_t jb = (a.sh + T - 1) / T + (a.sl + T - 1) / T;
    return dim3((unsigned)(STAG_XCD_STRIPES * jb), tiles);
  }
  return dim3((unsigned)((a.n_units + T - 1) / T), tiles);
}

template <int KIND>
void fwd_kind(const MaxArgs& a, int lpe, bool vec, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4, 2, 1>(lpe, vec, [&](auto L, auto V) {
    hipLaunchKernelGGL((agg_max_fwd_kernel<KIND, decltype(L)::value, decltype(V)::value>), grid, dim3(256), 0, s, a);
  });
}

template <int KIND, int NO>
void bwd_kind(const MaxArgs& a, int lpe, bool vec, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8, 4, 2, 1>(lpe, vec, [&](auto L, auto V) {
    hipLaunchKernelGGL((agg_max_bwd_kernel<KIND, decltype(L)::value, decltype(V)::value, NO>), grid, dim3(256), 0, s, a);
  });
}

}  // namespace

hipError_t max_fwd_launch(const MaxArgs& a, int32_t n_seg, hipStream_t s) {
  const int lpe = lanes_for((a.D + 3) / 4, 1);
  const bool vec = a.D % 4 == 0 && a.ldx % 4 == 0 && a.ldo % 4 == 0 && aligned16(a.x) && aligned16(a.out) &&
                   (n_seg == 0 || aligned16(a.ws));
  const dim3 grid = unit_grid(a, lpe);
  if (grid.x > 0)
    pick<kNone, kExplicit, kNormal, kUniform, kBernoulli>(a.kind, [&](auto K) { fwd_kind<decltype(K)::value>(a, lpe, vec, grid, s); });
  if (n_seg > 0 && a.n_long > 0) {
    const int T = 256 / lpe;
    const dim3 mg((a.n_long + T - 1) / T, grid.y);
    pick<64, 32, 16, 8, 4, 2, 1>(lpe, vec, [&](auto L, auto V) {
      hipLaunchKernelGGL((agg_max_merge_kernel<decltype(L)::value, decltype(V)::value>), mg, dim3(256), 0, s, a);
    });
  }
  return hipGetLastError();
}

hipError_t max_bwd_launch(const MaxArgs& a, int32_t n_seg, hipStream_t s) {
  const int nchunk = (a.D + 3) / 4;
  const int64_t n_prep = (int64_t)a.n_og_rows * nchunk;
  if (n_prep > 0)
    hipLaunchKernelGGL(agg_max_prep_kernel, dim3((unsigned)((n_prep + 255) / 256)), dim3(256), 0, s, a);
  const int lpe = lanes_for((a.D + 3) / 4, 1);
  const bool vec = a.D % 4 == 0 && a.ldx % 4 == 0 && a.ldd % 4 == 0 && aligned16(a.x) && (!a.dx || aligned16(a.dx)) &&
                   (!a.dp0 || (aligned16(a.dp0) && aligned16(a.dp1))) && (n_seg == 0 || aligned16(a.ws));
  const dim3 grid = unit_grid(a, lpe);
  const bool grad = a.dp0 != nullptr;
  if (grid.x > 0) {
    pick<kNone, kExplicit, kNormal, kUniform, kBernoulli>(a.kind, [&](auto K) {
      constexpr int KIND = decltype(K)::value;
      constexpr bool reparam = KIND == kNormal || KIND == kUniform;   // the kinds with parameter gradients
      if (reparam && grad) bwd_kind<KIND, reparam ? 3 : 1>(a, lpe, vec, grid, s);
      else bwd_kind<KIND, 1>(a, lpe, vec, grid, s);
    });
  }
  if (n_seg > 0 && a.n_long > 0) {
    const int T = 256 / lpe;
    const dim3 mg((a.n_long + T - 1) / T, grid.y);
    pick<64, 32, 16, 8, 4, 2, 1>(lpe, [&](auto L) {
      hipLaunchKernelGGL((agg_max_bwd_merge_kernel<decltype(L)::value>), mg, dim3(256), 0, s, a);
    });
  }
  return hipGetLastError();
}

}  // namespace stag
