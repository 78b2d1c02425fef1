// reorder.hip — a node order with L2 locality for a graph whose ids are arbitrary (graph preprocessing, not the hot
// path).  Every aggregation kernel gathers x[u] for the sources of a destination row; the XCD-aware walk
// (stag_plan.xcd_order) only pays when those sources lie near the destination in the ROW ORDER, which a citation or
// social graph with scrambled ids does not offer.  stag_reorder_locality finds an order that does:
//   1. coordinates x[v, j], j < dims, uniform in [-1, 1) from the project's Philox keyed by (seed, node, j / 4);
//   2. `rounds` smoothing rounds on the symmetrised graph, double-buffered:
//        x'[v] = (x[v] + sum_in x[u] + sum_out x[w]) / (1 + indeg + outdeg)
//      in-edges in csr position order, then out-edges in csr_t position order; after each round every column is
//      centred and divided by its standard deviation (fixed-order two-level reduction, a column without deviation is
//      left alone) — nodes of one community drift to the same corner of the cube, a hub cannot pull the rest along
//      because every column is re-spread every round;
//   3. key[v] = the signs of x[v, :], column 0 most significant;
//   4. stable radix sort of (key, node id): perm[new] = old; inv[perm[i]] = i.
// No float atomics and no order that depends on scheduling anywhere: the result is a pure function of the inputs.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kStatRows = 1024;      // rows one block of the first reduction level sums

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// x[v, 4c .. 4c+3] = 2 u - 1, u the four uniforms of the Philox block at (position v, chunk c)
__global__ __launch_bounds__(kThreads) void reorder_init_kernel(float* x, int32_t n, int32_t L, stag::PhiloxKey key) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)n * L) return;
  const int64_t v = i / L;
  const uint32_t c = (uint32_t)(i - v * L);
  uint32_t r[4];
  stag::philox_at(v, c, key, r);
  float4 o;
  o.x = 2.0f * stag::u01(r[0]) - 1.0f;
  o.y = 2.0f * stag::u01(r[1]) - 1.0f;
  o.z = 2.0f * stag::u01(r[2]) - 1.0f;
  o.w = 2.0f * stag::u01(r[3]) - 1.0f;
  reinterpret_cast<float4*>(x)[i] = o;
}

__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// the rows idx[b, e) of x, added to acc one after the other (four loads in flight, the adds in position order)
__device__ __forceinline__ void add_rows(float4& acc, const float4* x4, const int32_t* idx, int32_t b, int32_t e, int L, int c) {
  int32_t p = b;
  for (; p + 4 <= e; p += 4) {
    const int32_t u0 = idx[p], u1 = idx[p + 1], u2 = idx[p + 2], u3 = idx[p + 3];
    const float4 a0 = x4[(int64_t)u0 * L + c], a1 = x4[(int64_t)u1 * L + c];
    const float4 a2 = x4[(int64_t)u2 * L + c], a3 = x4[(int64_t)u3 * L + c];
    add4(acc, a0); add4(acc, a1); add4(acc, a2); add4(acc, a3);
  }
  for (; p < e; ++p) add4(acc, x4[(int64_t)idx[p] * L + c]);
}

// one smoothing round: a team of L = dims / 4 lanes per node, a lane owns 4 columns
__global__ __launch_bounds__(kThreads) void reorder_smooth_kernel(const float* xin, float* xout, int32_t n, int32_t L,
                                                                  const int32_t* indptr, const int32_t* indices,
                                                                  const int32_t* indptr_t, const int32_t* indices_t) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)n * L) return;
  const int32_t v = (int32_t)(i / L);
  const int c = (int)(i - (int64_t)v * L);
  const float4* x4 = reinterpret_cast<const float4*>(xin);
  float4 acc = x4[i];
  const int32_t b0 = indptr[v], e0 = indptr[v + 1];
  const int32_t b1 = indptr_t[v], e1 = indptr_t[v + 1];
  add_rows(acc, x4, indices, b0, e0, L, c);
  add_rows(acc, x4, indices_t, b1, e1, L, c);
  const float d = (float)(1 + (e0 - b0) + (e1 - b1));
  acc.x /= d; acc.y /= d; acc.z /= d; acc.w /= d;
  reinterpret_cast<float4*>(xout)[i] = acc;
}

// first level of the column statistics: block b leaves part[b][0][j] = sum, part[b][1][j] = sum of squares of column j
// over rows [b * kStatRows, ...): a lane walks its rows in order, then the lanes are added in lane order.
__global__ __launch_bounds__(kThreads) void reorder_stats1_kernel(const float* x, int32_t n, int32_t L, float* part) {
  __shared__ float s[kThreads][8];
  const int t = threadIdx.x;
  const int rp = kThreads / L;                 // rows a pass of the block covers (L in 1..8: the last lanes may idle)
  const int slot = t / L, c = t - slot * L;
  const int64_t r0 = (int64_t)blockIdx.x * kStatRows;
  const int64_t r1 = r0 + kStatRows < n ? r0 + kStatRows : n;
  float4 su = make_float4(0.f, 0.f, 0.f, 0.f), sq = su;
  if (slot < rp) {
    for (int64_t r = r0 + slot; r < r1; r += rp) {
      const float4 a = reinterpret_cast<const float4*>(x)[r * L + c];
      add4(su, a);
      add4(sq, make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w));
    }
  }
  s[t][0] = su.x; s[t][1] = su.y; s[t][2] = su.z; s[t][3] = su.w;
  s[t][4] = sq.x; s[t][5] = sq.y; s[t][6] = sq.z; s[t][7] = sq.w;
  __syncthreads();
  const int dims = 4 * L;
  if (t < 2 * dims) {
    const int which = t / dims, j = t - which * dims;
    const int cc = j >> 2, w = (j & 3) + 4 * which;
    float sum = 0.f;
    for (int k = 0; k < rp; ++k) sum += s[k * L + cc][w];
    part[((int64_t)blockIdx.x * 2 + which) * dims + j] = sum;
  }
}

// second level: the blocks' partials in block order (in double), then stats[j] = mean, stats[dims + j] = 1 / deviation.
// A column whose deviation is zero (below rounding: var <= 1e-10 of its mean square) is left alone: mean 0, factor 1.
__global__ __launch_bounds__(64) void reorder_stats2_kernel(const float* part, int32_t nblk, int32_t dims, int32_t n, float* stats) {
  __shared__ double tot[64];
  const int t = threadIdx.x;
  if (t < 2 * dims) {
    double sum = 0.0;
    for (int32_t b = 0; b < nblk; ++b) sum += (double)part[(int64_t)b * 2 * dims + t];
    tot[t] = sum;
  }
  __syncthreads();
  if (t < dims) {
    const double mean = tot[t] / n, msq = tot[dims + t] / n;
    const double var = msq - mean * mean;
    const bool flat = !(var > 1e-10 * msq);
    stats[t] = flat ? 0.0f : (float)mean;
    stats[dims + t] = flat ? 1.0f : (float)(1.0 / sqrt(var));
  }
}

__global__ __launch_bounds__(kThreads) void reorder_normalise_kernel(float* x, int32_t n, int32_t L, const float* stats) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)n * L) return;
  const int c = (int)(i % L);
  const float4 m = reinterpret_cast<const float4*>(stats)[c];
  const float4 f = reinterpret_cast<const float4*>(stats)[L + c];
  float4 a = reinterpret_cast<float4*>(x)[i];
  a.x = (a.x - m.x) * f.x; a.y = (a.y - m.y) * f.y; a.z = (a.z - m.z) * f.z; a.w = (a.w - m.w) * f.w;
  reinterpret_cast<float4*>(x)[i] = a;
}

// key[v]: bit (dims - 1 - j) = x[v, j] > 0; ids[v] = v
__global__ __launch_bounds__(kThreads) void reorder_keys_kernel(const float* x, int32_t n, int32_t L, uint32_t* keys, int32_t* ids) {
  const int32_t v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= n) return;
  uint32_t k = 0;
  for (int c = 0; c < L; ++c) {
    const float4 a = reinterpret_cast<const float4*>(x)[(int64_t)v * L + c];
    k = (k << 4) | ((a.x > 0.f ? 8u : 0u) | (a.y > 0.f ? 4u : 0u) | (a.z > 0.f ? 2u : 0u) | (a.w > 0.f ? 1u : 0u));
  }
  keys[v] = k;
  ids[v] = v;
}

__global__ __launch_bounds__(kThreads) void reorder_inverse_kernel(const int32_t* perm, int32_t n, int32_t* inv) {
  const int32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) inv[perm[i]] = i;
}

__global__ __launch_bounds__(kThreads) void relabel_edges_kernel(const int32_t* src, const int32_t* dst, int64_t E, const int32_t* inv,
                                                                 int32_t* src_out, int32_t* dst_out) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  src_out[e] = inv[src[e]];
  dst_out[e] = inv[dst[e]];
}

bool dims_ok(int32_t dims) { return dims >= 4 && dims <= 32 && dims % 4 == 0; }

struct ReorderWs {
  float *x0, *x1, *part, *stats;
  uint32_t *keys, *keys_s;
  int32_t* ids;
  void* tmp;
  size_t tmp_bytes, total;
};

// the pieces of the workspace (base == nullptr: sizes only)
ReorderWs reorder_ws(void* base, int32_t n, int32_t dims) {
  ReorderWs w{};
  const size_t xs = align_up((size_t)n * dims * 4), ks = align_up((size_t)n * 4);
  const size_t nblk = ((size_t)n + kStatRows - 1) / kStatRows;
  const size_t ps = align_up(nblk * 2 * dims * 4), ss = align_up((size_t)2 * dims * 4);
  size_t sort_tmp = 0;
  uint32_t* ku = nullptr;
  int32_t* null = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, ku, ku, null, null, (size_t)n, 0u, (unsigned)dims);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  w.x0 = reinterpret_cast<float*>(p + off); off += xs;
  w.x1 = reinterpret_cast<float*>(p + off); off += xs;
  w.part = reinterpret_cast<float*>(p + off); off += ps;
  w.stats = reinterpret_cast<float*>(p + off); off += ss;
  w.keys = reinterpret_cast<uint32_t*>(p + off); off += ks;
  w.keys_s = reinterpret_cast<uint32_t*>(p + off); off += ks;
  w.ids = reinterpret_cast<int32_t*>(p + off); off += ks;
  w.tmp = p + off;
  w.tmp_bytes = align_up(sort_tmp);
  w.total = off + w.tmp_bytes;
  return w;
}

}  // namespace

extern "C" size_t stag_reorder_workspace_bytes(int32_t n, int64_t n_edges, int32_t dims) {
  (void)n_edges;                         // (the edges are read where they lie: nothing per edge is kept)
  if (n <= 0 || !dims_ok(dims)) return 256;
  return reorder_ws(nullptr, n, dims).total;
}

extern "C" int stag_reorder_locality(const stag_csr* csr, const stag_csr* csr_t, int32_t dims, int32_t rounds, uint64_t seed,
                                     int32_t* perm, int32_t* inv, void* workspace, size_t workspace_bytes, void* stream) {
  if (!csr || !csr_t || !perm || !inv || !dims_ok(dims) || rounds < 0) return STAG_EINVAL;
  const int32_t n = csr->n_dst;
  if (n < 0 || csr->n_edges < 0 || csr->n_src != n) return STAG_EINVAL;
  if (csr_t->n_dst != n || csr_t->n_src != n || csr_t->n_edges != csr->n_edges) return STAG_EINVAL;
  if (n == 0) return STAG_OK;
  if (!csr->indptr || !csr_t->indptr) return STAG_EINVAL;
  if (csr->n_edges > 0 && (!csr->indices || !csr_t->indices)) return STAG_EINVAL;
  if (!workspace || workspace_bytes < stag_reorder_workspace_bytes(n, csr->n_edges, dims)) return STAG_ENOMEM;
  if (((uintptr_t)workspace & 15)) return STAG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const ReorderWs w = reorder_ws(workspace, n, dims);
  const int32_t L = dims / 4;
  const int64_t nl = (int64_t)n * L;
  const dim3 grid_x((unsigned)((nl + kThreads - 1) / kThreads)), grid_n((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
  const int32_t nblk = (n + kStatRows - 1) / kStatRows;
  stag::PhiloxKey key{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u, nullptr};
  float *cur = w.x0, *nxt = w.x1;
  hipLaunchKernelGGL(reorder_init_kernel, grid_x, block, 0, s, cur, n, L, key);
  for (int32_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(reorder_smooth_kernel, grid_x, block, 0, s, cur, nxt, n, L, csr->indptr, csr->indices, csr_t->indptr,
                       csr_t->indices);
    hipLaunchKernelGGL(reorder_stats1_kernel, dim3((unsigned)nblk), block, 0, s, nxt, n, L, w.part);
    hipLaunchKernelGGL(reorder_stats2_kernel, dim3(1), dim3(64), 0, s, w.part, nblk, dims, n, w.stats);
    hipLaunchKernelGGL(reorder_normalise_kernel, grid_x, block, 0, s, nxt, n, L, w.stats);
    float* t = cur; cur = nxt; nxt = t;
  }
  hipLaunchKernelGGL(reorder_keys_kernel, grid_n, block, 0, s, cur, n, L, w.keys, w.ids);
  size_t tmp_bytes = w.tmp_bytes;
  if (rocprim::radix_sort_pairs(w.tmp, tmp_bytes, w.keys, w.keys_s, w.ids, perm, (size_t)n, 0u, (unsigned)dims, s) != hipSuccess)
    return STAG_EIO;
  hipLaunchKernelGGL(reorder_inverse_kernel, grid_n, block, 0, s, perm, n, inv);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_relabel_edges(const int32_t* src, const int32_t* dst, int64_t n_edges, const int32_t* inv, int32_t* src_out,
                                  int32_t* dst_out, void* stream) {
  if (n_edges < 0 || n_edges > 0x7FFFFFFFll) return STAG_EINVAL;
  if (n_edges == 0) return STAG_OK;
  if (!src || !dst || !inv || !src_out || !dst_out) return STAG_EINVAL;
  hipLaunchKernelGGL(relabel_edges_kernel, dim3((unsigned)((n_edges + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, src, dst, n_edges, inv, src_out, dst_out);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}
