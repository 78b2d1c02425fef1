// csr_build.hip — COO -> destination-major CSR on the device (graph preprocessing, not the hot
// path).  The order inside a row is ascending original edge id, exactly
// what the CPU oracle's counting sort produces, so the Philox positions agree.
//   1. stable LSD radix sort of (dst, edge id) pairs          rocPRIM radix_sort_pairs
//   2. indices[p] = src[eid[p]]                                gather kernel
//   3. in/out degree histograms (integer atomics), indptr = exclusive scan of in-degrees
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/stag_hip.h"
#include "share_order.hpp"

namespace {

__global__ void iota_kernel(int32_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (int32_t)i;
}

__global__ void zero_kernel(int32_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ void gather_hist_kernel(const int32_t* src, const int32_t* dst, const int32_t* eid, int64_t E,
                                   int32_t* indices, int32_t* in_deg, int32_t* out_deg) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= E) return;
  const int32_t e = eid[p];
  const int32_t u = src[e];
  indices[p] = u;
  atomicAdd(in_deg + dst[e], 1);
  if (out_deg) atomicAdd(out_deg + u, 1);
}

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

unsigned key_bits(int32_t n) {
  unsigned b = 1;
  while (b < 31 && (1u << b) < (unsigned)n) ++b;
  return b;
}

}  // namespace

extern "C" size_t stag_csr_build_workspace_bytes(int32_t n_dst, int64_t E) {
  if (E <= 0 || n_dst <= 0) return 256;
  size_t sort_tmp = 0, scan_tmp = 0;
  int32_t* null = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, null, null, null, null, (size_t)E, 0u, key_bits(n_dst));
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, null, null, 0, (size_t)n_dst + 1, rocprim::plus<int32_t>());
  return align_up((size_t)E * 4) * 2 + align_up(((size_t)n_dst + 1) * 4) + align_up(sort_tmp > scan_tmp ? sort_tmp : scan_tmp);
}

extern "C" int stag_csr_build(const int32_t* src, const int32_t* dst, int32_t n_src, int32_t n_dst,
                              int64_t E, int32_t* indptr, int32_t* indices, int32_t* eid,
                              int32_t* out_deg, void* workspace, size_t workspace_bytes, void* stream) {
  if (E < 0 || n_src < 0 || n_dst < 0 || !indptr || E > 0x7FFFFFFFll) return STAG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (n_dst == 0 && E > 0) return STAG_EINVAL;
  if (E == 0) {
    hipLaunchKernelGGL(zero_kernel, dim3((n_dst + 1 + 255) / 256), dim3(256), 0, s, indptr, (int64_t)n_dst + 1);
    if (out_deg && n_src > 0)
      hipLaunchKernelGGL(zero_kernel, dim3((n_src + 255) / 256), dim3(256), 0, s, out_deg, (int64_t)n_src);
    return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
  }
  if (!src || !dst || !indices || !eid || !workspace) return STAG_EINVAL;
  if (workspace_bytes < stag_csr_build_workspace_bytes(n_dst, E)) return STAG_ENOMEM;
  char* w = static_cast<char*>(workspace);
  int32_t* keys_out = reinterpret_cast<int32_t*>(w); w += align_up((size_t)E * 4);
  int32_t* iota = reinterpret_cast<int32_t*>(w);     w += align_up((size_t)E * 4);
  int32_t* deg = reinterpret_cast<int32_t*>(w);      w += align_up(((size_t)n_dst + 1) * 4);
  void* tmp = w;
  size_t tmp_bytes = workspace_bytes - (size_t)(w - static_cast<char*>(workspace));
  const unsigned eb = (unsigned)((E + 255) / 256);
  hipLaunchKernelGGL(iota_kernel, dim3(eb), dim3(256), 0, s, iota, E);
  hipLaunchKernelGGL(zero_kernel, dim3((n_dst + 1 + 255) / 256), dim3(256), 0, s, deg, (int64_t)n_dst + 1);
  if (out_deg)
    hipLaunchKernelGGL(zero_kernel, dim3((n_src + 255) / 256), dim3(256), 0, s, out_deg, (int64_t)n_src);
  if (rocprim::radix_sort_pairs(tmp, tmp_bytes, dst, keys_out, iota, eid, (size_t)E, 0u, key_bits(n_dst), s) != hipSuccess)
    return STAG_EIO;
  hipLaunchKernelGGL(gather_hist_kernel, dim3(eb), dim3(256), 0, s, src, dst, eid, E, indices, deg, out_deg);
  if (rocprim::exclusive_scan(tmp, tmp_bytes, deg, indptr, 0, (size_t)n_dst + 1, rocprim::plus<int32_t>(), s) != hipSuccess)
    return STAG_EIO;
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// ---- the launch plan on the device (stag_plan_device) -----------------------------------------------------
// The same plan stag_plan_count / stag_plan_fill build on the host, array for array: long rows (more than seg_len
// edges) first, most edges first, cut into balanced segments; then the whole rows, longest first; ties in row order.
// A minibatch graph is planned where it was built: no indptr read-back, no host loops, no uploads — one 16-byte
// read-back of the counts at the end.
//   1. key[r] = long ? (0x7FFFFFFF - deg) : (1 << 31) | (seg_len - deg);  stable radix sort of (key, row)
//   2. units per sorted row (segments | 1), exclusive scan -> first unit of every sorted row
//   3. fill: one thread per sorted row writes its unit records, long_rows, long_seg_ptr
namespace {

__global__ void plan_keys_kernel(const int32_t* indptr, int32_t n, int32_t seg_len, uint32_t* keys, int32_t* rows) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int32_t deg = indptr[r + 1] - indptr[r];
  keys[r] = deg > seg_len ? (0x7FFFFFFFu - (uint32_t)deg) : (0x80000000u | (uint32_t)(seg_len - deg));
  rows[r] = r;
}

// nu[i] = units of sorted row i; counts[0..2] += (long rows, segments, whole rows longer than STAG_HEAVY_LEN)
__global__ void plan_units_kernel(const int32_t* indptr, const int32_t* rows, int32_t n, int32_t seg_len,
                                  int32_t* nu, int32_t* counts) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int32_t is_long = 0, nseg = 0, heavy = 0;
  if (i < n) {
    const int32_t v = rows[i];
    const int32_t deg = indptr[v + 1] - indptr[v];
    if (deg > seg_len) { is_long = 1; nseg = (deg + seg_len - 1) / seg_len; nu[i] = nseg; }
    else { nu[i] = 1; heavy = deg > STAG_HEAVY_LEN ? 1 : 0; }
  }
  // integer sums: any order gives the same counts
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    is_long += __shfl_xor(is_long, d); nseg += __shfl_xor(nseg, d); heavy += __shfl_xor(heavy, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (is_long) atomicAdd(counts + 0, is_long);
    if (nseg) atomicAdd(counts + 1, nseg);
    if (heavy) atomicAdd(counts + 2, heavy);
  }
}

__global__ void plan_fill_kernel(const int32_t* indptr, const int32_t* rows, const int32_t* uoff, int32_t n,
                                 int32_t seg_len, stag_unit* units, int32_t* long_rows, int32_t* long_seg_ptr,
                                 const int32_t* counts) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) long_seg_ptr[counts[0]] = counts[1];
  if (i >= n) return;
  const int32_t v = rows[i];
  const int32_t b = indptr[v], deg = indptr[v + 1] - b;
  const int32_t u0 = uoff[i];
  if (deg > seg_len) {                       // sorted position = index among the long rows (they come first)
    const int32_t nseg = (deg + seg_len - 1) / seg_len;
    const int32_t base = deg / nseg, rem = deg % nseg;      // balanced: lengths differ by at most 1
    long_rows[i] = v;
    long_seg_ptr[i] = u0;
    int32_t p = b;
    for (int32_t k = 0; k < nseg; ++k) {
      const int32_t l = base + (k < rem ? 1 : 0);
      units[u0 + k] = stag_unit{i, p, l, u0 + k};
      p += l;
    }
  } else {
    units[u0] = stag_unit{v, b, deg, -1};
  }
}

}  // namespace

extern "C" size_t stag_plan_device_workspace_bytes(int32_t n_dst) {
  if (n_dst <= 0) return 256;
  size_t sort_tmp = 0, scan_tmp = 0;
  uint32_t* ku = nullptr;
  int32_t* null = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, ku, ku, null, null, (size_t)n_dst, 0u, 32u);
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, null, null, 0, (size_t)n_dst, rocprim::plus<int32_t>());
  // keys in/out, rows in/out, units per row, unit offsets, 4 counters, rocPRIM's temporary storage
  return align_up((size_t)n_dst * 4) * 6 + 256 + align_up(sort_tmp > scan_tmp ? sort_tmp : scan_tmp);
}

extern "C" int stag_plan_device(const int32_t* indptr, int32_t n_dst, int64_t n_edges, int32_t seg_len,
                                stag_unit* units, int64_t units_capacity, int32_t* long_rows, int32_t* long_seg_ptr,
                                int64_t long_capacity, int32_t* counts_out_host, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!indptr || n_dst < 0 || n_edges < 0 || seg_len <= 0 || seg_len > (1 << 20) || !counts_out_host) return STAG_EINVAL;
  counts_out_host[0] = counts_out_host[1] = counts_out_host[2] = counts_out_host[3] = 0;
  if (n_dst == 0) return STAG_OK;
  // upper bounds the caller sized the arrays with: a long row has more than seg_len edges
  const int64_t max_long = n_edges / ((int64_t)seg_len + 1);
  const int64_t max_units = (int64_t)n_dst + n_edges / seg_len + 1;
  if (!units || !long_rows || !long_seg_ptr || units_capacity < max_units || long_capacity < max_long + 1) return STAG_EINVAL;
  if (!workspace || workspace_bytes < stag_plan_device_workspace_bytes(n_dst)) return STAG_ENOMEM;
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  const size_t slot = align_up((size_t)n_dst * 4);
  uint32_t* keys = reinterpret_cast<uint32_t*>(w);
  uint32_t* keys_s = reinterpret_cast<uint32_t*>(w + slot);
  int32_t* rows = reinterpret_cast<int32_t*>(w + 2 * slot);
  int32_t* rows_s = reinterpret_cast<int32_t*>(w + 3 * slot);
  int32_t* nu = reinterpret_cast<int32_t*>(w + 4 * slot);
  int32_t* uoff = reinterpret_cast<int32_t*>(w + 5 * slot);
  int32_t* counts = reinterpret_cast<int32_t*>(w + 6 * slot);
  void* tmp = w + 6 * slot + 256;
  size_t tmp_bytes = workspace_bytes - (6 * slot + 256);
  const dim3 grid((n_dst + 255) / 256), block(256);
  if (hipMemsetAsync(counts, 0, 16, s) != hipSuccess) return STAG_EIO;
  hipLaunchKernelGGL(plan_keys_kernel, grid, block, 0, s, indptr, n_dst, seg_len, keys, rows);
  if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_s, rows, rows_s, (size_t)n_dst, 0u, 32u, s) != hipSuccess)
    return STAG_EIO;
  hipLaunchKernelGGL(plan_units_kernel, grid, block, 0, s, indptr, rows_s, n_dst, seg_len, nu, counts);
  if (rocprim::exclusive_scan(tmp, tmp_bytes, nu, uoff, 0, (size_t)n_dst, rocprim::plus<int32_t>(), s) != hipSuccess)
    return STAG_EIO;
  hipLaunchKernelGGL(plan_fill_kernel, grid, block, 0, s, indptr, rows_s, uoff, n_dst, seg_len, units, long_rows,
                     long_seg_ptr, counts);
  int32_t c[4] = {0, 0, 0, 0};
  if (hipMemcpyAsync(c, counts, 16, hipMemcpyDeviceToHost, s) != hipSuccess) return STAG_EIO;
  if (hipStreamSynchronize(s) != hipSuccess) return STAG_EIO;
  const int64_t n_long = c[0], n_seg = c[1], n_heavy = (int64_t)c[1] + c[2];
  const int64_t n_units = (int64_t)n_dst - n_long + n_seg;
  if (n_units > 0x7FFFFFFFll) return STAG_EINVAL;
  counts_out_host[0] = (int32_t)n_units; counts_out_host[1] = (int32_t)n_long;
  counts_out_host[2] = (int32_t)n_seg; counts_out_host[3] = (int32_t)(n_heavy > 0x7FFFFFFFll ? 0x7FFFFFFFll : n_heavy);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// ---- the XCD-aware order of a plan's units on the device (stag_plan_xcd_device_count / _fill) ---------------
// stag_plan_xcd's stable partition as a stable radix sort of (fine stripe key, unit index); the stripe starts by
// lower-bound search; then every record goes to (its XCD stripe's base) + (its rank inside that stripe) — the fine
// stripes of one XCD stripe are neighbours in the sorted order.
namespace {

constexpr int kXcdMaxKeys = 2 * STAG_XCD_STRIPES * STAG_XCD_FINE_MAX;      // 256

__global__ void xcd_keys_kernel(const stag_unit* units, int32_t n_units, int32_t n_heavy, int64_t E, int32_t S,
                                uint32_t* keys, int32_t* idx) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units) return;
  int64_t k = (int64_t)units[i].start * S / E;
  k = k < 0 ? 0 : k >= S ? S - 1 : k;
  keys[i] = (uint32_t)((i >= n_heavy ? S : 0) + (int)k);
  idx[i] = i;
}

// the same with a range table (stag_plan_xcd_device_count_ranges): key of the range the unit's first edge lies in
__global__ void xcd_keys_ranges_kernel(const stag_unit* units, int32_t n_units, int32_t n_heavy, const int64_t* cuts,
                                       const int32_t* rkeys, int32_t R, int32_t S, uint32_t* keys, int32_t* idx) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units) return;
  const int64_t start = units[i].start;
  int32_t lo = 0, hi = R;
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (cuts[mid] <= start) lo = mid; else hi = mid;
  }
  int k = rkeys[lo];
  k = k < 0 ? 0 : k >= S ? S - 1 : k;
  keys[i] = (uint32_t)((i >= n_heavy ? S : 0) + k);
  idx[i] = i;
}

// starts[k] = first sorted position with key >= k, k in [0, 2 S]
__global__ void xcd_starts_kernel(const uint32_t* keys_s, int32_t n_units, int32_t S, int32_t* starts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > 2 * S) return;
  int32_t lo = 0, hi = n_units;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (keys_s[mid] < (uint32_t)t) lo = mid + 1; else hi = mid;
  }
  starts[t] = lo;
}

__global__ void xcd_clear_kernel(int32_t* xcd, int64_t n_rec, const int32_t* starts, int32_t fine, int32_t sh, int32_t sl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < STAG_XCD_HEADER) {
    int32_t v = 0;
    if (i < 2 * STAG_XCD_STRIPES) v = starts[(i + 1) * fine] - starts[i * fine];
    else if (i == 2 * STAG_XCD_STRIPES) v = sh;
    else if (i == 2 * STAG_XCD_STRIPES + 1) v = sl;
    else if (i == 2 * STAG_XCD_STRIPES + 2) v = fine;
    xcd[i] = v;
  }
  if (i < n_rec) reinterpret_cast<int4*>(xcd + STAG_XCD_HEADER)[i] = make_int4(-1, 0, 0, -1);
}

__global__ void xcd_fill_kernel(const stag_unit* units, const uint32_t* keys_s, const int32_t* idx_s, int32_t n_units,
                                const int32_t* starts, int32_t fine, int32_t sh, int32_t sl, int32_t* xcd) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units) return;
  const int x = (int)keys_s[i] / fine;               // XCD stripe: heavy [0, 8), the others [8, 16)
  const int64_t base = x < STAG_XCD_STRIPES ? (int64_t)x * sh
                                            : (int64_t)STAG_XCD_STRIPES * sh + (int64_t)(x - STAG_XCD_STRIPES) * sl;
  reinterpret_cast<int4*>(xcd + STAG_XCD_HEADER)[base + (i - starts[x * fine])] = reinterpret_cast<const int4*>(units)[idx_s[i]];
}

struct XcdWs {
  uint32_t *keys, *keys_s;
  int32_t *idx, *idx_s, *starts;
  void* tmp;
  size_t tmp_bytes;
};
constexpr size_t kXcdStartsBytes = 2048;     // >= (kXcdMaxKeys + 1) ints
XcdWs xcd_ws(void* workspace, size_t workspace_bytes, int32_t n_units) {
  char* w = static_cast<char*>(workspace);
  const size_t slot = align_up((size_t)(n_units > 0 ? n_units : 1) * 4);
  XcdWs x;
  x.keys_s = reinterpret_cast<uint32_t*>(w);                 // what _fill reads comes first
  x.idx_s = reinterpret_cast<int32_t*>(w + slot);
  x.starts = reinterpret_cast<int32_t*>(w + 2 * slot);
  x.keys = reinterpret_cast<uint32_t*>(w + 2 * slot + kXcdStartsBytes);
  x.idx = reinterpret_cast<int32_t*>(w + 3 * slot + kXcdStartsBytes);
  x.tmp = w + 4 * slot + kXcdStartsBytes;
  x.tmp_bytes = workspace_bytes - (4 * slot + kXcdStartsBytes);
  return x;
}

}  // namespace

extern "C" size_t stag_plan_xcd_device_workspace_bytes(int32_t n_units) {
  if (n_units <= 0) n_units = 1;
  size_t sort_tmp = 0;
  uint32_t* ku = nullptr;
  int32_t* null = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, ku, ku, null, null, (size_t)n_units, 0u, 9u);
  return align_up((size_t)n_units * 4) * 4 + kXcdStartsBytes + align_up(sort_tmp);
}

static int xcd_device_count_impl(const stag_unit* units, int32_t n_units, int32_t n_heavy, int64_t n_edges,
                                 const int64_t* cuts, const int32_t* rkeys, int32_t n_ranges,
                                 int32_t fine, int32_t* strides_out_host, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (n_units < 0 || n_heavy < 0 || n_heavy > n_units || n_edges < 0 || !strides_out_host || fine < 1 ||
      fine > STAG_XCD_FINE_MAX || (n_units > 0 && !units) || ((uintptr_t)units & 15)) return STAG_EINVAL;
  if (!workspace || workspace_bytes < stag_plan_xcd_device_workspace_bytes(n_units)) return STAG_ENOMEM;
  strides_out_host[0] = strides_out_host[1] = 0;
  if (n_units == 0) return STAG_OK;
  hipStream_t s = (hipStream_t)stream;
  const XcdWs x = xcd_ws(workspace, workspace_bytes, n_units);
  const int S = STAG_XCD_STRIPES * fine;
  unsigned bits = 1;
  while ((1u << bits) < (unsigned)(2 * S)) ++bits;
  const dim3 grid((unsigned)((n_units + 255) / 256)), block(256);
  if (cuts)
    hipLaunchKernelGGL(xcd_keys_ranges_kernel, grid, block, 0, s, units, n_units, n_heavy, cuts, rkeys, n_ranges, S, x.keys, x.idx);
  else
    hipLaunchKernelGGL(xcd_keys_kernel, grid, block, 0, s, units, n_units, n_heavy, n_edges > 0 ? n_edges : (int64_t)1, S,
                       x.keys, x.idx);
  size_t tmp_bytes = x.tmp_bytes;
  if (rocprim::radix_sort_pairs(x.tmp, tmp_bytes, x.keys, x.keys_s, x.idx, x.idx_s, (size_t)n_units, 0u, bits, s) != hipSuccess)
    return STAG_EIO;
  hipLaunchKernelGGL(xcd_starts_kernel, dim3((2 * S + 1 + 63) / 64), dim3(64), 0, s, x.keys_s, n_units, S, x.starts);
  int32_t h[kXcdMaxKeys + 1];
  if (hipMemcpyAsync(h, x.starts, sizeof(int32_t) * (2 * S + 1), hipMemcpyDeviceToHost, s) != hipSuccess) return STAG_EIO;
  if (hipStreamSynchronize(s) != hipSuccess) return STAG_EIO;
  for (int k = 0; k < STAG_XCD_STRIPES; ++k) {
    strides_out_host[0] = std::max(strides_out_host[0], h[(k + 1) * fine] - h[k * fine]);
    strides_out_host[1] = std::max(strides_out_host[1], h[S + (k + 1) * fine] - h[S + k * fine]);
  }
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_plan_xcd_device_count(const stag_unit* units, int32_t n_units, int32_t n_heavy, int64_t n_edges,
                                          int32_t fine, int32_t* strides_out_host, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return xcd_device_count_impl(units, n_units, n_heavy, n_edges, nullptr, nullptr, 0, fine, strides_out_host, workspace,
                               workspace_bytes, stream);
}

extern "C" int stag_plan_xcd_device_count_ranges(const stag_unit* units, int32_t n_units, int32_t n_heavy,
                                                 const int64_t* cuts, const int32_t* keys, int32_t n_ranges, int32_t fine,
                                                 int32_t* strides_out_host, void* workspace, size_t workspace_bytes,
                                                 void* stream) {
  if (n_ranges < 1 || !cuts || !keys) return STAG_EINVAL;
  return xcd_device_count_impl(units, n_units, n_heavy, 0, cuts, keys, n_ranges, fine, strides_out_host, workspace,
                               workspace_bytes, stream);
}

extern "C" int stag_plan_xcd_device_fill(const stag_unit* units, int32_t n_units, const int32_t* strides, int32_t fine,
                                         int32_t* xcd, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_units <= 0 || !units || !strides || !xcd || ((uintptr_t)xcd & 15) || ((uintptr_t)units & 15) ||
      strides[0] < 0 || strides[1] < 0 || fine < 1 || fine > STAG_XCD_FINE_MAX) return STAG_EINVAL;
  if (!workspace || workspace_bytes < stag_plan_xcd_device_workspace_bytes(n_units)) return STAG_ENOMEM;
  hipStream_t s = (hipStream_t)stream;
  const XcdWs x = xcd_ws(workspace, workspace_bytes, n_units);
  const int64_t n_rec = (int64_t)STAG_XCD_STRIPES * ((int64_t)strides[0] + strides[1]);
  if (n_rec < n_units || n_rec > 0x7FFFFFFFll) return STAG_EINVAL;
  const int64_t n_clear = n_rec > STAG_XCD_HEADER ? n_rec : STAG_XCD_HEADER;
  hipLaunchKernelGGL(xcd_clear_kernel, dim3((unsigned)((n_clear + 255) / 256)), dim3(256), 0, s, xcd, n_rec, x.starts, fine,
                     strides[0], strides[1]);
  hipLaunchKernelGGL(xcd_fill_kernel, dim3((unsigned)((n_units + 255) / 256)), dim3(256), 0, s, units, x.keys_s, x.idx_s,
                     n_units, x.starts, fine, strides[0], strides[1], xcd);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// ---- stripe locality of a square CSR (what "auto" decides the XCD-aware order by) ---------------------------
// edges whose source row starts in the same eighth of the CSR as the edge itself lies in: integer count, any order
namespace {
__global__ void stripe_locality_kernel(const int32_t* indptr, const int32_t* indices, int32_t n_dst, int64_t E,
                                       unsigned long long* same) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int hit = 0;
  if (p < E) {
    const int32_t u = indices[p];
    if (u >= 0 && u < n_dst) {
      int64_t ks = (int64_t)indptr[u] * STAG_XCD_STRIPES / E;
      ks = ks >= STAG_XCD_STRIPES ? STAG_XCD_STRIPES - 1 : ks;
      hit = (p * STAG_XCD_STRIPES / E) == ks;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) hit += __shfl_xor(hit, d);
  if ((threadIdx.x & 63) == 0 && hit) atomicAdd(same, (unsigned long long)hit);
}
}  // namespace

extern "C" int stag_stripe_locality(const int32_t* indptr, const int32_t* indices, int32_t n_dst, int64_t n_edges,
                                    int64_t* same_out_host, void* workspace, void* stream) {
  if (!same_out_host || n_dst < 0 || n_edges < 0 || !workspace) return STAG_EINVAL;
  *same_out_host = 0;
  if (n_edges == 0 || n_dst == 0) return STAG_OK;
  if (!indptr || !indices) return STAG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* same = static_cast<unsigned long long*>(workspace);
  if (hipMemsetAsync(same, 0, 8, s) != hipSuccess) return STAG_EIO;
  hipLaunchKernelGGL(stripe_locality_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, s, indptr, indices, n_dst,
                     n_edges, same);
  unsigned long long h = 0;
  if (hipMemcpyAsync(&h, same, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return STAG_EIO;
  if (hipStreamSynchronize(s) != hipSuccess) return STAG_EIO;
  *same_out_host = (int64_t)h;
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// ---- laying int32 arrays end to end with offsets (stag_concat_jobs) -------------------------------------------
// A block-diagonal batch's CSR views are its parts' arrays one after the other, shifted by the nodes / edges before the
// part.  ONE launch copies every piece of every array: a table of jobs on the device, a block per 1024 elements of a job.
namespace {
__global__ void concat_jobs_kernel(const stag_concat_job* jobs, const int64_t* chunk_start, int32_t n_jobs) {
  // the job of this block: chunk_start[j] <= blockIdx.x < chunk_start[j + 1]   (block-uniform binary search)
  int lo = 0, hi = n_jobs;
  const int64_t b = blockIdx.x;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= b) lo = mid; else hi = mid;
  }
  const stag_concat_job j = jobs[lo];
  const int64_t first = (b - chunk_start[lo]) * 1024;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = first + k * 256 + threadIdx.x;
    if (i >= j.count) return;
    j.dst[i] = (j.kind == STAG_CONCAT_FILL ? 0 : j.src[i]) + j.add;
  }
}
}  // namespace

extern "C" int stag_concat_jobs(const stag_concat_job* jobs, const int64_t* chunk_start, int32_t n_jobs, int64_t n_chunks,
                                void* stream) {
  if (n_jobs < 0 || n_chunks < 0 || n_chunks > 0x7FFFFFFFll) return STAG_EINVAL;
  if (n_jobs == 0 || n_chunks == 0) return STAG_OK;
  if (!jobs || !chunk_start) return STAG_EINVAL;
  hipLaunchKernelGGL(concat_jobs_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, jobs, chunk_start, n_jobs);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// ---- the share order of a plan's units (stag_plan_share / stag_plan_share_device) ---------------------------------
// Whole-row units that gather the same source row are put side by side — pairs at 2k, quads at 4k, octets at 8k of the
// absolute unit index — inside their class of equal trip count (len + 1) / 2, so that the teams of one workgroup ask
// for a shared row within the same few microseconds and the second request finds it in the L2.  Segments stay put.
//   per level (1 -> 2 -> 4 -> 8): the (source, cluster) pair of every edge of every cluster that is complete at this
//   size, sorted; a cluster's id is its smallest unit index, so inside a run of one source the clusters of one class are
//   neighbours.  Device: every cluster takes, of its neighbours in such runs, the one with the smallest hash (atomicMin
//   of (hash, partner): a pure function of the graph); mutual choices merge; kShareRounds rounds.  Host: the sequential
//   greedy — clusters in id order, each takes the first free cluster that shares one of its sources.
//   Then one sort of the unit keys (share_order.hpp) ranks every class, and share_layout / share_position place it.
namespace {

constexpr int kShareRounds = 4;
constexpr int kShareScan = 16;      // entries of a run a cluster looks ahead for a free neighbour

__global__ void share_init_kernel(int32_t n_seg, int32_t n_units, int32_t* cid, int32_t* lvl, int32_t* off) {
  const int32_t i = n_seg + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units) return;
  cid[i] = i; lvl[i] = 0; off[i] = 0;
}

// keys[p] = (source, cluster) for the edges of the clusters complete at `level`; every other position keeps ~0
__global__ void share_edge_keys_kernel(const stag_unit* units, int32_t n_seg, int32_t n_units, const int32_t* indices,
                                       int64_t E, const int32_t* cid, const int32_t* lvl, int32_t level, uint64_t* keys) {
  const int32_t i = n_seg + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units || lvl[i] != level) return;
  const stag_unit u = units[i];
  const uint64_t c = (uint32_t)cid[i];
  for (int32_t e = 0; e < u.len; ++e) {
    const int64_t p = (int64_t)u.start + e;
    if (p < 0 || p >= E) break;
    keys[p] = ((uint64_t)(uint32_t)indices[p] << 32) | c;
  }
}

__global__ void share_candidates_kernel(const stag_unit* units, const uint64_t* keys_s, int64_t E, const int32_t* mate,
                                        uint32_t salt, unsigned long long* best) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= E) return;
  const uint64_t k = keys_s[j];
  if (k == ~0ull) return;
  const uint32_t A = (uint32_t)k, src = (uint32_t)(k >> 32);
  if (mate[A] >= 0) return;
  const int32_t trips = share_trips(units[A].len);
  for (int64_t t = j + 1; t < E && t <= j + kShareScan; ++t) {
    const uint64_t kt = keys_s[t];
    if (kt == ~0ull || (uint32_t)(kt >> 32) != src) return;
    const uint32_t B = (uint32_t)kt;
    if (B == A) continue;
    if (share_trips(units[B].len) != trips) return;       // ids ascend with the class: the run's later clusters differ too
    if (mate[B] >= 0) continue;
    const unsigned long long h = (unsigned long long)share_hash(A, B, salt) << 32;
    atomicMin(best + A, h | B);
    atomicMin(best + B, h | A);
    return;
  }
}

__global__ void share_mutual_kernel(int32_t n_seg, int32_t n_units, const int32_t* cid, const int32_t* lvl, int32_t level,
                                    const unsigned long long* best, int32_t* mate) {
  const int32_t A = n_seg + blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= n_units || lvl[A] != level || cid[A] != A) return;
  const unsigned long long b = best[A];
  if (b == ~0ull) return;
  const int32_t B = (int32_t)(uint32_t)b;
  // (only the smaller id of a mutual pair writes, and a cluster's choice names one partner: no two threads write one slot)
  if (A < B && B < n_units && (uint32_t)best[B] == (uint32_t)A) { mate[A] = B; mate[B] = A; }
}

__global__ void share_merge_kernel(int32_t n_seg, int32_t n_units, const int32_t* mate, int32_t level, int32_t* cid,
                                   int32_t* lvl, int32_t* off) {
  const int32_t i = n_seg + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_units || lvl[i] != level) return;
  const int32_t c = cid[i], m = mate[c];
  if (m < 0) return;
  if (m < c) { cid[i] = m; off[i] += 1 << level; }
  lvl[i] = level + 1;
}

__global__ void share_unit_keys_kernel(const stag_unit* units, int32_t n_seg, int32_t n_units, int32_t seg_len,
                                       const int32_t* cid, const int32_t* lvl, const int32_t* off, uint64_t* keys, int32_t* idx) {
  const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t i = n_seg + j;
  if (i >= n_units) return;
  keys[j] = share_unit_key(share_class(units[i].len, seg_len), lvl[i], cid[i], off[i]);
  idx[j] = i;
}

// table[c] = the layout of class index c, from the sorted unit keys (5 lower bounds)
__global__ void share_table_kernel(const uint64_t* keys_s, int32_t n_w, int32_t n_seg, int32_t n_classes, ShareLayout* table) {
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_classes) return;
  int32_t at[5];
  for (int q = 0; q < 5; ++q) {
    const uint64_t want = ((uint64_t)(uint32_t)c << kShareClassShift) + ((uint64_t)q << kShareSizeShift);
    int32_t lo = 0, hi = n_w;
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (keys_s[mid] < want) lo = mid + 1; else hi = mid;
    }
    at[q] = lo;
  }
  table[c] = share_layout(n_seg + at[0], n_seg + at[4], (at[1] - at[0]) / 8, (at[2] - at[1]) / 4, (at[3] - at[2]) / 2,
                          at[4] - at[3]);
}

__global__ void share_place_kernel(const stag_unit* units, const uint64_t* keys_s, const int32_t* idx_s, int32_t n_seg,
                                   int32_t n_units, const ShareLayout* table, stag_unit* out) {
  const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_units) return;
  if (j < n_seg) { reinterpret_cast<int4*>(out)[j] = reinterpret_cast<const int4*>(units)[j]; return; }
  const int32_t s = j - n_seg;
  const ShareLayout L = table[(int32_t)(keys_s[s] >> kShareClassShift)];
  int32_t pos = share_position(L, j - L.a);
  if (pos < n_seg || pos >= n_units) pos = j;             // (cannot happen: share_layout fills [a, b) exactly)
  reinterpret_cast<int4*>(out)[pos] = reinterpret_cast<const int4*>(units)[idx_s[s]];
}

struct ShareWs {
  uint64_t *keys, *keys_s;
  unsigned long long* best;
  int32_t *cid, *lvl, *off, *mate, *idx, *idx_s;
  ShareLayout* table;
  void* tmp;
  size_t tmp_bytes, total;
};

int32_t share_classes(int32_t seg_len) { return share_trips(seg_len) + 1; }

ShareWs share_ws(void* workspace, int32_t n_units, int64_t n_edges, int32_t seg_len) {
  char* w = static_cast<char*>(workspace);
  const size_t nu = (size_t)(n_units > 0 ? n_units : 1);
  const size_t m = std::max(nu, (size_t)(n_edges > 0 ? n_edges : 1));
  size_t sort_keys = 0, sort_pairs = 0;
  uint64_t* k64 = nullptr;
  int32_t* null = nullptr;
  (void)rocprim::radix_sort_keys(nullptr, sort_keys, k64, k64, m, 0u, 64u);
  (void)rocprim::radix_sort_pairs(nullptr, sort_pairs, k64, k64, null, null, nu, 0u, (unsigned)kShareKeyBits);
  ShareWs x;
  size_t at = 0;
  auto take = [&](size_t bytes) { char* p = w ? w + at : nullptr; at += align_up(bytes); return p; };
  x.keys = reinterpret_cast<uint64_t*>(take(m * 8));
  x.keys_s = reinterpret_cast<uint64_t*>(take(m * 8));
  x.best = reinterpret_cast<unsigned long long*>(take(nu * 8));
  x.cid = reinterpret_cast<int32_t*>(take(nu * 4));
  x.lvl = reinterpret_cast<int32_t*>(take(nu * 4));
  x.off = reinterpret_cast<int32_t*>(take(nu * 4));
  x.mate = reinterpret_cast<int32_t*>(take(nu * 4));
  x.idx = reinterpret_cast<int32_t*>(take(nu * 4));
  x.idx_s = reinterpret_cast<int32_t*>(take(nu * 4));
  x.table = reinterpret_cast<ShareLayout*>(take((size_t)share_classes(seg_len) * sizeof(ShareLayout)));
  x.tmp_bytes = align_up(std::max(sort_keys, sort_pairs));
  x.tmp = take(x.tmp_bytes);
  x.total = at;
  return x;
}

bool share_args_ok(const void* units, int32_t n_units, int32_t n_seg, int32_t n_heavy, int32_t seg_len, const void* indices,
                   int64_t n_edges, const void* out) {
  return n_units >= 0 && n_seg >= 0 && n_seg <= n_heavy && n_heavy <= n_units && seg_len > 0 && seg_len <= (1 << 20) &&
         n_edges >= 0 && (n_units == 0 || (units && out && units != out)) && (n_edges == 0 || indices);
}

}  // namespace

extern "C" size_t stag_plan_share_device_workspace_bytes(int32_t n_units, int64_t n_edges, int32_t seg_len) {
  if (seg_len <= 0 || seg_len > (1 << 20)) seg_len = 1;
  return share_ws(nullptr, n_units, n_edges, seg_len).total;
}

extern "C" int stag_plan_share_device(const stag_unit* units, int32_t n_units, int32_t n_seg, int32_t n_heavy, int32_t seg_len,
                                      const int32_t* indices, int64_t n_edges, stag_unit* units_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!share_args_ok(units, n_units, n_seg, n_heavy, seg_len, indices, n_edges, units_out) || ((uintptr_t)units & 15) ||
      ((uintptr_t)units_out & 15)) return STAG_EINVAL;
  if (n_units == 0) return STAG_OK;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < stag_plan_share_device_workspace_bytes(n_units, n_edges, seg_len))
    return STAG_ENOMEM;
  hipStream_t s = (hipStream_t)stream;
  const ShareWs x = share_ws(workspace, n_units, n_edges, seg_len);
  const int32_t n_w = n_units - n_seg;
  const dim3 block(256), grid_u((unsigned)((n_units + 255) / 256)), grid_w((unsigned)((n_w + 255) / 256));
  if (n_w > 0 && n_edges > 0) {
    const dim3 grid_e((unsigned)((n_edges + 255) / 256));
    hipLaunchKernelGGL(share_init_kernel, grid_w, block, 0, s, n_seg, n_units, x.cid, x.lvl, x.off);
    for (int level = 0; level < kShareLevels; ++level) {
      if (hipMemsetAsync(x.keys, 0xFF, (size_t)n_edges * 8, s) != hipSuccess) return STAG_EIO;
      if (hipMemsetAsync(x.mate, 0xFF, (size_t)n_units * 4, s) != hipSuccess) return STAG_EIO;
      hipLaunchKernelGGL(share_edge_keys_kernel, grid_w, block, 0, s, units, n_seg, n_units, indices, n_edges, x.cid, x.lvl,
                         level, x.keys);
      size_t tmp_bytes = x.tmp_bytes;
      if (rocprim::radix_sort_keys(x.tmp, tmp_bytes, x.keys, x.keys_s, (size_t)n_edges, 0u, 64u, s) != hipSuccess) return STAG_EIO;
      for (int round = 0; round < kShareRounds; ++round) {
        if (hipMemsetAsync(x.best, 0xFF, (size_t)n_units * 8, s) != hipSuccess) return STAG_EIO;
        hipLaunchKernelGGL(share_candidates_kernel, grid_e, block, 0, s, units, x.keys_s, n_edges, x.mate,
                           (uint32_t)(level * kShareRounds + round), x.best);
        hipLaunchKernelGGL(share_mutual_kernel, grid_w, block, 0, s, n_seg, n_units, x.cid, x.lvl, level, x.best, x.mate);
      }
      hipLaunchKernelGGL(share_merge_kernel, grid_w, block, 0, s, n_seg, n_units, x.mate, level, x.cid, x.lvl, x.off);
    }
  } else if (n_w > 0) {
    hipLaunchKernelGGL(share_init_kernel, grid_w, block, 0, s, n_seg, n_units, x.cid, x.lvl, x.off);
  }
  if (n_w > 0) {
    hipLaunchKernelGGL(share_unit_keys_kernel, grid_w, block, 0, s, units, n_seg, n_units, seg_len, x.cid, x.lvl, x.off,
                       x.keys, x.idx);
    size_t tmp_bytes = x.tmp_bytes;
    if (rocprim::radix_sort_pairs(x.tmp, tmp_bytes, x.keys, x.keys_s, x.idx, x.idx_s, (size_t)n_w, 0u, (unsigned)kShareKeyBits,
                                  s) != hipSuccess) return STAG_EIO;
    const int32_t n_classes = share_classes(seg_len);
    hipLaunchKernelGGL(share_table_kernel, dim3((unsigned)((n_classes + 255) / 256)), block, 0, s, x.keys_s, n_w, n_seg,
                       n_classes, x.table);
  }
  hipLaunchKernelGGL(share_place_kernel, grid_u, block, 0, s, units, x.keys_s, x.idx_s, n_seg, n_units, x.table, units_out);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

// The host twin: the sequential greedy, the same layout.
extern "C" int stag_plan_share(const stag_unit* units_host, int32_t n_units, int32_t n_seg, int32_t n_heavy, int32_t seg_len,
                               const int32_t* indices_host, int64_t n_edges, stag_unit* units_out_host) {
  if (!share_args_ok(units_host, n_units, n_seg, n_heavy, seg_len, indices_host, n_edges, units_out_host)) return STAG_EINVAL;
  try {
    const stag_unit* U = units_host;
    std::vector<int32_t> cid(n_units), lvl(n_units, 0), off(n_units, 0), next(n_units, -1), mate(n_units);
    for (int32_t i = 0; i < n_units; ++i) cid[i] = i;
    struct Entry { int32_t trips_desc, src, c; };
    std::vector<Entry> run;
    std::vector<size_t> cursor;
    for (int level = 0; level < kShareLevels; ++level) {
      // (class, source, cluster) of every edge of the clusters complete at this size; next[] chains a cluster's units
      run.clear();
      for (int32_t i = n_seg; i < n_units; ++i) {
        if (lvl[i] != level) continue;
        for (int32_t e = 0; e < U[i].len; ++e) {
          const int64_t p = (int64_t)U[i].start + e;
          if (p < 0 || p >= n_edges) break;
          run.push_back(Entry{-share_trips(U[i].len), indices_host[p], cid[i]});
        }
      }
      auto less = [](const Entry& x, const Entry& y) {
        return x.trips_desc != y.trips_desc ? x.trips_desc < y.trips_desc : x.src != y.src ? x.src < y.src : x.c < y.c;
      };
      std::sort(run.begin(), run.end(), less);
      cursor.assign(run.size(), 0);
      for (size_t k = 0; k < run.size(); ++k) cursor[k] = k;
      std::fill(mate.begin(), mate.end(), -1);
      for (int32_t A = n_seg; A < n_units; ++A) {
        if (lvl[A] != level || cid[A] != A || mate[A] >= 0) continue;
        int32_t found = -1;
        for (int32_t m = A; m >= 0 && found < 0; m = next[m]) {               // the cluster's units, in member order
          for (int32_t e = 0; e < U[m].len && found < 0; ++e) {
            const int64_t p = (int64_t)U[m].start + e;
            if (p < 0 || p >= n_edges) break;
            const Entry want{-share_trips(U[A].len), indices_host[p], 0};
            const size_t first = std::lower_bound(run.begin(), run.end(), want, less) - run.begin();
            if (first >= run.size()) continue;
            auto in_run = [&](size_t k) {
              return k < run.size() && run[k].trips_desc == want.trips_desc && run[k].src == want.src;
            };
            size_t k = cursor[first];                     // (the taken clusters at the run's head are passed over once)
            while (in_run(k) && mate[run[k].c] >= 0) ++k;
            cursor[first] = k;
            for (; in_run(k); ++k)
              if (run[k].c != A && mate[run[k].c] < 0) { found = run[k].c; break; }
          }
        }
        if (found >= 0) { mate[A] = found; mate[found] = A; }
      }
      for (int32_t A = n_seg; A < n_units; ++A) {       // A < mate[A]: the clusters were visited in id order
        if (lvl[A] != level || cid[A] != A || mate[A] < A) continue;
        int32_t tail = A;
        while (next[tail] >= 0) tail = next[tail];
        next[tail] = mate[A];
      }
      for (int32_t i = n_seg; i < n_units; ++i) {
        if (lvl[i] != level) continue;
        const int32_t c = cid[i], m = mate[c];
        if (m < 0) continue;
        if (m < c) { cid[i] = m; off[i] += 1 << level; }
        lvl[i] = level + 1;
      }
    }
    const int32_t n_w = n_units - n_seg;
    std::vector<std::pair<uint64_t, int32_t>> keyed(n_w);
    for (int32_t j = 0; j < n_w; ++j) {
      const int32_t i = n_seg + j;
      keyed[j] = {share_unit_key(share_class(U[i].len, seg_len), lvl[i], cid[i], off[i]), i};
    }
    std::sort(keyed.begin(), keyed.end());
    std::copy(U, U + n_seg, units_out_host);
    for (int32_t j = 0; j < n_w;) {
      const uint64_t cls = keyed[j].first >> kShareClassShift;
      int32_t at[5] = {j, j, j, j, j}, e = j;
      for (; e < n_w && (keyed[e].first >> kShareClassShift) == cls; ++e)
        for (int q = (int)((keyed[e].first >> kShareSizeShift) & 3) + 1; q < 5; ++q) at[q] = e + 1;
      const ShareLayout L = share_layout(n_seg + j, n_seg + e, (at[1] - at[0]) / 8, (at[2] - at[1]) / 4, (at[3] - at[2]) / 2,
                                         at[4] - at[3]);
      for (int32_t r = j; r < e; ++r) units_out_host[share_position(L, r - j)] = U[keyed[r].second];
      j = e;
    }
  } catch (...) {
    return STAG_ENOMEM;
  }
  return STAG_OK;
}
