// node_norm.hpp — the arguments of the fused node block (node_norm.hip): stag_node_norm_stats / _fwd / _bwd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

// Rows of one workgroup of the column reductions: a function of nothing but the number of rows, so the partials — and
// with them every bit of the result — depend on (n_rows, D, the data) alone.  64 rows up to 131,072, then the power of
// two that keeps the slabs at 2048 or fewer.
inline int64_t node_slab_rows(int64_t n_rows) {
  int64_t s = 64;
  while (s * 2048 < n_rows) s <<= 1;
  return s;
}
inline int64_t node_slabs(int64_t n_rows) {
  const int64_t s = node_slab_rows(n_rows);
  return (n_rows + s - 1) / s;
}

// What the elementwise map needs of one call: y = relu?(((x - mean) * rstd) * gamma + beta) * keep-mask / keep_prob
struct NodeMapArgs {
  const float* x;
  int64_t ldx;             // row strides in floats
  int64_t N;
  int32_t D;
  int32_t xvec;            // x rows take 16-byte loads
  const float* mean;       // [D]
  const float* rstd;       // [D]
  const float* gamma;      // [D] or null (1)
  const float* beta;       // [D] or null (0)
  int32_t relu;
  int32_t drop;            // a mask is drawn: draw4<kBernoulli> at (row, chunk) under key
  float keep, inv_keep;
  PhiloxKey key;
};

// column statistics: slab partials (mean, M2) into part, merged in slab order
struct NodeStatsArgs {
  const float* x;
  int64_t ldx, N, slab;
  int32_t D, xvec;
  float* part;             // [n_slabs][2][D]
  int32_t n_slabs;
  float eps;
  float* mean_out;         // [D]
  float* rstd_out;         // [D]
  float* running_mean;     // [D] or null
  float* running_var;      // [D] or null
  float factor;            // running = (1 - factor) * running + factor * batch
};

struct NodeFwdArgs {
  NodeMapArgs m;
  float* y;
  int64_t ldy;
  int32_t yvec;
};

struct NodeBwdArgs {
  NodeMapArgs m;
  const float* g;
  int64_t ldg;
  int32_t gvec;
  int64_t slab;
  int32_t n_slabs;
  int32_t batch_stats;     // the statistics were the batch's: dx carries the two mean terms
  float* sums;             // [2][D]: sum g', sum g' xhat (the merge writes them, the dx pass reads them)
  float* part;             // [n_slabs][2][D]
  float* dbeta;            // [D] or null
  float* dgamma;           // [D] or null
  float* dx;
  int64_t lddx;
  int32_t dvec;
};

hipError_t node_stats_launch(const NodeStatsArgs& a, hipStream_t s);
hipError_t node_fwd_launch(const NodeFwdArgs& a, hipStream_t s);
hipError_t node_bwd_launch(const NodeBwdArgs& a, bool want_sums, bool want_dx, hipStream_t s);

}  // namespace stag
