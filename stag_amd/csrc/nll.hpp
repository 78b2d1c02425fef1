// nll.hpp — the arguments of the fused likelihood head (nll.hip): stag_nll_categorical_fwd / _bwd, stag_nll_bernoulli_fwd / _bwd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stag_hip.h"

namespace stag {

// Rows of one workgroup of the forward: a function of nothing but the number of rows, so the partials — and with them
// every bit of the value — depend on (n_rows, C, the data) alone.  64 rows up to 131,072, then the power of two that
// keeps the slabs at 2048 or fewer (node_norm.hpp's rule).
inline int64_t nll_slab_rows(int64_t n_rows) {
  int64_t s = 64;
  while (s * 2048 < n_rows) s <<= 1;
  return s;
}
inline int64_t nll_slabs(int64_t n_rows) {
  const int64_t s = nll_slab_rows(n_rows);
  return (n_rows + s - 1) / s;
}

// what a slab leaves in the workspace: the sum of its masked rows' terms and how many rows that were
struct NllPartial {
  float sum;
  int32_t count;
};

// One call, either likelihood and either direction (the fields a direction does not read stay null).
struct NllArgs {
  const float* p;          // probabilities [N, C]
  int64_t ldp;             // row strides in floats
  int64_t N;
  int32_t C;
  int32_t pvec;            // p rows take 16-byte loads
  const int64_t* label;    // categorical: [N]
  const float* y;          // Bernoulli: [N, C]
  int64_t ldy;
  int32_t yvec;
  const uint8_t* mask;     // [N] or null: every row
  // forward
  int64_t slab;
  int32_t n_slabs;
  NllPartial* part;        // [n_slabs]
  float* value;            // [1]
  float* denom;            // [1]
  // backward
  const float* g;          // [1], device
  const float* denom_in;   // [1], device
  float* dp;
  int64_t lddp;
  int32_t dvec;
};

hipError_t nll_fwd_launch(const NllArgs& a, bool bernoulli, hipStream_t s);
hipError_t nll_bwd_launch(const NllArgs& a, bool bernoulli, hipStream_t s);

}  // namespace stag
