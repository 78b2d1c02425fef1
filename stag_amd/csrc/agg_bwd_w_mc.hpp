// agg_bwd_w_mc.hpp — the arguments of the batched Monte-Carlo parameter-gradient kernel (agg_bwd_w_mc.hip):
// stag_agg_bwd_w_mc.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

constexpr int kBwdWMcMaxK = 4;   // samples per pass: 4, 2, 1 (every instantiation: 0 bytes of scratch)

struct BwdWMcArgs {
  // graph: destination-major
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // may be null (the position itself): parameters and gradients go by edge id
  const int32_t* nidx;     // may be null (the position itself)
  int32_t n_rows;
  int32_t D;
  // the gathered rows and the unit's own gradient rows: fp32
  const float* x;
  int64_t ldx;
  const float* g;          // sample 0 of the pass; sample s at g + s * g_sample_stride
  int64_t ldg;
  int64_t g_sample_stride;
  const float* src_scale;
  const float* g_scale;
  int32_t xvec, gvec;      // rows take 16-byte loads
  // noise (noise.hpp flags: relu, log-scale); pmode PER_EDGE: p0 / p1 = [E, D] by edge id, rows D floats apart;
  // PER_EDGE1: [E]
  int32_t pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  int32_t pvec;            // [E, D] parameter rows take 16-byte loads
  PhiloxKey key;           // sample 0 of the pass; sample s draws mc_stride * s offsets further on
  uint32_t pos_lo, pos_hi;
  uint64_t mc_stride;
  // plan: null units = one unit per row, in row order
  const stag_unit* units;
  const int32_t* long_rows;
  int32_t n_units;
  // output: [E, D] rows ldw floats apart, or [E, 1] with reduce_k (the sum over k as well)
  int32_t reduce_k;
  int32_t accumulate;      // a later pass of the call: add to what the previous pass left for the same edge
  float* dw0;
  float* dw1;              // may be null
  int64_t ldw;
  int32_t wvec;            // gradient rows take 16-byte loads and stores
};

// one pass: k = 1, 2 or 4 samples from one walk of the units
hipError_t bwd_w_mc_launch(const BwdWMcArgs& a, int kind, int k, hipStream_t s);

}  // namespace stag
