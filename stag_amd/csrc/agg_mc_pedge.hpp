// agg_mc_pedge.hpp — the arguments of the Monte-Carlo aggregation kernels for [E, D] parameters (agg_mc_pedge.hip):
// stag_agg_fwd_mc_pedge.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

constexpr int kMcPEdgeMaxK = 4;   // samples per pass: 4, 2, 1 (every instantiation: 0 bytes of scratch)

struct McPEdgeArgs {
  // graph: destination-major
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // may be null (the position itself): the [E, D] parameter rows go by edge id
  const int32_t* nidx;     // may be null (the position itself)
  int32_t n_rows;
  int32_t D;
  // the gathered rows: fp32
  const float* x;
  uint32_t ldxb;           // row stride in bytes
  uint32_t x_bytes;        // extent of x when 32-bit byte offsets and 24-bit multiplies reach all of it, else 0
  int32_t xvec;            // rows take 16-byte loads
  // noise (noise.hpp flags: relu, log-scale); pmode is PER_EDGE: p0 / p1 = [E, D] by edge id, rows D floats apart
  int32_t pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  int32_t pvec;            // parameter rows take 16-byte loads
  PhiloxKey key;           // sample 0 of the pass; sample s draws mc_stride * s offsets further on
  uint32_t pos_lo, pos_hi;
  uint64_t mc_stride;
  // scaling / reduce
  const float* src_scale;
  const float* dst_scale;
  int32_t mean;
  // plan: null units = one unit per row, in row order
  const stag_unit* units;
  const int32_t* long_rows;
  const int32_t* long_seg_ptr;
  int32_t n_units, n_long, n_seg;
  float* ws;               // segment partials, sample-major: [K][n_seg][D] fp32
  // output: sample s of the pass at out + s * sample_stride
  float* out;
  int64_t ldo;
  int64_t sample_stride;
  int32_t ovec;            // out and ws take 16-byte stores
};

// one pass: k = 1, 2 or 4 samples from one walk of the units
hipError_t mc_pedge_launch(const McPEdgeArgs& a, int kind, int k, hipStream_t s);

}  // namespace stag
