// agg_w1.hpp — the arguments of the one-weight-per-edge aggregation kernels (agg_w1.hip): stag_agg_fwd_w1.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

struct W1Args {
  // graph: destination-major, or source-major with nidx = forward position (the transposed walk)
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // may be null (the position itself): explicit weights and [E, 1] parameters go by edge id
  const int32_t* nidx;     // may be null (the position itself)
  int32_t n_rows;
  int32_t D;
  // the gathered rows: fp32
  const float* x;
  uint32_t ldxb;           // row stride in bytes
  uint32_t x_bytes;        // extent of x when 32-bit byte offsets and 24-bit multiplies reach all of it, else 0
  int32_t xvec;            // rows take 16-byte loads
  // noise at width 1 (noise.hpp flags: relu, log-scale); EXPLICIT: p0 = w[E] by edge id
  int32_t pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  PhiloxKey key;
  uint32_t pos_lo, pos_hi;
  // scaling / reduce
  const float* src_scale;
  const float* dst_scale;
  int32_t mean;
  // plan: null units = one unit per row, in row order
  const stag_unit* units;
  const int32_t* long_rows;
  const int32_t* long_seg_ptr;
  int32_t n_units, n_long;
  float* ws;               // segment partials: [n_seg][D] fp32
  // output
  float* out;
  int64_t ldo;
  int32_t ovec;            // out and ws take 16-byte stores
};

hipError_t w1_fwd_launch(const W1Args& a, int kind, int32_t n_seg, hipStream_t s);

}  // namespace stag
