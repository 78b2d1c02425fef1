// agg_bwd_pedge.hpp — the arguments of the one-pass backward of an aggregation with [E, D] noise parameters
// (agg_bwd_pedge.hip): stag_agg_bwd_pedge.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

struct BwdPEdgeArgs {
  // graph: source-major (rows = source nodes u, indices = destination rows v)
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // the edge id: parameter and gradient rows
  const int32_t* nidx;     // the forward CSR position: the draw
  int32_t n_rows;
  int32_t D;
  // the gathered gradient rows: fp32
  const float* g;
  uint32_t ldgb;           // row stride in bytes
  uint32_t g_bytes;        // extent of g when 32-bit byte offsets and 24-bit multiplies reach all of it, else 0
  int32_t gvec;            // rows take 16-byte loads
  const float* g_scale;    // [n_src] by destination row, may be null
  // the unit's own row of x
  const float* x;
  int64_t ldx;
  int32_t xvec;
  // noise (noise.hpp flags: relu, log-scale); pmode is PER_EDGE: p0 / p1 = [E, D] by edge id, rows D floats apart
  int32_t pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  int32_t pvec;            // parameter rows take 16-byte loads
  PhiloxKey key;
  uint32_t pos_lo, pos_hi;
  // scaling (unit_sum.hpp's names): dst_scale = row_scale[u], no mean
  const float* dst_scale;
  int32_t mean;
  // plan: null units = one unit per row, in row order
  const stag_unit* units;
  const int32_t* long_rows;
  const int32_t* long_seg_ptr;
  int32_t n_units, n_long, n_seg;
  float* ws;               // segment partials of dx: [n_seg][D] fp32
  // outputs
  float* out;              // dx, may be null (parameter gradients only)
  int64_t ldo;
  int32_t ovec;            // dx and ws take 16-byte stores
  float* dp0;              // [E, D] by edge id, rows ldp floats apart
  float* dp1;              // may be null
  int64_t ldp;
  int32_t wvec;            // gradient rows take 16-byte stores
};

// one walk of the units, then the merge of the long rows' dx partials (when dx is asked for and the plan has segments)
hipError_t bwd_pedge_launch(const BwdPEdgeArgs& a, int kind, hipStream_t s);

}  // namespace stag
