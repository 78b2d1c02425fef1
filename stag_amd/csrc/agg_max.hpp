// agg_max.hpp — the arguments of the max-reducer kernels (agg_max.hip), shared with the entry points in api.hip.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

struct MaxArgs {
  // graph: destination-major (forward) or source-major (backward; nidx = forward position, eid = edge id)
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // may be null (identity)
  const int32_t* nidx;     // may be null (the position itself)
  int32_t n_rows;
  int32_t D;
  // the rows: gathered (forward) or owned by the unit (backward)
  const float* x;
  int64_t ldx;
  // noise (noise.hpp flags: relu | log-scale)
  int32_t kind, pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  PhiloxKey key;
  int64_t pos_base;
  uint32_t chunk_base;
  // plan: null units = one unit per row, in row order.  xcd: units point past the header of stag_plan.xcd_order,
  // sh / sl = records per heavy / light stripe; workgroup b serves stripe b % 8
  const stag_unit* units;
  const int32_t* long_rows;
  const int32_t* long_seg_ptr;
  int32_t n_units, n_long;
  int32_t xcd, sh, sl;
  float* ws;               // segment partials: [n_seg][nws * D]
  int32_t nws;
  // forward outputs
  float* out;
  int64_t ldo;
  int32_t* cnt;            // may be null
  int64_t ldc;
  // backward: og = [n_dst][ceil(D/4)][8] = (out[v, 4c..4c+3], gq[v, 4c..4c+3]) per chunk, written by the prep kernel
  const float* out_in;
  const int32_t* cnt_in;
  const float* g;
  int64_t ldf;             // row stride of out_in, cnt_in, g
  float* og;
  int32_t n_og_rows;
  float* dx;               // may be null
  float* dp0;              // [n_rows, ldd] parameter-derivative aggregates, or null
  float* dp1;
  int64_t ldd;             // row stride of dx, dp0, dp1
  float* dw;               // [E, ldw] by edge id (explicit weights), or null
  int64_t ldw;
};

hipError_t max_fwd_launch(const MaxArgs& a, int32_t n_seg, hipStream_t s);
hipError_t max_bwd_launch(const MaxArgs& a, int32_t n_seg, hipStream_t s);

}  // namespace stag
