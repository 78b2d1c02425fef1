// agg_half.hpp — the arguments of the half-row aggregation kernels (agg_half.hip): stag_agg_fwd_half.
#pragma once
#include "../../include/stag_hip.h"
#include "noise.hpp"

namespace stag {

struct HalfArgs {
  // graph: destination-major, or source-major with nidx = forward position (the transposed walk)
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* nidx;     // may be null (the position itself)
  int32_t n_rows;
  int32_t D;
  // the gathered rows: fp16 or bf16, 16-byte aligned, row stride a multiple of 8 elements
  const void* x;
  uint32_t ldxb;           // row stride in bytes
  uint32_t x_bytes;        // extent of x when 32-bit byte offsets and 24-bit multiplies reach all of it, else 0
  // noise (noise.hpp flags: relu only)
  int32_t pmode, nflags;
  const float* p0;
  const float* p1;
  float p0s, p1s;
  PhiloxKey key;
  uint32_t pos_lo, pos_hi;
  uint32_t chunk_base;
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

hipError_t half_fwd_launch(const HalfArgs& a, int kind, int dtype, int32_t n_seg, hipStream_t s);

}  // namespace stag
