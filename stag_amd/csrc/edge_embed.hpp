// edge_embed.hpp — the arguments of the wide edge-embedding kernels (edge_embed.hip): stag_edge_embed_fwd / _bwd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stag_hip.h"

namespace stag {

// h[e, :] = SiLU(ps[src[e], :] + pd[dst[e], :]), edges by edge id
struct EmbedFwdArgs {
  const int32_t* src;
  const int32_t* dst;
  int64_t E;
  const float* ps;
  const float* pd;
  int64_t ldps, ldpd;      // row strides in floats
  int32_t D;
  int32_t pvec;            // both tables take 16-byte loads
  float* h;
  int64_t ldh;
  int32_t hvec;            // h takes 16-byte stores
};

// d_own[r, :] = sum_{p in row r} g[eid[p], :] * SiLU'(own[r, :] + other[indices[p], :]) over one CSR view.
// The plan fields, ws, out, ldo, ovec, dst_scale and mean carry the names unit_sum.hpp reads.
struct EmbedBwdArgs {
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* eid;      // may be null (the position itself)
  int32_t D;
  const float* own;        // the row's endpoint: one row per unit
  int64_t ld_own;
  const float* x;          // the other endpoint's table, gathered by indices[p]
  uint32_t ldxb;           // row stride in bytes
  uint32_t x_bytes;        // extent of x when 32-bit byte offsets and 24-bit multiplies reach all of it, else 0
  const float* g;          // the incoming gradient [E, D], gathered by edge id
  uint32_t ldgb;
  uint32_t g_bytes;
  int32_t xvec;            // own, x and g rows take 16-byte loads
  // (no scaling: seg_merge's row_scale multiplies by 1)
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

hipError_t embed_fwd_launch(const EmbedFwdArgs& a, hipStream_t s);
hipError_t embed_bwd_launch(const EmbedBwdArgs& a, int32_t n_seg, hipStream_t s);

}  // namespace stag
