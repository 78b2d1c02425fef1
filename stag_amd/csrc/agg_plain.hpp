// agg_plain.hpp — the fused draw-and-aggregate kernel for the PLAIN FORWARD launch (gfx950).
//
// agg_kernel (agg_kernel.hpp) serves every launch form with one instruction stream: relu, the derivative selector,
// src_scale, in-norm, the transposed walk's noise index, both addressing forms and the parameter mode are run-time
// members of AggArgs, and the branches around them cost the hot loop register copies where they rejoin, VALU
// re-materialisations of wave-uniform flags and the packed forms of its multiplies.  The launch that a layer's forward
// pass makes most often uses none of them:
//   one output, sampled noise with SCALAR parameters, no derivative, no src_scale, no in-norm, the CSR's own positions
//   as noise indices, rows behind a buffer descriptor, D a multiple of 4, 32 or 64 lanes per row.
// agg_plain_kernel is that launch with every one of these a compile-time fact.  Unit decoding, the epilogue, the
// segment partials and the long-row combine are agg_unit's, run on a copy of the arguments whose launch-uniform
// members are constants; the unit's edges are walked by plain_walk, AggTeam::compute at two edges per block written out
// for this launch alone.  Every addition and every fp32 operation happens in the order of the general kernel, so the
// result is bit-identical to it (tests/test_gpu_agg_plain.py).  agg_launch_shape takes the kernel exactly when
// plain_launch_ok() holds; STAG_AGG_PLAIN=0 in the environment keeps the general kernel (read at each launch).
// Instruction counts, the occupancy decision and the measurements: DESIGN.md 4.1.
#pragma once
#include "agg_kernel.hpp"

namespace stag {

// Waves per SIMD the kernel is built for, as BOTH bounds of amdgpu_waves_per_eu: the register allocator may use what
// that occupancy leaves (72 VGPRs at 7) and the kernel descriptor asks for at least the registers that keep an eighth
// wave out, however few the loop needs — fewer instructions and more residency are separate decisions.
#ifndef STAG_PLAIN_WAVES
#define STAG_PLAIN_WAVES 7
#endif

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// draw4 of a launch with SCALAR parameters, in the packed form: w[0] = channels 0-1, w[1] = channels 2-3 of the lane's
// chunk.  The same operations on the same values as draw4 (one multiply, one fused multiply-add per channel; nothing
// is contracted or reassociated), written as pairs so that every one of them is a v_pk_* instruction and the pairs
// come out in the order the multiply with the gathered row wants them.  p0 = {p0s, p0s} lives in VGPRs (a second
// scalar operand would cost the packed fma a copy: the constant bus takes one); p1 = the scale (Normal), high - low
// (Uniform), unused (Bernoulli).
template <int KIND, bool RELU>
__device__ __forceinline__ void plain_draw4(uint32_t c0, uint32_t c1, const PhiloxKey& key, f32x2_t p0, float p1,
                                            f32x2_t (&w)[2]) {
  uint32_t r[4];
  philox4x32_10(c0, c1, key, r);
  const f32x2_t s = {p1, p1};
  if constexpr (KIND == kNormal) {
    const f32x2_t z01 = f32x2_t{bm_cos(r[1]), bm_sin(r[1])} * bm_radius(r[0]);
    const f32x2_t z23 = f32x2_t{bm_cos(r[3]), bm_sin(r[3])} * bm_radius(r[2]);
    w[0] = __builtin_elementwise_fma(s, z01, p0);
    w[1] = __builtin_elementwise_fma(s, z23, p0);
  } else if constexpr (KIND == kUniform) {
    w[0] = __builtin_elementwise_fma(s, f32x2_t{u01(r[0]), u01(r[1])}, p0);
    w[1] = __builtin_elementwise_fma(s, f32x2_t{u01(r[2]), u01(r[3])}, p0);
  } else {
    w[0] = f32x2_t{u01(r[0]) < p0.x ? 1.0f : 0.0f, u01(r[1]) < p0.y ? 1.0f : 0.0f};
    w[1] = f32x2_t{u01(r[2]) < p0.x ? 1.0f : 0.0f, u01(r[3]) < p0.y ? 1.0f : 0.0f};
  }
  if constexpr (RELU) {
    w[0] = __builtin_elementwise_max(w[0], f32x2_t{0.f, 0.f});
    w[1] = __builtin_elementwise_max(w[1], f32x2_t{0.f, 0.f});
  }
}

// The unit's edges, two per block: ids -> rows -> draws -> the block's sum from zero -> fold, as AggTeam::compute
// does it at BLK 2, MULT 1 (one slot, draws first), with nothing in the loop that the plain launch does not need.
template <int KIND, int LPE, bool RELU, class TEAM>
__device__ __forceinline__ void plain_walk(const AggArgs& a, TEAM& T, const int b, const int pend, const int len) {
  // column ids: 32-bit byte offsets behind a descriptor of `indices` (no 64-bit pointer to bump: quarter rate)
  const __amdgpu_buffer_rsrc_t ri =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(a.indices), 0, (int)a.idx_bytes, 0x00020000);
  f32x2_t p0 = {a.p0s, a.p0s};
  asm volatile("" : "+v"(p0));                  // stays in a VGPR pair: not re-made from the SGPR at every draw
  const float p1 = KIND == kUniform ? a.p1s - a.p0s : a.p1s;
  const uint32_t pos1 = a.pos_lo + 1u;
  f32x2_t s01 = {0.f, 0.f}, s23 = {0.f, 0.f}, c01 = {0.f, 0.f}, c23 = {0.f, 0.f};
  const int pend1 = pend - 1;
  for (int p = b; p < pend; p += 2) {
    const bool two = p < pend1;        // the block's second edge exists (what it loads stays unread otherwise)
#if STAG_LOAD_PRIO
    __builtin_amdgcn_s_setprio(3);   // get the loads out ahead of other waves' draws
#endif
    const int u0 = (int)__builtin_amdgcn_raw_buffer_load_b32(ri, p << 2, 0, 0);
    int u1;
    if (two) u1 = (int)__builtin_amdgcn_raw_buffer_load_b32(ri, (p << 2) + 4, 0, 0);
    // the noise indices are complete in registers before the rows are asked for (AggTeam::pin_idx)
    uint32_t n0 = a.pos_lo + (uint32_t)p, n1 = pos1 + (uint32_t)p;
    asm volatile("" : "+v"(n0));
    asm volatile("" : "+v"(n1));
    u32x4_t x1;
    const u32x4_t x0 = __builtin_amdgcn_raw_buffer_load_b128(T.rx, (int)(__umul24((uint32_t)u0, a.ldxb) + T.koff), 0, STAG_X_AUX);
    if (two) x1 = __builtin_amdgcn_raw_buffer_load_b128(T.rx, (int)(__umul24((uint32_t)u1, a.ldxb) + T.koff), 0, STAG_X_AUX);
#if STAG_LOAD_PRIO
    if (len > STAG_PRIO_MIN_LEN) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(0);
#endif
    // all the block's draws first: they need nothing from memory and run while its rows are in flight
    f32x2_t w0[2], w1[2];
    plain_draw4<KIND, RELU>(n0, T.c1, T.key, p0, p1, w0);
    if (two) plain_draw4<KIND, RELU>(n1, T.c1, T.key, p0, p1, w1);
    const f32x2_t zero = {0.f, 0.f};
    f32x2_t t01 = __builtin_elementwise_fma(w0[0], f32x2_t{__uint_as_float(x0.x), __uint_as_float(x0.y)}, zero);
    f32x2_t t23 = __builtin_elementwise_fma(w0[1], f32x2_t{__uint_as_float(x0.z), __uint_as_float(x0.w)}, zero);
    if (two) {
      asm volatile("" ::: "memory");   // keep this a branch: as selects it costs 4 VALU ops per block
      t01 = __builtin_elementwise_fma(w1[0], f32x2_t{__uint_as_float(x1.x), __uint_as_float(x1.y)}, t01);
      t23 = __builtin_elementwise_fma(w1[1], f32x2_t{__uint_as_float(x1.z), __uint_as_float(x1.w)}, t23);
    }
    if (T.kahan) {                     // AggTeam::fold_into, two channels per instruction
      const f32x2_t y01 = t01 - c01, y23 = t23 - c23;
      const f32x2_t n01 = s01 + y01, n23 = s23 + y23;
      c01 = (n01 - s01) - y01; c23 = (n23 - s23) - y23;
      s01 = n01; s23 = n23;
    } else {
      s01 += t01; s23 += t23;
    }
  }
  T.acc[0] = s01.x; T.acc[1] = s01.y; T.acc[2] = s23.x; T.acc[3] = s23.y;
}

template <int KIND, int LPE, bool RELU, bool WALK>
__global__ __launch_bounds__(STAG_BLOCK_THREADS)
__attribute__((amdgpu_waves_per_eu(STAG_PLAIN_WAVES, STAG_PLAIN_WAVES))) void agg_plain_kernel(const AggArgs a_in) {
  static_assert(KIND >= kNormal && (LPE == 32 || LPE == 64), "the plain launch: sampled noise, 32 or 64 lanes per row");
  static_assert(heavy_slots_of<KIND, LPE>() == 1 && mult_of<KIND, LPE>() == 1, "wide shapes walk one slot, one block");
  AggArgs a = a_in;
  // what a unit needs before its first gather, fetched together (hoist_args; only the members this launch reads)
  if constexpr (WALK) {
    STAG_PIN_S(a.walk.smask); STAG_PIN_S(a.walk.sshift); STAG_PIN_S(a.walk.jh_light);
    STAG_PIN_S(a.walk.sh); STAG_PIN_S(a.walk.lbase); STAG_PIN_S(a.walk.sl); STAG_PIN_S(a.walk.n_total);
  }
  STAG_PIN_S(a.D); STAG_PIN_S(a.units); STAG_PIN_S(a.indptr); STAG_PIN_S(a.indices);
  STAG_PIN_S(a.x); STAG_PIN_S(a.ldxb); STAG_PIN_S(a.x_bytes); STAG_PIN_S(a.idx_bytes);
  STAG_PIN_S(a.p0s); STAG_PIN_S(a.p1s);
  STAG_PIN_S(a.key.k0); STAG_PIN_S(a.key.k1); STAG_PIN_S(a.key.o0); STAG_PIN_S(a.key.o1); STAG_PIN_S(a.key.epoch);
  STAG_PIN_S(a.pos_lo); STAG_PIN_S(a.pos_hi); STAG_PIN_S(a.chunk_base);
  // the launch-uniform facts (plain_launch_ok): constants from here on
  a.nflags = RELU ? kFlagRelu : 0;
  a.in_norm = 0; a.norm_scale_out = nullptr;
  a.src_scale = nullptr;
  a.nidx = nullptr; a.eid = nullptr;
  a.pmode = STAG_PARAM_SCALAR; a.p0 = nullptr; a.p1 = nullptr;
  a.wide = 0;
  __builtin_assume(a.x_bytes != 0);
  __builtin_assume(a.out != nullptr);

  const int c = threadIdx.x % LPE;
  constexpr int TPB = STAG_BLOCK_THREADS / LPE;
  if constexpr (!WALK) {
    const int unit = blockIdx.x * TPB + threadIdx.x / LPE;
    if (unit >= a.n_units) return;
    agg_unit<KIND, LPE, true, 0, 1, 1, 1, false, false, false, RELU ? 3 : 1>(a, unit, c, 0);
  } else {
    // the one-slot walk of agg_kernel: heavy stripes first (jh_light blocks each), then the light ones
    const AggArgs::Walk w = a.walk;
    const int stripe = blockIdx.x & w.smask;
    int j = blockIdx.x >> w.sshift;
    int unit0, end;
    if (j < w.jh_light) {
      unit0 = stripe * w.sh + j * TPB;
      end = (stripe + 1) * w.sh;
    } else {
      j -= w.jh_light;
      unit0 = w.lbase + stripe * w.sl + j * TPB;
      end = min(w.lbase + (stripe + 1) * w.sl, w.n_total);
    }
    const int unit = unit0 + threadIdx.x / LPE;
    if (unit >= end) return;
    agg_unit<KIND, LPE, true, 0, 1, 1, 1, false, false, true, RELU ? 3 : 1>(a, unit, c, 0);
  }
}

template <int KIND>
inline void agg_launch_plain_impl(const AggArgs& a, int lpe, bool walk, dim3 grid, hipStream_t s) {
  const dim3 block(STAG_BLOCK_THREADS);
  const bool relu = (a.nflags & kFlagRelu) != 0;
#define STAG_PLAIN_GO(L, R, W) hipLaunchKernelGGL((agg_plain_kernel<KIND, L, R, W>), grid, block, STAG_AGG_LDS_BYTES, s, a)
  if (lpe == 32) {
    if (walk) { if (relu) STAG_PLAIN_GO(32, true, true); else STAG_PLAIN_GO(32, false, true); }
    else      { if (relu) STAG_PLAIN_GO(32, true, false); else STAG_PLAIN_GO(32, false, false); }
  } else {
    if (walk) { if (relu) STAG_PLAIN_GO(64, true, true); else STAG_PLAIN_GO(64, false, true); }
    else      { if (relu) STAG_PLAIN_GO(64, true, false); else STAG_PLAIN_GO(64, false, false); }
  }
#undef STAG_PLAIN_GO
}

}  // namespace stag
