// agg_half.hip — stag_agg_fwd_half: the fused draw-and-aggregate pass over fp16 / bf16 feature rows (gfx950).
//
//   out[v, k] = dscale[v] * sum_p w[p, k] * sscale[u_p] * float(x[u_p, k])        fp32 accumulation, fp32 output
//
// What a layer under torch.autocast hands the aggregation is a half-typed h = x @ W; widened to fp32 before the launch
// it costs a streaming cast pass, an fp32 copy and a gather of E rows at 4 bytes per channel.  Here the rows are
// gathered as they are: a lane owns EIGHT consecutive channels — one 16-byte buffer load per edge, half the bytes of
// the fp32 kernels' row — widens them in registers (bf16: a shift or a mask; fp16: v_cvt_f32_f16; both exact) and
// draws the two Philox blocks its channels belong to (chunks chunk_base + 2c and + 2c + 1 of include/stag_hip.h's
// noise stream: the same w[e, k] bits as an fp32 launch with the same spec).  A row takes D / 8 lanes, a team is the
// next power of two of that (8 ... 64 lanes); channels past 512 go to further channel tiles (blockIdx.y).
// How the plan's units are walked, a block sum is folded and a long row's segments are merged: unit_sum.hpp.  Edges are
// taken in blocks (2 with a draw, 4 without).  agg_kernel / agg_plain_kernel are not touched: they are tuned to the VGPR.
#include "agg_half.hpp"
#include "unit_sum.hpp"     // the unit walk, the row scale, the N-wide store; agg_kernel.hpp's load4, u32x4_t

namespace stag {
namespace {

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// edges fetched together by a team: the draws of a block run while its rows are in flight
template <int KIND>
constexpr int half_blk() { return KIND == kNone ? 4 : 2; }

// the 8 channels of one 16-byte piece of a row, widened exactly
template <int DT>
__device__ __forceinline__ void widen8(const u32x4_t t, float (&v)[8]) {
  const uint32_t wd[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (DT == STAG_DTYPE_BF16) {
      v[2 * i] = __uint_as_float(wd[i] << 16);
      v[2 * i + 1] = __uint_as_float(wd[i] & 0xFFFF0000u);
    } else {
      const f16x2_t h = __builtin_bit_cast(f16x2_t, wd[i]);
      v[2 * i] = (float)h.x;
      v[2 * i + 1] = (float)h.y;
    }
  }
}

template <int KIND, int DT, int LPE>
__global__ __launch_bounds__(256) void agg_half_fwd_kernel(const HalfArgs a) {
  constexpr int BLK = half_blk<KIND>();
  const int c = blockIdx.y * LPE + threadIdx.x % LPE;   // the lane's group of 8 channels
  const int k0 = 8 * c;
  int row, start, len, slot;
  if (k0 >= a.D || !unit_of<LPE>(a, row, start, len, slot)) return;
  const PhiloxKey key = resolve_epoch(a.key);
  const uint32_t koff = (uint32_t)k0 * 2u;
  const bool narrow = a.x_bytes != 0;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  // the two Philox blocks of the lane's channels: chunks chunk_base + 2c, + 2c + 1 (word 1: chunk | hi32(gpos) << 20)
  const uint32_t c1a = (a.chunk_base + 2u * (uint32_t)c) | (a.pos_hi << 20);
  const uint32_t c1b = (a.chunk_base + 2u * (uint32_t)c + 1u) | (a.pos_hi << 20);
  [[maybe_unused]] float pa[2][4], pb[2][4];
  if constexpr (KIND >= kNormal) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool row_p = a.pmode == STAG_PARAM_PER_CHANNEL;
      pa[q >> 2][q & 3] = row_p ? a.p0[k0 + q] : a.p0s;
      pb[q >> 2][q & 3] = row_p ? (a.p1 ? a.p1[k0 + q] : 0.f) : a.p1s;
    }
  }
  const bool kahan = len > kKahanMinLen;
  float acc[8], comp[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = comp[q] = 0.f;
  const int end = start + len;
  for (int p0 = start; p0 < end; p0 += BLK) {
    int u[BLK];
    uint32_t nn[BLK];
    float xs[BLK];
    u32x4_t xr[BLK];
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
      const int p = p0 + j;
      if (p < end) {
        u[j] = a.indices[p];
        nn[j] = a.pos_lo + (uint32_t)(a.nidx ? a.nidx[p] : p);
      }
    }
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
      if (p0 + j < end) {
        if (narrow) {
          xr[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(__umul24((uint32_t)u[j], a.ldxb) + koff), 0, 0);
        } else {
          const char* r = static_cast<const char*>(a.x) + (uint64_t)(uint32_t)u[j] * a.ldxb + koff;
          xr[j] = *reinterpret_cast<const u32x4_t*>(r);
        }
        if (a.src_scale) xs[j] = a.src_scale[u[j]];
      }
    }
    // all the block's draws first: they need nothing from memory and run while its rows are in flight
    [[maybe_unused]] float w[BLK][2][4];
    if constexpr (KIND >= kNormal) {
#pragma unroll
      for (int j = 0; j < BLK; ++j) {
        if (p0 + j < end) {
          draw4<KIND>(nn[j], c1a, key, pa[0], pb[0], a.nflags, w[j][0]);
          draw4<KIND>(nn[j], c1b, key, pa[1], pb[1], a.nflags, w[j][1]);
        }
      }
    }
    float t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = 0.f;
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
      if (p0 + j < end) {
        float xv[8];
        widen8<DT>(xr[j], xv);
        if (a.src_scale) {
#pragma unroll
          for (int q = 0; q < 8; ++q) xv[q] *= xs[j];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if constexpr (KIND == kNone) t[q] += xv[q];
          else t[q] = __builtin_fmaf(w[j][q >> 2][q & 3], xv[q], t[q]);
        }
      }
    }
    // fold_block<8> (unit_sum.hpp), written out: through the helper this kernel's instructions move
    if (kahan) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float y = t[q] - comp[q];
        const float n = acc[q] + y;
        comp[q] = (n - acc[q]) - y;
        acc[q] = n;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += t[q];
    }
  }
  if (slot >= 0) {   // a segment: its partial, added by agg_half_merge_kernel
    store_n(a.ws + (int64_t)slot * a.D, k0, a.D, a.ovec != 0, acc);
    return;
  }
  const float dv = row_scale(a, row, len);
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] *= dv;
  store_n(a.out + (int64_t)row * a.ldo, k0, a.D, a.ovec != 0, acc);
}

// seg_merge<8, LPE> (unit_sum.hpp), written out: through the template the call at seg_len = 16 on the arxiv-shaped graph
// (four rounds of the merge) measured 0.17 us slower than this body, the parent's own spread being 0.03 (profiles/r16)
template <int LPE>
__global__ __launch_bounds__(256) void agg_half_merge_kernel(const HalfArgs a) {
  constexpr int T = 256 / LPE, kAhead = 8;
  __shared__ float part[T][2][LPE * 8];          // a round's group sums and what they still owe (16 KB)
  const int r = blockIdx.x, team = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const int k0 = 8 * (blockIdx.y * LPE + lane);
  const bool live = k0 < a.D;                    // (no early return: the workgroup meets at barriers)
  const int row = a.long_rows[r];
  const int s0 = a.long_seg_ptr[r], s1 = a.long_seg_ptr[r + 1];
  const bool vec = a.ovec != 0;
  float sum[8], comp[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) sum[q] = comp[q] = 0.f;
  for (int g0 = s0; g0 < s1; g0 += kCombineGroup * T) {   // uniform over the workgroup
    const int gs = g0 + team * kCombineGroup;
    if (live && gs < s1) {
      const int ge = min(gs + kCombineGroup, s1);
      float gsum[8], gres[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) gsum[q] = gres[q] = 0.f;
      for (int s = gs; s < ge; s += kAhead) {
        float t[kAhead][2][4];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
          if (s + j < ge) {
            const float* ws = a.ws + (int64_t)(s + j) * a.D;
            load4(ws, k0, a.D, vec, t[j][0]);
            load4(ws, k0 + 4, a.D, vec, t[j][1]);
          }
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
          if (s + j < ge) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const float y = t[j][q >> 2][q & 3] - gres[q];
              const float n = gsum[q] + y;
              gres[q] = (n - gsum[q]) - y;
              gsum[q] = n;
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) { part[team][0][lane * 8 + q] = gsum[q]; part[team][1][lane * 8 + q] = gres[q]; }
    }
    __syncthreads();
    if (team == 0 && live) {
      for (int j = 0; j < T && g0 + j * kCombineGroup < s1; ++j) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          comp[q] += part[j][1][lane * 8 + q];             // true group sum = its sum - its residual
          const float y = part[j][0][lane * 8 + q] - comp[q];
          const float n = sum[q] + y;
          comp[q] = (n - sum[q]) - y;
          sum[q] = n;
        }
      }
    }
    __syncthreads();                                       // the next round overwrites the group sums
  }
  if (team != 0 || !live) return;
  const float dv = row_scale(a, row, a.indptr[row + 1] - a.indptr[row]);
#pragma unroll
  for (int q = 0; q < 8; ++q) sum[q] = (sum[q] - comp[q]) * dv;
  store_n(a.out + (int64_t)row * a.ldo, k0, a.D, vec, sum);
}

template <int KIND>
void half_fwd_kind(const HalfArgs& a, int dtype, int lpe, dim3 grid, hipStream_t s) {
  pick<64, 32, 16, 8>(lpe, [&](auto L) {
    pick<STAG_DTYPE_BF16, STAG_DTYPE_F16>(dtype, [&](auto DT) {
      hipLaunchKernelGGL((agg_half_fwd_kernel<KIND, decltype(DT)::value, decltype(L)::value>), grid, dim3(256), 0, s, a);
    });
  });
}

}  // namespace

hipError_t half_fwd_launch(const HalfArgs& a, int kind, int dtype, int32_t n_seg, hipStream_t s) {
  return unit_sum_launch(a.D, 8, 8, a.n_units, a.n_long, n_seg,
      [&](int lpe, dim3 grid) {
        pick<kNone, kNormal, kUniform, kBernoulli>(kind, [&](auto K) { half_fwd_kind<decltype(K)::value>(a, dtype, lpe, grid, s); });
      },
      [&](int lpe, dim3 grid) {
        pick<64, 32, 16, 8>(lpe, [&](auto L) {
          hipLaunchKernelGGL((agg_half_merge_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
        });
      });
}

}  // namespace stag

using namespace stag;

extern "C" int stag_agg_fwd_half(const stag_csr* csr, const stag_plan* plan, const void* x, int32_t x_dtype, int64_t ldx,
                                 int32_t D, const stag_noise_spec* spec, int32_t reduce, const float* src_scale,
                                 const float* dst_scale, float* out, int64_t ldo, void* stream) {
  // every decision below is taken before any device work
  int rc = check_csr(csr);
  if (rc) return rc;
  if (!x || !spec || !out) return STAG_EINVAL;
  if (D <= 0 || ldx < 0 || (ldx > 0 && ldx < D) || ldo < D) return STAG_EINVAL;
  if (x_dtype != STAG_DTYPE_F16 && x_dtype != STAG_DTYPE_BF16) return STAG_EINVAL;
  if (spec->kind < STAG_NOISE_NONE || spec->kind > STAG_NOISE_BERNOULLI) return STAG_EINVAL;
  if (reduce != STAG_REDUCE_SUM && reduce != STAG_REDUCE_MEAN) return STAG_EINVAL;
  if (spec->deriv != 0) return STAG_EINVAL;
  if (spec->chunk_base < 0 || spec->chunk_base >= (1 << 20)) return STAG_EINVAL;
  if (spec->p1_log != 0 && (spec->p1_log != 1 || spec->kind != STAG_NOISE_NORMAL)) return STAG_EINVAL;
  const bool drawn = spec->kind >= STAG_NOISE_NORMAL;
  if (drawn) {
    if (!counter_space_ok(spec->pos_base, csr->n_edges, spec->chunk_base, ((int64_t)D + 3) / 4)) return STAG_EINVAL;
    if (spec->param_mode < STAG_PARAM_SCALAR || spec->param_mode > STAG_PARAM_PER_EDGE) return STAG_EINVAL;
    if (spec->param_mode == STAG_PARAM_PER_CHANNEL && (!spec->p0 || (spec->kind != STAG_NOISE_BERNOULLI && !spec->p1)))
      return STAG_EINVAL;
  }
  const bool use_plan = plan_in_use(plan);
  if (use_plan && check_plan_units(plan, kPlanCounts)) return STAG_EINVAL;
  // what the cast route (x.float(), stag_agg_fwd) keeps
  if (D % 8 != 0 || ldx == 0 || ldx % 8 != 0 || !aligned16(x)) return STAG_ENOSYS;
  if (spec->in_norm || spec->kind == STAG_NOISE_EXPLICIT || spec->p1_log) return STAG_ENOSYS;
  if (drawn && spec->param_mode > STAG_PARAM_PER_CHANNEL) return STAG_ENOSYS;
  rc = check_positions(spec, csr->n_edges, D, drawn);                      // as stag_agg_fwd: one 2^32 range per call
  if (rc) return rc;
  const int32_t n_seg = use_plan ? plan->n_seg : 0;
  if (use_plan && (rc = check_plan_segments(plan, kPlanSegPtr | kPlanWorkspace, stag_plan_workspace_bytes(n_seg, D, 0)))) return rc;
  if (csr->n_dst == 0) return STAG_OK;

  HalfArgs a{};
  a.indptr = csr->indptr; a.indices = csr->indices; a.nidx = csr->nidx;   // (csr->eid: nothing here is indexed by edge id)
  a.n_rows = csr->n_dst; a.D = D;
  a.x = x; a.ldxb = (uint32_t)(ldx * 2);
  if ((rc = narrow_rows(csr->n_src, ldx, D, 2, a.x_bytes))) return rc;
  fill_spec(a, spec, 0);   // (flags: relu only; a derivative and a log-scale were refused above)
  a.src_scale = src_scale; a.dst_scale = dst_scale; a.mean = reduce == STAG_REDUCE_MEAN;
  fill_plan(a, csr, plan);   // plan->xcd_order is ignored: the units are walked in plan order
  a.out = out; a.ldo = ldo;
  a.ovec = aligned16(out) && ldo % 4 == 0 && (n_seg == 0 || aligned16(plan->workspace));
  return half_fwd_launch(a, spec->kind, x_dtype, n_seg, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}
