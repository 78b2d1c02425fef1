// nll.hip — the likelihood end of the objective as fused passes (gfx950): the masked mean of the negative log-likelihood
// of Categorical(probs = p) or Bernoulli(probs = p) over node rows p [N, C], and its gradient (stag/models.py:69-76 with
// stag/likelihoods.py; torch's own arithmetic with validate_args off, eps = 2^-23).
//
//   categorical  s = sum_c p[n,c];  q = p[n,y_n] / s;  nll_n = -log(min(max(q, eps), 1 - eps))
//                value = sum_{n in mask} nll_n / count;  denom = count                                 stag_nll_categorical_fwd
//                dp[n,c] = -(g / count) * [eps <= q <= 1 - eps] * ([c == y_n] / p[n,y_n] - 1 / s)      stag_nll_categorical_bwd
//   Bernoulli    pc = min(max(p, eps), 1 - eps);  nll = -(y * log(pc) + (1 - y) * log1p(-pc))
//                value = sum / (count * C);  denom = count * C                                         stag_nll_bernoulli_fwd
//                dp = (g / denom) * [eps <= p <= 1 - eps] * (-y / pc + (1 - y) / (1 - pc))             stag_nll_bernoulli_bwd
//
// A team of LPE lanes takes a row, 4 channels a lane (16-byte loads when the rows allow it) and, past 256 channels,
// further channel tiles in a loop; 64 / LPE rows share a wave.  The mask byte is tested per team and the row's loads sit
// behind it: a row outside the mask costs that byte.  The row sum is a fixed xor butterfly inside the team.
//
// Forward: a workgroup takes a slab of nll_slab_rows(N) rows, a team the rows team, team + T, ... of it.  A team adds
// its rows' terms in row order; the teams of a wave are added by the same butterfly over the team bits, the four waves
// in wave order through LDS, and (sum, count) of the slab goes to the workspace.  A one-workgroup merge launch adds
// the slab partials in double: thread t the run of consecutive slabs t in slab order, then the 256 runs by a fixed
// halving tree, and writes value and denom.  No atomics, no arrival counters: the result is a function of (N, C, the
// data) alone and two calls give the same bits.  The backward is one elementwise launch that forms s again from the row;
// it reads g and denom on the device.  Rows take 64-bit offsets.
//
// A label outside [0, C) in a masked row gives that row the term NaN (so value is NaN) and a zero gradient, and no
// address is formed from it (torch device-asserts there).  A NaN in a masked row makes q, hence value, NaN.
#include "nll.hpp"
#include "agg_kernel.hpp"   // load4 / store4
#include "entry_args.hpp"

namespace stag {
namespace {

constexpr float kEps = 1.1920928955078125e-07f;   // 2^-23: torch.finfo(torch.float32).eps
constexpr float kHi = 1.0f - kEps;
constexpr int kBwdRows = 4;                        // rows a team of the backward takes, one after the other

// the sum over the LPE lanes of a team, the same bits in each of them
template <int LPE>
__device__ __forceinline__ float team_sum(float v) {
#pragma unroll
  for (int o = LPE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// min(max(q, eps), 1 - eps) as torch.clamp forms it: a NaN stays one
__device__ __forceinline__ float clamp_prob(float q) { return q < kEps ? kEps : (q > kHi ? kHi : q); }

__device__ __forceinline__ bool in_window(float q) { return q >= kEps && q <= kHi; }   // (false for a NaN)

__device__ __forceinline__ bool row_in_mask(const NllArgs& a, int64_t r) { return !a.mask || a.mask[r] != 0; }

// the lane's part of sum_c p[row, c]
template <int LPE>
__device__ __forceinline__ float lane_row_sum(const float* row, int lane, int C, bool vec) {
  float s = 0.0f;
  for (int k0 = 4 * lane; k0 < C; k0 += 4 * LPE) {
    float v[4];
    load4(row, k0, C, vec, v);       // (a channel past C: 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += v[j];
  }
  return s;
}

// the lane's part of a Bernoulli row's sum of terms
template <int LPE>
__device__ __forceinline__ float lane_bernoulli_sum(const NllArgs& a, int64_t r, int lane) {
  const float* prow = a.p + r * a.ldp;
  const float* yrow = a.y + r * a.ldy;
  float s = 0.0f;
  for (int k0 = 4 * lane; k0 < a.C; k0 += 4 * LPE) {
    float p[4], y[4];
    load4(prow, k0, a.C, a.pvec != 0, p);
    load4(yrow, k0, a.C, a.yvec != 0, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k0 + j < a.C) {
        const float pc = clamp_prob(p[j]);
        s += -(y[j] * logf(pc) + (1.0f - y[j]) * log1pf(-pc));
      }
    }
  }
  return s;
}

// teams of a wave by the butterfly over the team bits, waves in wave order: thread 0 writes the slab's partial
template <int LPE>
__device__ __forceinline__ void slab_fold(const NllArgs& a, float acc, int cnt) {
  __shared__ float ssum[4];
  __shared__ int scnt[4];
#pragma unroll
  for (int o = LPE; o < 64; o <<= 1) {
    acc += __shfl_xor(acc, o);
    cnt += __shfl_xor(cnt, o);
  }
  if (threadIdx.x % 64 == 0) {
    ssum[threadIdx.x / 64] = acc;
    scnt[threadIdx.x / 64] = cnt;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  NllPartial out{ssum[0], scnt[0]};
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    out.sum += ssum[w];
    out.count += scnt[w];
  }
  a.part[blockIdx.x] = out;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int LPE>
__global__ __launch_bounds__(256) void nll_cat_fwd_kernel(const NllArgs a) {
  constexpr int T = 256 / LPE;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = min(r0 + a.slab, a.N);
  float acc = 0.0f;
  int cnt = 0;
  for (int64_t base = r0; base < r1; base += T) {      // (the trip count is the workgroup's: every lane meets the butterfly)
    const int64_t r = base + team;
    const bool live = r < r1 && row_in_mask(a, r);
    float s = 0.0f, py = 0.0f;
    bool label_ok = false;
    if (live) {
      const float* row = a.p + r * a.ldp;
      const int64_t yl = a.label[r];
      label_ok = yl >= 0 && yl < a.C;
      if (label_ok) py = row[yl];
      s = lane_row_sum<LPE>(row, lane, a.C, a.pvec != 0);
    }
    s = team_sum<LPE>(s);
    if (live) {
      acc += label_ok ? -logf(clamp_prob(py / s)) : __builtin_nanf("");
      cnt += 1;
    }
  }
  slab_fold<LPE>(a, acc, cnt);
}

template <int LPE>
__global__ __launch_bounds__(256) void nll_bern_fwd_kernel(const NllArgs a) {
  constexpr int T = 256 / LPE;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = min(r0 + a.slab, a.N);
  float acc = 0.0f;
  int cnt = 0;
  for (int64_t base = r0; base < r1; base += T) {
    const int64_t r = base + team;
    const bool live = r < r1 && row_in_mask(a, r);
    float s = 0.0f;
    if (live) s = lane_bernoulli_sum<LPE>(a, r, lane);
    s = team_sum<LPE>(s);
    if (live) {
      acc += s;
      cnt += 1;
    }
  }
  slab_fold<LPE>(a, acc, cnt);
}

// the slab partials in double: runs of consecutive slabs in slab order, the runs by a fixed halving tree
__global__ __launch_bounds__(256) void nll_merge_kernel(const NllArgs a, int per_row) {
  __shared__ double ssum[256];
  __shared__ long long scnt[256];
  const int t = threadIdx.x;
  const int per = (a.n_slabs + 255) / 256;
  const int s0 = min(t * per, a.n_slabs), s1 = min(s0 + per, a.n_slabs);
  double sum = 0.0;
  long long cnt = 0;
  for (int s = s0; s < s1; ++s) {
    const NllPartial p = a.part[s];
    sum += (double)p.sum;
    cnt += p.count;
  }
  ssum[t] = sum;
  scnt[t] = cnt;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if (t < o) {
      ssum[t] += ssum[t + o];
      scnt[t] += scnt[t + o];
    }
  }
  if (t != 0) return;
  const double denom = (double)scnt[0] * (double)per_row;
  *a.value = (float)(ssum[0] / denom);            // no masked row: 0 / 0 = NaN, as the mean of nothing
  *a.denom = (float)denom;
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <int LPE>
__global__ __launch_bounds__(256) void nll_cat_bwd_kernel(const NllArgs a) {
  constexpr int T = 256 / LPE;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const float c0 = -(a.g[0] / a.denom_in[0]);
  const int64_t rb = (int64_t)blockIdx.x * (T * kBwdRows) + team;
  for (int j = 0; j < kBwdRows; ++j) {
    const int64_t r = rb + (int64_t)j * T;
    const bool inb = r < a.N;
    const bool live = inb && row_in_mask(a, r);
    float s = 0.0f, py = 0.0f;
    int64_t yl = -1;
    if (live) {
      const float* row = a.p + r * a.ldp;
      yl = a.label[r];
      if (yl >= 0 && yl < a.C) py = row[yl];
      else yl = -1;
      s = lane_row_sum<LPE>(row, lane, a.C, a.pvec != 0);
    }
    s = team_sum<LPE>(s);
    float d_y = 0.0f, d_other = 0.0f;
    if (live && yl >= 0 && in_window(py / s)) {       // (inside the window p_y > 0 and s > 0: nothing divides by 0)
      const float inv_s = 1.0f / s;
      d_y = c0 * (1.0f / py - inv_s);
      d_other = c0 * (0.0f - inv_s);
    }
    if (inb) {
      float* drow = a.dp + r * a.lddp;
      for (int k0 = 4 * lane; k0 < a.C; k0 += 4 * LPE) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (k0 + q == yl) ? d_y : d_other;
        store4(drow, k0, a.C, a.dvec != 0, v);
      }
    }
  }
}

template <int LPE>
__global__ __launch_bounds__(256) void nll_bern_bwd_kernel(const NllArgs a) {
  constexpr int T = 256 / LPE;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const float c0 = a.g[0] / a.denom_in[0];
  const int64_t rb = (int64_t)blockIdx.x * (T * kBwdRows) + team;
  for (int j = 0; j < kBwdRows; ++j) {
    const int64_t r = rb + (int64_t)j * T;
    if (r >= a.N) continue;
    const bool live = row_in_mask(a, r);
    const float* prow = a.p + r * a.ldp;
    const float* yrow = a.y + r * a.ldy;
    float* drow = a.dp + r * a.lddp;
    for (int k0 = 4 * lane; k0 < a.C; k0 += 4 * LPE) {
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (live) {
        float p[4], y[4];
        load4(prow, k0, a.C, a.pvec != 0, p);
        load4(yrow, k0, a.C, a.yvec != 0, y);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (in_window(p[q])) v[q] = c0 * (-y[q] / p[q] + (1.0f - y[q]) / (1.0f - p[q]));
      }
      store4(drow, k0, a.C, a.dvec != 0, v);
    }
  }
}

int lanes_of(int32_t C) { return lanes_for((C + 3) / 4, 1); }

}  // namespace

hipError_t nll_fwd_launch(const NllArgs& a, bool bernoulli, hipStream_t s) {
  pick<64, 32, 16, 8, 4, 2, 1>(lanes_of(a.C), [&](auto L) {
    if (bernoulli) hipLaunchKernelGGL((nll_bern_fwd_kernel<decltype(L)::value>), dim3((unsigned)a.n_slabs), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((nll_cat_fwd_kernel<decltype(L)::value>), dim3((unsigned)a.n_slabs), dim3(256), 0, s, a);
  });
  hipLaunchKernelGGL(nll_merge_kernel, dim3(1), dim3(256), 0, s, a, bernoulli ? a.C : 1);
  return hipGetLastError();
}

hipError_t nll_bwd_launch(const NllArgs& a, bool bernoulli, hipStream_t s) {
  const int lpe = lanes_of(a.C);
  const int64_t per_block = (256 / lpe) * kBwdRows;
  const dim3 grid((unsigned)((a.N + per_block - 1) / per_block));
  pick<64, 32, 16, 8, 4, 2, 1>(lpe, [&](auto L) {
    if (bernoulli) hipLaunchKernelGGL((nll_bern_bwd_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((nll_cat_bwd_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
  return hipGetLastError();
}

}  // namespace stag

using namespace stag;

namespace {

constexpr int64_t kMaxRows = 1ll << 34;    // the backward's row groups (16 rows or more each) fill grid.x below 2^31
constexpr int32_t kMaxC = 1 << 30;         // the channel loops count in 32 bits

bool vec_rows(const void* p, int64_t ld, int32_t C) { return C % 4 == 0 && ld % 4 == 0 && aligned16(p); }

// what every entry checks after its own strides and pointers: STAG_ENOSYS, or STAG_OK
int check_form(int64_t n_rows, int32_t C) { return (n_rows > kMaxRows || C > kMaxC) ? STAG_ENOSYS : STAG_OK; }

int nll_fwd(bool bernoulli, const float* probs, int64_t ldp, const int64_t* label, const float* y, int64_t ldy,
            int64_t n_rows, int32_t C, const uint8_t* mask, float* value, float* denom, void* workspace,
            size_t workspace_bytes, void* stream) {
  // every decision below is taken before any device work
  if (C <= 0 || n_rows < 0 || ldp < C || (bernoulli && ldy < C)) return STAG_EINVAL;
  if (n_rows > 0 && (!probs || (bernoulli ? !y : !label) || !value || !denom || !workspace)) return STAG_EINVAL;
  if (int rc = check_form(n_rows, C)) return rc;
  if (workspace_bytes < stag_nll_workspace_bytes(n_rows, C)) return STAG_ENOMEM;
  if (n_rows == 0) return STAG_OK;
  NllArgs a{};
  a.p = probs; a.ldp = ldp; a.N = n_rows; a.C = C;
  a.pvec = vec_rows(probs, ldp, C);
  a.label = label;
  a.y = y; a.ldy = ldy;
  a.yvec = bernoulli && vec_rows(y, ldy, C);
  a.mask = mask;
  a.slab = nll_slab_rows(n_rows);
  a.n_slabs = (int32_t)nll_slabs(n_rows);
  a.part = static_cast<NllPartial*>(workspace);
  a.value = value; a.denom = denom;
  return nll_fwd_launch(a, bernoulli, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}

int nll_bwd(bool bernoulli, const float* probs, int64_t ldp, const int64_t* label, const float* y, int64_t ldy,
            int64_t n_rows, int32_t C, const uint8_t* mask, const float* g, const float* denom, float* dprobs,
            int64_t lddp, void* stream) {
  // every decision below is taken before any device work
  if (C <= 0 || n_rows < 0 || ldp < C || (bernoulli && ldy < C) || lddp < C) return STAG_EINVAL;
  if (n_rows > 0 && (!probs || (bernoulli ? !y : !label) || !g || !denom || !dprobs)) return STAG_EINVAL;
  if (int rc = check_form(n_rows, C)) return rc;
  if (n_rows == 0) return STAG_OK;
  NllArgs a{};
  a.p = probs; a.ldp = ldp; a.N = n_rows; a.C = C;
  a.pvec = vec_rows(probs, ldp, C);
  a.label = label;
  a.y = y; a.ldy = ldy;
  a.yvec = bernoulli && vec_rows(y, ldy, C);
  a.mask = mask;
  a.g = g; a.denom_in = denom;
  a.dp = dprobs; a.lddp = lddp;
  a.dvec = vec_rows(dprobs, lddp, C);
  return nll_bwd_launch(a, bernoulli, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}

}  // namespace

extern "C" size_t stag_nll_workspace_bytes(int64_t n_rows, int32_t C) {
  if (n_rows <= 0 || C <= 0) return 0;
  return (size_t)nll_slabs(n_rows) * sizeof(NllPartial);
}

extern "C" int stag_nll_categorical_fwd(const float* probs, int64_t ldp, int64_t n_rows, int32_t C, const int64_t* y,
                                        const uint8_t* mask, float* value, float* denom, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return nll_fwd(false, probs, ldp, y, nullptr, 0, n_rows, C, mask, value, denom, workspace, workspace_bytes, stream);
}

extern "C" int stag_nll_categorical_bwd(const float* probs, int64_t ldp, int64_t n_rows, int32_t C, const int64_t* y,
                                        const uint8_t* mask, const float* g, const float* denom, float* dprobs,
                                        int64_t lddp, void* stream) {
  return nll_bwd(false, probs, ldp, y, nullptr, 0, n_rows, C, mask, g, denom, dprobs, lddp, stream);
}

extern "C" int stag_nll_bernoulli_fwd(const float* probs, int64_t ldp, const float* y, int64_t ldy, int64_t n_rows,
                                      int32_t C, const uint8_t* mask, float* value, float* denom, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return nll_fwd(true, probs, ldp, nullptr, y, ldy, n_rows, C, mask, value, denom, workspace, workspace_bytes, stream);
}

extern "C" int stag_nll_bernoulli_bwd(const float* probs, int64_t ldp, const float* y, int64_t ldy, int64_t n_rows,
                                      int32_t C, const uint8_t* mask, const float* g, const float* denom, float* dprobs,
                                      int64_t lddp, void* stream) {
  return nll_bwd(true, probs, ldp, nullptr, y, ldy, n_rows, C, mask, g, denom, dprobs, lddp, stream);
}
