// node_norm.hip — BatchNorm1d + ReLU + Dropout on node rows [N, D] as fused passes (gfx950): the block every arxiv model
// of the reference puts between its stochastic layers (scripts/arxiv_mle/*/run.py:89-119).
//
//   statistics  mean[k], rstd[k] = 1 / sqrt(var[k] + eps) over the rows (biased var), running buffers      stag_node_norm_stats
//   forward     xhat = (x - mean) * rstd;  pre = xhat * gamma + beta;  y = relu(pre) * m / keep              stag_node_norm_fwd
//   backward    g' = g * m / keep * [pre > 0];  dbeta = sum_n g';  dgamma = sum_n g' * xhat
//               dx = gamma * rstd * (g' - dbeta / N - xhat * dgamma / N)      (batch statistics)
//               dx = gamma * rstd * g'                                         (running statistics)          stag_node_norm_bwd
//
// Every kernel gives a team of LPE lanes a row, 4 channels a lane (16-byte loads when the rows allow it), channels past
// a team's width to further channel tiles (grid.y), and keeps kRows rows of a team in flight.  Rows take 64-bit
// addresses.  The mask m[n, k] is draw4<kBernoulli> at position n, chunk k / 4: the field stag_noise_materialize writes
// for a Bernoulli spec on the N-edge identity graph.  The backward draws it again and forms xhat and pre again from x
// and the four [D] vectors, with the forward's own operations (pre4 below; the build contracts nothing), so a ReLU
// decision is the same bit in all three passes and nothing [N, D]-sized but x is kept between them.
//
// The column reductions (statistics; the backward's two sums) are two launches each.  A workgroup takes a slab of
// node_slab_rows(N) rows: team t sums rows t, t + T, ... of it per lane, the teams' sums are added in team order through
// LDS, and one partial per channel goes to the workspace.  A second small launch merges the partials of 8 runs of
// consecutive slabs in slab order, then the 8 runs in order.  No atomics, no arrival counters: the result is a function
// of (N, D, the data) alone and two launches give the same bits.
// The statistics partial of a slab is (mean, M2) from the sums of x - K and (x - K)^2 with K the slab's first row, and
// partials merge by Chan's formula: a column whose mean is far from 0 keeps its variance (E[x^2] - mean^2 loses it).
// The backward's sums are plain sums per slab, Kahan-compensated across the slabs.
#include "node_norm.hpp"
#include "agg_kernel.hpp"   // load4 / store4
#include "entry_args.hpp"

namespace stag {
namespace {

constexpr int kRows = 4;           // rows whose loads a team has in flight together
constexpr int kMergeCh = 32;       // a merge workgroup: 32 channels x 8 runs of slabs
constexpr int kMergeRuns = 256 / kMergeCh;

// the lane's 4 channels of the four [D] vectors (a channel past D: zeros, never stored)
struct Chan4 {
  float mean[4], rstd[4], gamma[4], beta[4];
};

__device__ __forceinline__ void load_chan(const NodeMapArgs& m, int k0, Chan4& c) {
  load4(m.mean, k0, m.D, false, c.mean);
  load4(m.rstd, k0, m.D, false, c.rstd);
#pragma unroll
  for (int j = 0; j < 4; ++j) { c.gamma[j] = 1.0f; c.beta[j] = 0.0f; }
  if (m.gamma) load4(m.gamma, k0, m.D, false, c.gamma);
  if (m.beta) load4(m.beta, k0, m.D, false, c.beta);
}

// the one definition of xhat and pre: forward, column sums and dx pass form the same bits
__device__ __forceinline__ void pre4(const Chan4& c, const float (&x)[4], float (&xhat)[4], float (&pre)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    xhat[j] = (x[j] - c.mean[j]) * c.rstd[j];
    pre[j] = xhat[j] * c.gamma[j] + c.beta[j];
  }
}

// m / keep of the lane's 4 channels of `row`
__device__ __forceinline__ void keep4(const NodeMapArgs& m, const PhiloxKey& key, int64_t row, uint32_t chunk,
                                      float (&f)[4]) {
  if (!m.drop) {
    f[0] = f[1] = f[2] = f[3] = 1.0f;
    return;
  }
  const float p[4] = {m.keep, m.keep, m.keep, m.keep};
  float w[4];
  draw4<kBernoulli>((uint32_t)row, ctr1_of(row, chunk), key, p, p, 0, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = w[j] * m.inv_keep;
}

// g' = g * m / keep * [pre > 0] and xhat of the lane's 4 channels of `row`
__device__ __forceinline__ void gprime4(const NodeMapArgs& m, const Chan4& c, const PhiloxKey& key, int64_t row,
                                        uint32_t chunk, const float (&x)[4], const float (&g)[4], float (&xhat)[4],
                                        float (&gp)[4]) {
  float pre[4], f[4];
  pre4(c, x, xhat, pre);
  keep4(m, key, row, chunk, f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gp[j] = g[j] * f[j];
    if (m.relu && !(pre[j] > 0.0f)) gp[j] = 0.0f;
  }
}

__device__ __forceinline__ PhiloxKey key_of(const NodeMapArgs& m) { return m.drop ? resolve_epoch(m.key) : m.key; }

// the sums of the workgroup's teams, in team order, into team 0's lanes (every thread of the workgroup calls this)
template <int LPE>
__device__ __forceinline__ void team_fold(float (&sm)[2][1024], float (&a)[4], float (&b)[4]) {
  constexpr int T = 256 / LPE;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sm[0][threadIdx.x * 4 + j] = a[j];
    sm[1][threadIdx.x * 4 + j] = b[j];
  }
  __syncthreads();
  if (threadIdx.x >= LPE) return;
  for (int t = 1; t < T; ++t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] += sm[0][(t * LPE + threadIdx.x) * 4 + j];
      b[j] += sm[1][(t * LPE + threadIdx.x) * 4 + j];
    }
  }
}

// ---- statistics ------------------------------------------------------------------------------------------------------
template <int LPE>
__global__ __launch_bounds__(256) void node_stats_kernel(const NodeStatsArgs a) {
  constexpr int T = 256 / LPE;
  __shared__ float sm[2][1024];
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const int k0 = 4 * (blockIdx.y * LPE + lane);
  const bool live = k0 < a.D;                  // (a lane without channels still meets the others at the barrier)
  const bool xv = a.xvec != 0;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = min(r0 + a.slab, a.N);
  float K[4] = {0.f, 0.f, 0.f, 0.f};           // the shift: the slab's first row
  if (live) load4(a.x + r0 * a.ldx, k0, a.D, xv, K);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    for (int64_t r = r0 + team; r < r1; r += (int64_t)kRows * T) {
      float v[kRows][4];
#pragma unroll
      for (int j = 0; j < kRows; ++j)
        if (r + j * T < r1) load4(a.x + (r + j * T) * a.ldx, k0, a.D, xv, v[j]);
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (r + j * T < r1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float d = v[j][c] - K[c];
            s1[c] += d;
            s2[c] += d * d;
          }
        }
      }
    }
  }
  team_fold<LPE>(sm, s1, s2);
  if (team != 0 || !live) return;
  const float n = (float)(r1 - r0);
  float mean[4], m2[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mean[c] = K[c] + s1[c] / n;
    const float t = s2[c] - s1[c] * s1[c] / n;
    m2[c] = t < 0.0f ? 0.0f : t;               // (a NaN stays one)
  }
  float* p = a.part + (int64_t)blockIdx.x * 2 * a.D;
  store4(p, k0, a.D, false, mean);
  store4(p + a.D, k0, a.D, false, m2);
}

// (n, mean, M2) of a run of rows, with the (nb, mb, Mb) of the rows behind it (Chan et al.)
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.0f) return;
  if (na == 0.0f) { na = nb; ma = mb; Ma = Mb; return; }
  const float n = na + nb, d = mb - ma, w = nb / n;
  ma += d * w;
  Ma += Mb + d * d * (na * w);
  na = n;
}

__global__ __launch_bounds__(256) void node_stats_merge_kernel(const NodeStatsArgs a) {
  __shared__ float sh[3][kMergeRuns][kMergeCh];
  const int c = threadIdx.x % kMergeCh, run = threadIdx.x / kMergeCh;
  const int k = blockIdx.x * kMergeCh + c;
  const int per = (a.n_slabs + kMergeRuns - 1) / kMergeRuns;
  const int s0 = min(run * per, a.n_slabs), s1 = min(s0 + per, a.n_slabs);
  float n = 0.0f, mean = 0.0f, m2 = 0.0f;
  if (k < a.D) {
    for (int s = s0; s < s1; ++s) {
      const float* p = a.part + (int64_t)s * 2 * a.D;
      const float nb = (float)min(a.slab, a.N - (int64_t)s * a.slab);
      chan_merge(n, mean, m2, nb, p[k], p[a.D + k]);
    }
  }
  sh[0][run][c] = n; sh[1][run][c] = mean; sh[2][run][c] = m2;
  __syncthreads();
  if (run != 0 || k >= a.D) return;
  for (int r = 1; r < kMergeRuns; ++r) chan_merge(n, mean, m2, sh[0][r][c], sh[1][r][c], sh[2][r][c]);
  const float N = (float)a.N;
  a.mean_out[k] = mean;
  a.rstd_out[k] = 1.0f / sqrtf(m2 / N + a.eps);
  if (a.running_mean) a.running_mean[k] = (1.0f - a.factor) * a.running_mean[k] + a.factor * mean;
  // the unbiased variance (torch.nn.BatchNorm1d); one row has none, and its buffer takes the biased 0
  if (a.running_var) a.running_var[k] = (1.0f - a.factor) * a.running_var[k] + a.factor * (m2 / (a.N > 1 ? N - 1.0f : 1.0f));
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int LPE>
__global__ __launch_bounds__(256) void node_fwd_kernel(const NodeFwdArgs a) {
  constexpr int T = 256 / LPE;
  const NodeMapArgs& m = a.m;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const uint32_t chunk = blockIdx.y * LPE + lane;
  const int k0 = 4 * (int)chunk;
  if (k0 >= m.D) return;
  const int64_t r0 = (int64_t)blockIdx.x * (T * kRows) + team;
  const bool xv = m.xvec != 0;
  Chan4 c;
  load_chan(m, k0, c);
  const PhiloxKey key = key_of(m);
  float v[kRows][4];
#pragma unroll
  for (int j = 0; j < kRows; ++j)
    if (r0 + j * T < m.N) load4(m.x + (r0 + j * T) * m.ldx, k0, m.D, xv, v[j]);
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int64_t r = r0 + j * T;
    if (r < m.N) {
      float xhat[4], pre[4], f[4], y[4];
      pre4(c, v[j], xhat, pre);
      keep4(m, key, r, chunk, f);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float t = (m.relu && pre[q] <= 0.0f) ? 0.0f : pre[q];   // (a NaN stays one, as torch's relu keeps it)
        y[q] = t * f[q];
      }
      store4(a.y + r * a.ldy, k0, m.D, a.yvec != 0, y);
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <int LPE>
__global__ __launch_bounds__(256) void node_bsum_kernel(const NodeBwdArgs a) {
  constexpr int T = 256 / LPE;
  __shared__ float sm[2][1024];
  const NodeMapArgs& m = a.m;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const uint32_t chunk = blockIdx.y * LPE + lane;
  const int k0 = 4 * (int)chunk;
  const bool live = k0 < m.D;
  const bool xv = m.xvec != 0, gv = a.gvec != 0;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = min(r0 + a.slab, m.N);
  float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    Chan4 c;
    load_chan(m, k0, c);
    const PhiloxKey key = key_of(m);
    for (int64_t r = r0 + team; r < r1; r += (int64_t)kRows * T) {
      float v[kRows][4], g[kRows][4];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (r + j * T < r1) {
          load4(m.x + (r + j * T) * m.ldx, k0, m.D, xv, v[j]);
          load4(a.g + (r + j * T) * a.ldg, k0, m.D, gv, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (r + j * T < r1) {
          float xhat[4], gp[4];
          gprime4(m, c, key, r + j * T, chunk, v[j], g[j], xhat, gp);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            sb[q] += gp[q];
            sg[q] += gp[q] * xhat[q];
          }
        }
      }
    }
  }
  team_fold<LPE>(sm, sb, sg);
  if (team != 0 || !live) return;
  float* p = a.part + (int64_t)blockIdx.x * 2 * m.D;
  store4(p, k0, m.D, false, sb);
  store4(p + m.D, k0, m.D, false, sg);
}

__device__ __forceinline__ void kahan_add(float& sum, float& comp, float v) {
  const float y = v - comp;
  const float t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}

__global__ __launch_bounds__(256) void node_bsum_merge_kernel(const NodeBwdArgs a) {
  __shared__ float sh[4][kMergeRuns][kMergeCh];
  const int D = a.m.D;
  const int c = threadIdx.x % kMergeCh, run = threadIdx.x / kMergeCh;
  const int k = blockIdx.x * kMergeCh + c;
  const int per = (a.n_slabs + kMergeRuns - 1) / kMergeRuns;
  const int s0 = min(run * per, a.n_slabs), s1 = min(s0 + per, a.n_slabs);
  float sum[2] = {0.f, 0.f}, comp[2] = {0.f, 0.f};
  if (k < D) {
    for (int s = s0; s < s1; ++s) {
      const float* p = a.part + (int64_t)s * 2 * D;
      kahan_add(sum[0], comp[0], p[k]);
      kahan_add(sum[1], comp[1], p[D + k]);
    }
  }
  sh[0][run][c] = sum[0]; sh[1][run][c] = comp[0]; sh[2][run][c] = sum[1]; sh[3][run][c] = comp[1];
  __syncthreads();
  if (run != 0 || k >= D) return;
  for (int r = 1; r < kMergeRuns; ++r) {
    kahan_add(sum[0], comp[0], sh[0][r][c]);
    kahan_add(sum[0], comp[0], -sh[1][r][c]);
    kahan_add(sum[1], comp[1], sh[2][r][c]);
    kahan_add(sum[1], comp[1], -sh[3][r][c]);
  }
  a.sums[k] = sum[0];
  a.sums[D + k] = sum[1];
  if (a.dbeta) a.dbeta[k] = sum[0];
  if (a.dgamma) a.dgamma[k] = sum[1];
}

template <int LPE>
__global__ __launch_bounds__(256) void node_dx_kernel(const NodeBwdArgs a) {
  constexpr int T = 256 / LPE;
  const NodeMapArgs& m = a.m;
  const int lane = threadIdx.x % LPE, team = threadIdx.x / LPE;
  const uint32_t chunk = blockIdx.y * LPE + lane;
  const int k0 = 4 * (int)chunk;
  if (k0 >= m.D) return;
  const int64_t r0 = (int64_t)blockIdx.x * (T * kRows) + team;
  const bool xv = m.xvec != 0, gv = a.gvec != 0;
  Chan4 c;
  load_chan(m, k0, c);
  float mb[4] = {0.f, 0.f, 0.f, 0.f}, mg[4] = {0.f, 0.f, 0.f, 0.f}, scale[4];
  if (a.batch_stats) {
    const float n = (float)m.N;
    load4(a.sums, k0, m.D, false, mb);
    load4(a.sums + m.D, k0, m.D, false, mg);
#pragma unroll
    for (int q = 0; q < 4; ++q) { mb[q] = mb[q] / n; mg[q] = mg[q] / n; }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) scale[q] = c.gamma[q] * c.rstd[q];
  const PhiloxKey key = key_of(m);
  float v[kRows][4], g[kRows][4];
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    if (r0 + j * T < m.N) {
      load4(m.x + (r0 + j * T) * m.ldx, k0, m.D, xv, v[j]);
      load4(a.g + (r0 + j * T) * a.ldg, k0, m.D, gv, g[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int64_t r = r0 + j * T;
    if (r < m.N) {
      float xhat[4], gp[4], d[4];
      gprime4(m, c, key, r, chunk, v[j], g[j], xhat, gp);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = a.batch_stats ? scale[q] * (gp[q] - mb[q] - xhat[q] * mg[q]) : scale[q] * gp[q];
      store4(a.dx + r * a.lddx, k0, m.D, a.dvec != 0, d);
    }
  }
}

// lanes per row and channel tiles (grid.y) of a width
struct Shape {
  int lpe;
  unsigned tiles;
};
Shape shape_of(int32_t D) {
  const int nchunk = (D + 3) / 4;
  const int lpe = lanes_for(nchunk, 4);
  return {lpe, (unsigned)((nchunk + lpe - 1) / lpe)};
}

}  // namespace

hipError_t node_stats_launch(const NodeStatsArgs& a, hipStream_t s) {
  const Shape sh = shape_of(a.D);
  pick<64, 32, 16, 8, 4>(sh.lpe, [&](auto L) {
    hipLaunchKernelGGL((node_stats_kernel<decltype(L)::value>), dim3((unsigned)a.n_slabs, sh.tiles), dim3(256), 0, s, a);
  });
  hipLaunchKernelGGL(node_stats_merge_kernel, dim3((a.D + kMergeCh - 1) / kMergeCh), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t node_fwd_launch(const NodeFwdArgs& a, hipStream_t s) {
  const Shape sh = shape_of(a.m.D);
  const int64_t per_block = (256 / sh.lpe) * kRows;
  const dim3 grid((unsigned)((a.m.N + per_block - 1) / per_block), sh.tiles);
  pick<64, 32, 16, 8, 4>(sh.lpe, [&](auto L) {
    hipLaunchKernelGGL((node_fwd_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
  });
  return hipGetLastError();
}

hipError_t node_bwd_launch(const NodeBwdArgs& a, bool want_sums, bool want_dx, hipStream_t s) {
  const Shape sh = shape_of(a.m.D);
  if (want_sums) {
    pick<64, 32, 16, 8, 4>(sh.lpe, [&](auto L) {
      hipLaunchKernelGGL((node_bsum_kernel<decltype(L)::value>), dim3((unsigned)a.n_slabs, sh.tiles), dim3(256), 0, s, a);
    });
    hipLaunchKernelGGL(node_bsum_merge_kernel, dim3((a.m.D + kMergeCh - 1) / kMergeCh), dim3(256), 0, s, a);
  }
  if (want_dx) {
    const int64_t per_block = (256 / sh.lpe) * kRows;
    const dim3 grid((unsigned)((a.m.N + per_block - 1) / per_block), sh.tiles);
    pick<64, 32, 16, 8, 4>(sh.lpe, [&](auto L) {
      hipLaunchKernelGGL((node_dx_kernel<decltype(L)::value>), grid, dim3(256), 0, s, a);
    });
  }
  return hipGetLastError();
}

}  // namespace stag

using namespace stag;

namespace {

constexpr int64_t kMaxRows = 1ll << 34;      // the row groups of a launch fill grid.x below 2^31
constexpr int64_t kMaxChunks = 1ll << 20;    // the chunk field of the counter word; the channel tiles fill grid.y below 2^16

bool vec_rows(const void* p, int64_t ld, int32_t D) { return D % 4 == 0 && ld % 4 == 0 && aligned16(p); }

// what every entry checks of its rows and its drop record before anything else: STAG_EINVAL, or STAG_OK
int check_shape(int64_t n_rows, int32_t D, const stag_node_drop* drop) {
  if (D <= 0 || n_rows < 0) return STAG_EINVAL;
  if (drop) {
    if (!(drop->keep_prob > 0.0f && drop->keep_prob <= 1.0f)) return STAG_EINVAL;
    if (!counter_space_ok(0, n_rows, 0, ((int64_t)D + 3) / 4)) return STAG_EINVAL;
  }
  return STAG_OK;
}

int check_form(int64_t n_rows, int32_t D) {
  return (n_rows > kMaxRows || ((int64_t)D + 3) / 4 > kMaxChunks) ? STAG_ENOSYS : STAG_OK;
}

void fill_map(NodeMapArgs& m, const float* x, int64_t ldx, int64_t n_rows, int32_t D, const float* mean, const float* rstd,
              const float* gamma, const float* beta, int32_t relu, const stag_node_drop* drop) {
  m.x = x; m.ldx = ldx; m.N = n_rows; m.D = D;
  m.xvec = vec_rows(x, ldx, D);
  m.mean = mean; m.rstd = rstd; m.gamma = gamma; m.beta = beta;
  m.relu = relu != 0;
  m.drop = drop && drop->keep_prob < 1.0f;
  m.keep = m.drop ? drop->keep_prob : 1.0f;
  m.inv_keep = 1.0f / m.keep;
  m.key = m.drop ? make_key(drop->seed, drop->offset, drop->epoch) : PhiloxKey{};
}

}  // namespace

extern "C" size_t stag_node_norm_workspace_bytes(int64_t n_rows, int32_t D) {
  if (n_rows <= 0 || D <= 0) return 0;
  return (size_t)(node_slabs(n_rows) + 1) * 2u * (size_t)D * sizeof(float);
}

extern "C" int stag_node_norm_stats(const float* x, int64_t ldx, int64_t n_rows, int32_t D, float eps, float* mean_out,
                                    float* rstd_out, float* running_mean, float* running_var, float momentum_factor,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  // every decision below is taken before any device work
  int rc = check_shape(n_rows, D, nullptr);
  if (rc) return rc;
  if (ldx < D || !(eps > 0.0f) || !std::isfinite(eps)) return STAG_EINVAL;
  if ((running_mean || running_var) && !std::isfinite(momentum_factor)) return STAG_EINVAL;
  if (n_rows == 0) return STAG_OK;
  if (!x || !mean_out || !rstd_out || !workspace) return STAG_EINVAL;
  if ((rc = check_form(n_rows, D))) return rc;
  if (workspace_bytes < stag_node_norm_workspace_bytes(n_rows, D)) return STAG_ENOMEM;
  NodeStatsArgs a{};
  a.x = x; a.ldx = ldx; a.N = n_rows; a.slab = node_slab_rows(n_rows); a.D = D;
  a.xvec = vec_rows(x, ldx, D);
  a.part = static_cast<float*>(workspace) + 2 * (size_t)D;
  a.n_slabs = (int32_t)node_slabs(n_rows);
  a.eps = eps;
  a.mean_out = mean_out; a.rstd_out = rstd_out;
  a.running_mean = running_mean; a.running_var = running_var; a.factor = momentum_factor;
  return node_stats_launch(a, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_node_norm_fwd(const float* x, int64_t ldx, int64_t n_rows, int32_t D, const float* mean,
                                  const float* rstd, const float* gamma, const float* beta, int32_t relu,
                                  const stag_node_drop* drop, float* y, int64_t ldy, void* stream) {
  // every decision below is taken before any device work
  int rc = check_shape(n_rows, D, drop);
  if (rc) return rc;
  if (ldx < D || ldy < D) return STAG_EINVAL;
  if (n_rows == 0) return STAG_OK;
  if (!x || !mean || !rstd || !y) return STAG_EINVAL;
  if ((rc = check_form(n_rows, D))) return rc;
  NodeFwdArgs a{};
  fill_map(a.m, x, ldx, n_rows, D, mean, rstd, gamma, beta, relu, drop);
  a.y = y; a.ldy = ldy;
  a.yvec = vec_rows(y, ldy, D);
  return node_fwd_launch(a, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}

extern "C" int stag_node_norm_bwd(const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t n_rows, int32_t D,
                                  const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  int32_t relu, const stag_node_drop* drop, int32_t batch_stats, float* dx, int64_t lddx,
                                  float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  // every decision below is taken before any device work
  int rc = check_shape(n_rows, D, drop);
  if (rc) return rc;
  if (ldx < D || ldg < D || (dx && lddx < D)) return STAG_EINVAL;
  if (n_rows == 0) return STAG_OK;
  const bool want_sums = (dx && batch_stats) || dgamma || dbeta;
  if (!x || !g || !mean || !rstd || (want_sums && !workspace)) return STAG_EINVAL;
  if ((rc = check_form(n_rows, D))) return rc;
  if (want_sums && workspace_bytes < stag_node_norm_workspace_bytes(n_rows, D)) return STAG_ENOMEM;
  if (!dx && !want_sums) return STAG_OK;
  NodeBwdArgs a{};
  fill_map(a.m, x, ldx, n_rows, D, mean, rstd, gamma, beta, relu, drop);
  a.g = g; a.ldg = ldg;
  a.gvec = vec_rows(g, ldg, D);
  a.slab = node_slab_rows(n_rows);
  a.n_slabs = (int32_t)node_slabs(n_rows);
  a.batch_stats = batch_stats != 0;
  a.sums = static_cast<float*>(workspace);
  a.part = a.sums ? a.sums + 2 * (size_t)D : nullptr;
  a.dbeta = dbeta; a.dgamma = dgamma;
  a.dx = dx; a.lddx = lddx;
  a.dvec = dx && vec_rows(dx, lddx, D);
  return node_bwd_launch(a, want_sums, dx != nullptr, (hipStream_t)stream) == hipSuccess ? STAG_OK : STAG_EIO;
}
