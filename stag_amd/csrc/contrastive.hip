// Contrastive NLL of amortised edge noise (include/stag_hip.h: stag_contrastive_nll; stag/models.py:7-25).
//
// What the reference computes for AmortizedDistribution(in, 1) over a Normal: with E uniformly drawn fake edges
//     h'    = SiLU(W_e [feat[fake_src] || feat[fake_dst]] + b_e)          [E, hidden]   (an [E, 2 in] concatenation)
//     m', l' = W_loc h' + b_loc,  W_ls h' + b_ls                          [E, 1] each
//     nll   = (-N(loc, exp(log_scale)).log_prob(1) - N(m', exp(l')).log_prob(0)).sum(-1).mean()
// The MLP is the one of stag_edge_mlp_fwd on other endpoints (the concatenation is a sum of two projected rows, amort.hip)
// and the log-density is closed-form, so a thread per edge id forms its term in registers: no [E, 2 in] tensor, no
// [E, hidden] activation, no [E, 1] intermediates.  The same pass writes every gradient of the mean.
// Reduction: per-thread fp32 sums over a fixed edge walk -> wave butterfly -> the block's four waves in order -> one
// partial per block; a second launch adds the partials in index order, in double.  No atomics: bit-identical from run
// to run.
#include <hip/hip_runtime.h>

#include "../../include/stag_hip.h"
#include "entry_args.hpp"

using stag::pick;

namespace {

constexpr int kRedBlocks = 512;     // first-stage blocks (amort.hip's)
constexpr int kMaxHidden = 8;
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// (the three helpers below repeat amort.hip's: that unit's objects stay as they are)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

inline int ht_for(int h) { return h <= 1 ? 1 : h <= 2 ? 2 : h <= 4 ? 4 : 8; }

// values of a block partial: [0] the sum of the terms, [1 + 2 j + p] d wh[j, p], [1 + 2 HT + p] d bh[p]
constexpr int nv_for(int ht) { return 2 * ht + 3; }

struct ContrastiveArgs {
  const float* loc; const float* ls; int64_t E;
  const int32_t* fsrc; const int32_t* fdst;
  const float* ps; const float* pd; int ldp; int hidden;
  const float* wh; const float* bh;
  float pos, neg, inv_e;
  float* dloc; float* dls; float* dpre;
  float* part;
};

// thread i of the grid walks edge ids i, i + total, ... (fixed); GRAD: the head sums and the per-edge gradients too.
// The value's arithmetic is the same instruction sequence with and without GRAD.
template <int HT, bool GRAD>
__global__ __launch_bounds__(256) void contrastive_nll_kernel(const ContrastiveArgs a) {
  constexpr int NV = nv_for(HT), NA = GRAD ? NV : 1;
  __shared__ float s_w[4][NA];
  float acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.f;
  float w0[HT], w1[HT];
#pragma unroll
  for (int j = 0; j < HT; ++j) {
    w0[j] = j < a.hidden ? a.wh[j * 2] : 0.f;
    w1[j] = j < a.hidden ? a.wh[j * 2 + 1] : 0.f;
  }
  const float b0 = a.bh ? a.bh[0] : 0.f, b1 = a.bh ? a.bh[1] : 0.f;
  const int64_t total = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.E; e += total) {
    const int u = a.fsrc[e], v = a.fdst[e];
    const float m = a.loc[e], l = a.ls[e];
    float pre[HT], sg[HT], h[HT];
    float mf = b0, lf = b1;
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      pre[j] = sg[j] = h[j] = 0.f;
      if (j < a.hidden) {
        pre[j] = a.ps[(int64_t)u * a.ldp + j] + a.pd[(int64_t)v * a.ldp + j];
        sg[j] = sigmoidf(pre[j]);
        h[j] = pre[j] * sg[j];
        mf = __builtin_fmaf(h[j], w0[j], mf);
        lf = __builtin_fmaf(h[j], w1[j], lf);
      }
    }
    // nlp(v; m, l) = 0.5 ((v - m) exp(-l))^2 + l + 0.5 log(2 pi)
    const float ir = expf(-l), irf = expf(-lf);
    const float zr = (a.pos - m) * ir, zf = (a.neg - mf) * irf;
    acc[0] += ((0.5f * (zr * zr) + l) + kHalfLog2Pi) + ((0.5f * (zf * zf) + lf) + kHalfLog2Pi);
    if constexpr (GRAD) {
      if (a.dloc) a.dloc[e] = -(zr * ir) * a.inv_e;
      if (a.dls) a.dls[e] = (1.0f - zr * zr) * a.inv_e;
      const float g0 = -(zf * irf), g1 = 1.0f - zf * zf;        // d term / d m', d l' (1 / E joins at the stores)
      acc[NA - 2] += g0;
      acc[NA - 1] += g1;
#pragma unroll
      for (int j = 0; j < HT; ++j) {
        if (j < a.hidden) {
          acc[1 + 2 * j] = __builtin_fmaf(h[j], g0, acc[1 + 2 * j]);
          acc[2 + 2 * j] = __builtin_fmaf(h[j], g1, acc[2 + 2 * j]);
          if (a.dpre) {
            const float dh = __builtin_fmaf(g1, w1[j], g0 * w0[j]);
            a.dpre[e * a.hidden + j] = (dh * (sg[j] * (1.0f + pre[j] * (1.0f - sg[j])))) * a.inv_e;     // SiLU'(pre)
          }
        }
      }
    }
  }
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const float s = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) s_w[wv][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NA) {
    const float s = (s_w[0][threadIdx.x] + s_w[1][threadIdx.x]) + (s_w[2][threadIdx.x] + s_w[3][threadIdx.x]);
    a.part[(int64_t)blockIdx.x * NV + threadIdx.x] = s;
  }
}

// block i owns value i of the partials [nb][nv]: thread t adds partials [t nb / 256, (t + 1) nb / 256) in index order,
// thread 0 the 256 shares in thread order, all in double; times 1 / n_edges
__global__ __launch_bounds__(256) void contrastive_final_kernel(const float* part, int nb, int nv, int hidden,
                                                                double inv_e, float* nll_mean, float* dwh,
                                                                float* dbh) {
  __shared__ double red[256];
  const int i = blockIdx.x, ht = (nv - 3) / 2;
  const int lo = (int)((int64_t)threadIdx.x * nb / 256), hi = (int)((int64_t)(threadIdx.x + 1) * nb / 256);
  double s = 0.0;
  for (int b = lo; b < hi; ++b) s += (double)part[(int64_t)b * nv + i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot = 0.0;
  for (int t = 0; t < 256; ++t) tot += red[t];
  const float r = (float)(tot * inv_e);
  if (i == 0) { nll_mean[0] = r; return; }
  const int k = i - 1;
  if (k < 2 * ht) { if (dwh && k / 2 < hidden) dwh[k] = r; }
  else if (dbh) dbh[k - 2 * ht] = r;
}

}  // namespace

extern "C" {

size_t stag_contrastive_nll_workspace_bytes(int32_t hidden) {
  if (hidden <= 0 || hidden > kMaxHidden) return 0;
  return (size_t)kRedBlocks * (size_t)nv_for(ht_for(hidden)) * sizeof(float);
}

int stag_contrastive_nll(const float* loc, const float* log_scale, int64_t n_edges, const int32_t* fake_src,
                         const int32_t* fake_dst, const float* ps, const float* pd, int64_t ldp, int32_t hidden,
                         const float* wh, const float* bh, float pos_value, float neg_value, float* nll_mean,
                         float* dloc, float* dlog_scale, float* dpre, float* dwh, float* dbh, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (n_edges <= 0 || hidden <= 0 || hidden > kMaxHidden || ldp < hidden || ldp >= (1 << 30)) return STAG_EINVAL;
  if (!loc || !log_scale || !fake_src || !fake_dst || !ps || !pd || !wh || !nll_mean) return STAG_EINVAL;
  if (!workspace || workspace_bytes < stag_contrastive_nll_workspace_bytes(hidden)) return STAG_ENOMEM;
  const int ht = ht_for(hidden), nv = nv_for(ht);
  const bool grad = dloc || dlog_scale || dpre || dwh || dbh;
  ContrastiveArgs a;
  a.loc = loc; a.ls = log_scale; a.E = n_edges;
  a.fsrc = fake_src; a.fdst = fake_dst;
  a.ps = ps; a.pd = pd; a.ldp = (int)ldp; a.hidden = hidden;
  a.wh = wh; a.bh = bh;
  a.pos = pos_value; a.neg = neg_value; a.inv_e = (float)(1.0 / (double)n_edges);
  a.dloc = dloc; a.dls = dlog_scale; a.dpre = dpre;
  a.part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  // the rung is (ht, grad) as one number, 2 ht + grad; the last of them, <8, true>, is the default
  pick<2, 3, 4, 5, 8, 9, 16, 17>(2 * ht + (grad ? 1 : 0), [&](auto R) {
    constexpr int r = decltype(R)::value;
    hipLaunchKernelGGL((contrastive_nll_kernel<r / 2, (r & 1) != 0>), dim3(kRedBlocks), dim3(256), 0, s, a);
  });
  // block 0: the value; blocks 1 ...: the head gradients (only when one of them is asked for)
  hipLaunchKernelGGL(contrastive_final_kernel, dim3((dwh || dbh) ? nv : 1), dim3(256), 0, s, a.part, kRedBlocks, nv,
                     hidden, 1.0 / (double)n_edges, nll_mean, dwh, dbh);
  return hipGetLastError() == hipSuccess ? STAG_OK : STAG_EIO;
}

}  // extern "C"
