// Launchers of the Normal policy-head kernels in normal_policy.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kNormalMaxActions = 256;     // a row in one wave64: 4 values per lane
constexpr int kNormalMaxBlocks = 2048;     // the grid's cap, 4 waves per workgroup; more rows: grid stride

constexpr int kNormalBounded = 0;          // mean = tanh(m), std = (hi - lo) sigmoid(s + 2) + lo   (heads.py:146-155)
constexpr int kNormalLogstd = 1;           // mean = m,       std = exp(s)                           (heads.py:157-162)

// mean_raw, std_raw: (N, T, A), float32 or bfloat16, both the same (arithmetic in
// float32); act: (N, T, A) float32, or null (no action: logpi = 0).  Per element
//   z = (act - mean) / std,  logp_a = -z^2 / 2 - log(std) - log(2 pi) / 2     (outs.py:174-176)
//   ent_a = log(2 pi std^2) / 2 + 1 / 2                                      (outs.py:178-179)
// and per output row r = (n, t), t < T - drop, read at the inputs' row n * T + t and
// summed over the A action dimensions in an order A alone fixes (outs.py:63-64,
// 69-71; dreamerv3/agent.py:411-414):
//   logpi = sum_a logp_a,  ent = sum_a ent_a
//   loss  = weight[n * weight_stride + t] * -(logpi * adv[r] + actent * ent)
// adv (N, T - drop) and weight may be null: 1.  loss, logpi and ent may each be
// null (not written), not all three.  drop is 0 or 1: the last step of every n is
// not read.  A NaN in m, s or act makes the row's three outputs NaN.  N, T - drop
// >= 1, 1 <= A <= kNormalMaxActions, N * T * A <= 2^31 - 1, weight_stride >= T - drop,
// and for kNormalBounded hi >= lo > 0 (refused otherwise).
hipError_t launch_normal_policy_loss(const void* mean_raw, const void* std_raw, const float* act, bool bf16, int64_t N,
                                     int64_t T, int64_t drop, int64_t A, int kind, float lo, float hi, float actent,
                                     const float* adv, const float* weight, int64_t weight_stride, float* loss,
                                     float* logpi, float* ent, hipStream_t stream);

// grad_mean, grad_std (N, T, A) in the inputs' dtype, rounded once at the store:
// gout[r] * d loss[r] / d (m, s), the closed form from one more read of the inputs
//   d loss / d m_a = -w g adv (z / std) dmean/dm
//   d loss / d s_a = -w g (adv (z^2 - 1) + actent) / std dstd/ds
// with dmean/dm = 1 - tanh^2(m) formed from exp(-2 |m|) (no difference of two
// numbers near 1) and dstd/ds = (hi - lo) sigmoid(s + 2) sigmoid(-(s + 2)), or 1
// and std for kNormalLogstd.  The rows of a dropped step are written as zeros; a
// row with a NaN in m, s or act is NaN throughout.  Here T - drop may be 0.
hipError_t launch_normal_policy_loss_grad(const void* mean_raw, const void* std_raw, const float* act, bool bf16,
                                          int64_t N, int64_t T, int64_t drop, int64_t A, int kind, float lo, float hi,
                                          float actent, const float* adv, const float* weight, int64_t weight_stride,
                                          const float* gout, void* grad_mean, void* grad_std, hipStream_t stream);

// The stream every draw comes from: element e takes the Philox4x32-10 block at
// counter (e, offset) under key seed (philox.h, the keying of onehot_sample.h):
//   u1 = ((word0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (word1 >> 8) * 2^-24 in [0, 1)
//   eps = sqrt(-2 ln u1) cos(2 pi u2)                                        (Box-Muller)
// out[i] = eps(seed, offset, first + i) for i < count, float32.  count >= 1.
hipError_t launch_philox_normal(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, float* out,
                                hipStream_t stream);

// act[e] = mean_e + std_e * eps_e (outs.py:170-172) for the rows * A elements e,
// float32; eps is the caller's (rows, A) float32 or, if null, the draw above at
// e = row * A + a.  rows >= 1, A >= 1, rows * A <= 2^31 - 1.
hipError_t launch_normal_sample(const void* mean_raw, const void* std_raw, bool bf16, int64_t rows, int64_t A, int kind,
                                float lo, float hi, uint64_t seed, uint64_t offset, const float* eps, float* act,
                                hipStream_t stream);

// Kernel launches the four launchers have issued in this process.
int64_t normal_policy_launches();

}  // namespace emb
