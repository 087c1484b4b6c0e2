// Launchers of the TwoHot head's kernels in twohot.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kTwoHotMaxBins = 1024;       // a row in registers: 16 values per lane of a wave64
constexpr int kTwoHotMaxTargets = 4;

// The targets of one loss_sum: k device arrays of `rows` float32 and their
// coefficients.  Travels by value into the kernels.
struct TwoHotTargets {
  const float* target[kTwoHotMaxTargets];
  float coef[kTwoHotMaxTargets];
  int32_t k;
};

// Per row of `logits` (rows, n), float32 or bfloat16 (arithmetic in float32):
// lse = max + log(sum(exp(x - max))) and pred = the symmetric weighted average of
// embodied/jax/outs.py:285-309 over softmax(x) = exp(x - max) / sum.
// rows >= 1, 1 <= n <= kTwoHotMaxBins, rows * n <= 2^31 - 1 (refused otherwise).
hipError_t launch_twohot_stats(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                               float* lse, float* pred, hipStream_t stream);

// loss[r] = sum_k coef[k] * -(w_below * (x[below] - lse) + w_above * (x[above] - lse)),
// the terms added in the order of k; below, above and the weights as outs.py:314-324.
hipError_t launch_twohot_loss(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                              const float* lse, const TwoHotTargets& targets, float* loss, hipStream_t stream);

// grad[r, i] = gout[r] * (sum(coef) * exp(x[r, i] - lse[r]) - sum_k coef[k] * twohot_k[r, i]),
// in the logits' dtype.
hipError_t launch_twohot_grad(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                              const float* lse, const TwoHotTargets& targets, const float* gout, void* grad,
                              hipStream_t stream);

// Kernel launches the three launchers have issued in this process.
int64_t twohot_launches();

}  // namespace emb
