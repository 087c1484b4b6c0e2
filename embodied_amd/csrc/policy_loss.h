// Launchers of the policy-head kernels in policy_loss.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kPolicyMaxClasses = 256;     // a group in one wave64: 4 values per lane

// logits: (N, T, groups, classes), float32 or bfloat16 (arithmetic in float32);
// act: (N, T, groups) int32, or null (no action: logpi = 0).  Per output row
// r = (n, t), t < T - drop, read at the logits' row n * T + t and summed over the
// groups in a fixed order (embodied/jax/outs.py:208-234 under Agg, outs.py:63-71,
// and dreamerv3/agent.py:411-414):
//   logpi = sum_g logp[g, act[g]]        an action outside [0, classes) adds 0
//   ent   = sum_g -sum_k p_k logp_k
//   loss  = weight[n * weight_stride + t] * -(logpi * adv[r] + actent * ent)
// with p = (1 - unimix) softmax + unimix / classes and logp = log p (unimix == 0:
// log_softmax in the log domain).  adv (N, T - drop) and weight may be null: 1.
// loss may be null: not written.  drop is 0 or 1: the last step of every n is
// not read.  N, T - drop, groups >= 1, 1 <= classes <= kPolicyMaxClasses,
// N * T * groups * classes <= 2^31 - 1, weight_stride >= T - drop (refused otherwise).
hipError_t launch_policy_loss(const void* logits, const int32_t* act, bool bf16, int64_t N, int64_t T, int64_t drop,
                              int64_t groups, int64_t classes, float unimix, float actent, const float* adv,
                              const float* weight, int64_t weight_stride, float* loss, float* logpi, float* ent,
                              hipStream_t stream);

// grad (N, T, groups, classes) in the logits' dtype: gout[r] * d loss[r] / d logits,
// the closed form from one more read of the logits; the rows of a dropped step
// are written as zeros; a row with a NaN or +inf logit or a group of -inf is NaN
// throughout.  Here T - drop may be 0 (every row is a dropped one).
hipError_t launch_policy_loss_grad(const void* logits, const int32_t* act, bool bf16, int64_t N, int64_t T,
                                   int64_t drop, int64_t groups, int64_t classes, float unimix, float actent,
                                   const float* adv, const float* weight, int64_t weight_stride, const float* gout,
                                   void* grad, hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t policy_loss_launches();

}  // namespace emb
