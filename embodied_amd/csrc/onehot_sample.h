// Launchers of the OneHot / Categorical sample kernels in onehot_sample.hip
// (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kSampleMaxClasses = 256;     // a group in one wave64: 4 values per lane

constexpr int kSampleDraw = 0;             // index by the inverse CDF of a uniform
constexpr int kSamplePred = 1;             // index = argmax of the logits, no uniform

// The stream every draw comes from, Philox4x32-10 (Salmon et al., SC'11):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (g & 0xffffffff, g >> 32, offset & 0xffffffff, offset >> 32)
//   u       = (word0 >> 8) * 2^-24, in [0, 1)
// out[i] = u(seed, offset, first + i) for i < count, float32.  count >= 1.
hipError_t launch_philox_uniform(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, float* out,
                                 hipStream_t stream);

// logits: (rows, groups, classes), float32 or bfloat16 (arithmetic in float32),
// read as rows * groups groups g.  Per group (embodied/jax/outs.py:208-224,
// 243-254, 265-270; dreamerv3/rssm.py:87, 100; dreamerv3/agent.py:18, 126, 192):
//   p = (1 - unimix) softmax(x) + unimix / classes           (unimix == 0: softmax(x))
//   mode kSampleDraw: u = uniform[g], or the Philox draw above if uniform is null;
//     index = the smallest k with p_k > 0 and C_k > u * C_last, C the inclusive
//     prefix sum of p in class order; none (rounding): the last class with p > 0
//   mode kSamplePred: index = argmax(x), the first on ties
//   index[g] int32; onehot[g, :] in the logits' dtype, exactly 0 or 1 -- the value
//   of sg(onehot) + (probs - sg(probs)), outs.py:267-269.  Either may be null.
// A group holding a NaN or +inf logit, or nothing but -inf: index -1, a one-hot
// row of NaN, no other group touched.  rows, groups >= 1, 1 <= classes <=
// kSampleMaxClasses, rows * groups * classes <= 2^31 - 1 (refused otherwise).
hipError_t launch_onehot_sample(const void* logits, bool bf16, int64_t rows, int64_t groups, int64_t classes,
                                float unimix, int mode, uint64_t seed, uint64_t offset, const float* uniform,
                                int32_t* index, void* onehot, hipStream_t stream);

// The straight-through gradient, which does not depend on the draw.  The value
// is sg(onehot) + (probs - sg(probs)) with probs = softmax(log p) (outs.py:268)
// and p = keep s + uni, s = softmax(x), keep = 1 - unimix (outs.py:213-216):
//   d value_k / d x_j = d probs_k / d x_j
//   probs_k = p_k / S, S = sum_m p_m = 1:  d probs_k / d p_m = delta_km - p_k
//   d p_m / d x_j = keep s_m (delta_mj - s_j),  and  sum_m d p_m / d x_j = 0
//   => d probs_k / d x_j = keep s_k (delta_kj - s_j)      (the p_k term drops out)
//   grad_j = sum_k gout_k d value_k / d x_j = keep s_j (gout_j - sum_k s_k gout_k)
// gout and grad (rows, groups, classes) in the logits' dtype, grad rounded once at
// the store.  An invalid group's gradient is NaN throughout.
hipError_t launch_onehot_sample_grad(const void* logits, const void* gout, bool bf16, int64_t rows, int64_t groups,
                                     int64_t classes, float unimix, void* grad, hipStream_t stream);

// Kernel launches the three launchers have issued in this process.
int64_t onehot_sample_launches();

}  // namespace emb
