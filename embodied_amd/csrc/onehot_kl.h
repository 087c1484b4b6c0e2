// Launchers of the OneHot KL kernels in onehot_kl.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kOneHotMaxClasses = 256;     // a group in one wave64: 4 values per lane

// post, prior: (rows, stoch, classes) logits, float32 or bfloat16 (arithmetic in
// float32).  Per row, summed over the stoch groups in a fixed order
// (dreamerv3/rssm.py:123-132 with embodied/jax/outs.py:208-263):
//   kl = sum p * (log p - log q), ent_post = -sum p log p, ent_prior = -sum q log q
// with p = (1 - unimix) softmax(post) + unimix / classes (q of prior alike;
// unimix == 0: p = softmax(post), its log taken in the log domain).
// dyn and rep (either may be null) both receive max(kl, free_nats), or kl where
// free_nats == 0.  rows, stoch >= 1, 1 <= classes <= kOneHotMaxClasses,
// rows * stoch * classes <= 2^31 - 1 (refused otherwise).
hipError_t launch_onehot_kl(const void* post, const void* prior, bool bf16, int64_t rows, int64_t stoch,
                            int64_t classes, float unimix, float free_nats, float* kl, float* ent_post,
                            float* ent_prior, float* dyn, float* rep, hipStream_t stream);

// grad_post = g_rep * f * d kl / d post, grad_prior = g_dyn * f * d kl / d prior in
// the logits' dtype, f the gradient of the maximum from the saved kl: 1 above
// free_nats, 0 below, 1/2 at equality, NaN for a NaN kl; free_nats == 0: 1 (NaN
// for a NaN kl).  A null grad_post / grad_prior is not written and its g not read.
hipError_t launch_onehot_kl_grad(const void* post, const void* prior, bool bf16, int64_t rows, int64_t stoch,
                                 int64_t classes, float unimix, float free_nats, const float* kl,
                                 const float* g_rep, const float* g_dyn, void* grad_post, void* grad_prior,
                                 hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t onehot_kl_launches();

}  // namespace emb
