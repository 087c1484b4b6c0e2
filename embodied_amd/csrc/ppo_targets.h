// Launcher of the fused PPO targets in ppo_targets.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

// One running mean-std normaliser as the launch receives it: its five state
// words in device memory (normalize.h) and its hyper-parameters, `keep` = 1 - rate
// formed in double and rounded to float32 once.
struct PpoNorm {
  float* state;
  float keep, rate, limit;
  bool debias;
};

// The top of ppo_loss (ppo/agent.py:188-210) as ONE launch of one workgroup:
// val = pred * vscale + voffset from valnorm's statistics before the step, GAE
// over (B, T) -> adv, tar (B, T-1); with `update` both normalisers take their
// EMA step from tar resp. adv; then tar_normed (B, T) = clip((tar - voffset') /
// vscale', +-tarclip) with a zero last column (tarclip = 0: no clip) and
// adv_normed (B, T-1) = (adv - aoffset) / ascale.  B >= 1, T >= 2,
// B * T <= INT32_MAX (the caller checks).
hipError_t launch_ppo_targets(const float* rew, const float* pred, const uint8_t* last, const uint8_t* term,
                              int64_t B, int64_t T, float live_scale, float lam, float tarclip, bool update,
                              float* adv, float* tar, float* tar_normed, float* adv_normed,
                              const PpoNorm& valnorm, const PpoNorm& advnorm, hipStream_t stream);

// Kernel launches launch_ppo_targets has issued in this process.
int64_t ppo_targets_launches();

}  // namespace emb
