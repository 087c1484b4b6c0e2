// Launcher of the fused DreamerV3 imagination targets in dreamer_targets.hip
// (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "normalize.h"

namespace emb {

// One running normaliser as the launch receives it: its five state words in
// device memory (normalize.h) and its hyper-parameters, `keep` = 1 - rate formed
// in double and rounded to float32 once.  impl 0 = none: the state is not read
// and (offset, scale) = (0, 1).
struct DreamerNorm {
  int impl;                // 0 | kNormMeanStd | kNormPerc
  float* state;
  float keep, rate, limit;
  bool debias;
  NormRank lo, hi;         // kNormPerc: the two percentile positions among N * (T-1) values
};

// imag_loss's targets (dreamerv3/agent.py:397-419) as ONE launch of one
// workgroup: tarval = pred * vscale + voffset from valnorm's statistics before
// the step, the lambda-return with term = 1 - con -> ret (N, T-1), weight (N, T)
// = cumprod(disc * con) / disc in numpy's order, retnorm ('perc') takes its
// step from ret, adv = (ret - tarval[:, :-1]) / rscale, advnorm its step from
// adv, valnorm its step from ret; adv_normed = (adv - aoffset) / ascale and
// tar_padded (N, T) = (ret - voffset') / vscale' with a zero last column.
// N >= 1, T >= 2, N * (T-1) <= kNormLdsMax (the caller checks; refused here too).
hipError_t launch_dreamer_targets(const float* rew, const float* con, const float* pred, int64_t N, int64_t T,
                                  float disc, float lam, bool update, float* ret, float* weight, float* adv,
                                  float* adv_normed, float* tar_padded, const DreamerNorm& retnorm,
                                  const DreamerNorm& valnorm, const DreamerNorm& advnorm, hipStream_t stream);

// Kernel launches launch_dreamer_targets has issued in this process.
int64_t dreamer_targets_launches();

}  // namespace emb
