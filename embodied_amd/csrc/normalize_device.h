// Device pieces of the running return normaliser (embodied/jax/utils.py:16-91)
// that more than one kernel runs -- normalize.hip and ppo_targets.hip: the
// workgroup reduction of float64 sums, the EMA step with debiasing, and the
// (offset, scale) formed from the running statistics.  ONE definition, so that
// two kernels that hold the same state words return the same bits.
// Internal linkage: every translation unit gets its own copy.
#pragma once

#include "normalize.h"

// The reference runs float32 operations one by one; a fused multiply-add would
// round once where it rounds twice.  (From here to the end of the including
// translation unit: include the headers whose arithmetic may contract first.)
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kNormWave = 64;
constexpr int kNormWaves = kNormThreads / kNormWave;

// s[k] summed over the workgroup's kNormThreads lanes, for every lane: wave
// shuffles, then one partial per wave through LDS.  One __syncthreads.
template <int N>
__device__ __forceinline__ void norm_block_sum(double (&s)[N], double (*partial)[N]) {
  const uint32_t lane = threadIdx.x % kNormWave, wave = threadIdx.x / kNormWave;
  for (int o = kNormWave / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += __shfl_xor(s[k], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) partial[wave][k] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
  // (all partials of a fully unrolled loop are in registers at once: two doubles
  // per wave fit, four would spill under the 128 registers of a 1024-lane workgroup)
  constexpr int kAtOnce = N <= 2 ? kNormWaves : kNormWaves / 4;
#pragma unroll kAtOnce
  for (int w = 0; w < kNormWaves; ++w) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += partial[w][k];
  }
}

__device__ __forceinline__ float norm_ema(float keep, float var, float rate, float value) {
  return keep * var + rate * value;
}

// The hyper-parameters as the kernels receive them: `keep` = 1 - rate formed in
// double and rounded to float32 once, as the reference forms it.
struct NormParams {
  float keep, rate, limit;
};

// The running statistics (state words 0-2) and what stats() makes of them.
struct NormWords {
  float v0, v1, vc, offset, scale;
};

// utils.py:44-74: with `update` the statistics take one EMA step towards
// (new0, new1) and, with `debias`, corr towards 1; then (offset, scale).
__device__ __forceinline__ NormWords norm_step(float v0, float v1, float vc, float new0, float new1,
                                               uint32_t impl, bool update, bool debias, NormParams p) {
  if (update) {
    v0 = norm_ema(p.keep, v0, p.rate, new0);
    v1 = norm_ema(p.keep, v1, p.rate, new1);
    if (debias) vc = norm_ema(p.keep, vc, p.rate, 1.0f);
  }
  const float corr = debias ? 1.0f / fmaxf(p.rate, vc) : 1.0f;
  float offset, scale;
  if (impl == kNormMeanStd) {
    const float mean = v0 * corr;
    const float var = v1 * corr - mean * mean;
    offset = mean;
    scale = fmaxf(p.limit, sqrtf(fmaxf(0.f, var)));
  } else {
    const float lo = v0 * corr, hi = v1 * corr;
    offset = lo;
    scale = fmaxf(p.limit, hi - lo);
  }
  return {v0, v1, vc, offset, scale};
}

// One lane's write of the state words (update = 0 writes only the words nobody reads).
__device__ __forceinline__ void norm_store(float* state, const NormWords& w, bool update, bool debias) {
  if (update) {
    state[0] = w.v0;
    state[1] = w.v1;
    if (debias) state[2] = w.vc;
  }
  state[3] = w.offset;
  state[4] = w.scale;
}

}  // namespace
}  // namespace emb
