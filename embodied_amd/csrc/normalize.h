// Launcher of the running return normaliser in normalize.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

enum NormImpl { kNormMeanStd = 1, kNormPerc = 2 };

constexpr int kNormThreads = 1024;     // one workgroup of 16 waves
constexpr int kNormLdsMax = 16384;     // values whose sort keys stay in LDS (64 KiB)
constexpr int kNormState = 5;          // mean|lo, sqrs|hi, corr, offset, scale

// Percentile position of numpy's "linear" method: pos = q/100 * (n-1) in double;
// the order statistics floor(pos) and floor(pos)+1 (clipped) and the weight.
struct NormRank {
  uint32_t k;
  float frac;
};
NormRank norm_rank(double q, int64_t n);

// One launch of one workgroup (embodied/jax/utils.py:16-91): with `update` the
// running statistics in state[0..2] take one step from x[0..n), then
// state[3..4] = (offset, scale); with `out` the same launch writes
// out[i] = (x[i] - (sub ? sub[i] : offset)) / scale.
// `keep` = 1 - rate as the reference forms it: in double, rounded to float32 once.
hipError_t launch_normalize(const float* x, int64_t n, float* state, int impl, bool update,
                            bool debias, float keep, float rate, float limit, NormRank lo, NormRank hi,
                            const float* sub, float* out, hipStream_t stream);

// Kernel launches launch_normalize has issued in this process.
int64_t normalize_launches();

}  // namespace emb
