// Launcher of the running return normaliser in normalize.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

enum NormImpl { kNormMeanStd = 1, kNormPerc = 2 };

constexpr int kNormThreads = 1024;     // one workgroup of 16 waves
constexpr int kNormLdsMax = 16384;     // values whose sort keys stay in LDS (64 KiB)
constexpr int kNormState = 5;          // mean|lo, sqrs|hi, corr, offset, scale

// From kNormGridMin values on, a call is the chain of launches in
// normalize_grid.hip: `groups` workgroups of kNormGridThreads lanes, each on one
// contiguous tile of x for the whole call.  Measured (tools/bench_normalize.py,
// profiles/normalize_bench.txt): the smallest n of that table at which the chain
// is below the one-workgroup kernel for both impls, with and without `out`.
constexpr int kNormGridMin = 131072;
constexpr int kNormGridThreads = 256;  // four waves: one per rank of the select
constexpr int kNormGridPer = 4096;     // values of a workgroup while there are fewer than ...
constexpr int kNormGridMax = 256;      // ... this many workgroups (one per CU)
constexpr int kNormGridRanks = 4;      // k_lo, k_lo + 1, k_hi, k_hi + 1

struct NormGridPlan {
  uint32_t groups, tile;               // tile: a multiple of 4, groups * tile >= n
};
inline NormGridPlan norm_grid_plan(int64_t n) {
  const int64_t want = (n + kNormGridPer - 1) / kNormGridPer;
  const int64_t groups = want < 1 ? 1 : want > kNormGridMax ? kNormGridMax : want;
  const int64_t tile = ((n + groups - 1) / groups + 3) / 4 * 4;
  return {static_cast<uint32_t>(groups), static_cast<uint32_t>(tile)};
}

// Percentile position of numpy's "linear" method: pos = q/100 * (n-1) in double;
// the order statistics floor(pos) and floor(pos)+1 (clipped) and the weight.
struct NormRank {
  uint32_t k;
  float frac;
};
NormRank norm_rank(double q, int64_t n);

// embodied/jax/utils.py:16-91: with `update` the running statistics in
// state[0..2] take one step from x[0..n), then state[3..4] = (offset, scale);
// with `out`, out[i] = (x[i] - (sub ? sub[i] : offset)) / scale.
// One launch of one workgroup up to kNormGridMin values; from there (with
// `update` or `out`) launch_normalize_grid's chain.
// `keep` = 1 - rate as the reference forms it: in double, rounded to float32 once.
hipError_t launch_normalize(const float* x, int64_t n, float* state, int impl, bool update,
                            bool debias, float keep, float rate, float limit, NormRank lo, NormRank hi,
                            const float* sub, float* out, hipStream_t stream);

// normalize_grid.hip: the same call over norm_grid_plan(n) workgroups, phases
// ordered by the stream -- up to 3 histogram passes (perc) or one of partial
// sums (meanstd), a one-workgroup finish, the output.  `launched`: += the
// kernels that reached the stream.  *taken = false, and nothing launched, where
// the stream is being captured and has no scratch block yet (none can be
// allocated then): the caller launches the one-workgroup kernel.
hipError_t launch_normalize_grid(const float* x, int64_t n, float* state, int impl, bool update,
                                 bool debias, float keep, float rate, float limit, NormRank lo, NormRank hi,
                                 const float* sub, float* out, hipStream_t stream, int64_t* launched, bool* taken);

// Kernel launches launch_normalize has issued in this process.
int64_t normalize_launches();

}  // namespace emb
