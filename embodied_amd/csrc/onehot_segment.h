// What one wave64 does with ONE operand of the Categorical / OneHot kernels
// (onehot_kl.hip, policy_loss.hip): a group of `classes` logits in a segment of W
// lanes, W the next power of two >= classes (2 .. 64), so a wave works on 64 / W
// groups at a time; 65 .. 256 classes: the whole wave on one group with 2 or 4
// values per lane.  Reductions are butterflies inside a segment, then one
// butterfly across the segments.  Device code only; included by those two
// translation units, which launch 4 such waves per workgroup and pick W and the
// values per lane from `classes` on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

// float32 operations one by one, as twohot.hip (holds to the end of the including file)
#pragma clang fp contract(off)

namespace emb {
namespace segment {

constexpr int kLanes = 64;                        // the wave

using bf16_t = uint16_t;                          // the storage; arithmetic is float32

__device__ __forceinline__ float load(const float* x, int64_t i) { return x[i]; }
__device__ __forceinline__ float load(const bf16_t* x, int64_t i) {
  return __uint_as_float(static_cast<uint32_t>(x[i]) << 16);
}
__device__ __forceinline__ void store(float* x, int64_t i, float v) { x[i] = v; }
__device__ __forceinline__ void store(bf16_t* x, int64_t i, float v) {
  const uint32_t u = __float_as_uint(v);
  // round to nearest even; a NaN keeps a set mantissa bit
  x[i] = v != v ? static_cast<bf16_t>((u >> 16) | 0x40u) : static_cast<bf16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// Butterflies over the W lanes of a segment: every lane of it ends with the same bits.
template <int W>
__device__ __forceinline__ float seg_max(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kLanes));
  return v;
}
template <int W>
__device__ __forceinline__ float seg_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kLanes);
  return v;
}
// ... and over the 64 / W segments of the wave, of a value every lane of a segment shares.
template <int W>
__device__ __forceinline__ float across_sum(float v) {
#pragma unroll
  for (int o = kLanes / 2; o >= W; o >>= 1) v = v + __shfl_xor(v, o, kLanes);
  return v;
}

// One group of one side, lane sl of its segment holding elements sl, sl + W, ...:
// sm = softmax(x) (outs.py:213), prob and logp the distribution the reference's
// logp, kl and entropy work on -- outs.py:214-216 with unimix, the logits themselves
// (log_softmax in the log domain, finite for an underflowed class) without.
// After the mix the probabilities sum to 1 up to rounding, so the second softmax
// / log_softmax of outs.py:228, 231-232, 237-239 is the identity and is not repeated.
// Lanes past `classes` hold zeros; a segment past the row's groups (!live) works on
// zeros and reads nothing.
template <int NPER>
struct Side {
  float sm[NPER], prob[NPER], logp[NPER];
};

template <typename T, int W, int NPER>
__device__ __forceinline__ Side<NPER> side(const T* x, bool live, int sl, int classes, float unimix, float keep,
                                           float uni) {
  Side<NPER> s;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    s.logp[j] = i < classes ? (live ? load(x, i) : 0.f) : -INFINITY;
    m = fmaxf(m, s.logp[j]);
  }
  m = seg_max<W>(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    s.sm[j] = i < classes ? expf(s.logp[j] - m) : 0.f;
    sum = sum + s.sm[j];
  }
  sum = seg_sum<W>(sum);
  const float lsum = logf(sum);
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const bool ok = sl + W * j < classes;
    const float sm = s.sm[j] / sum;
    s.sm[j] = ok ? sm : 0.f;
    if (unimix != 0.f) {
      const float prob = keep * sm + uni;
      s.prob[j] = ok ? prob : 0.f;
      s.logp[j] = ok ? logf(prob) : 0.f;
    } else {
      s.prob[j] = s.sm[j];
      s.logp[j] = ok ? (s.logp[j] - m) - lsum : 0.f;
    }
  }
  return s;
}

}  // namespace segment
}  // namespace emb
