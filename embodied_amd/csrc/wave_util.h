// What the row-kernel families (the heads, the RSSM kernels, the optimizer, the
// metrics) share below their own arithmetic: bfloat16 storage, the butterflies of
// one wave64, sigmoid, the NaN they flag with and the launch counter.  A new
// family includes this header; it does not copy from it.
//
// No fp-contract pragma here (it would hold to the end of the including file, and
// ppo_targets.hip / dreamer_targets.hip include this ahead of scans that keep
// contraction on), so no function below may hold a multiply that feeds an add.
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

namespace emb {
namespace segment {

constexpr int kLanes = 64;                        // the wave

using bf16_t = uint16_t;                          // the storage; arithmetic is float32

__device__ __forceinline__ float widen(bf16_t v) { return __uint_as_float(static_cast<uint32_t>(v) << 16); }
// v as bfloat16: round to nearest even; a NaN keeps a set mantissa bit.
__device__ __forceinline__ bf16_t bf16_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return v != v ? static_cast<bf16_t>((u >> 16) | 0x40u) : static_cast<bf16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float load(const float* x, int64_t i) { return x[i]; }
__device__ __forceinline__ float load(const bf16_t* x, int64_t i) { return widen(x[i]); }
__device__ __forceinline__ void store(float* x, int64_t i, float v) { x[i] = v; }
__device__ __forceinline__ void store(bf16_t* x, int64_t i, float v) { x[i] = bf16_bits(v); }

// Butterflies over the W lanes of a segment: every lane of it ends with the same
// bits (a + b == b + a).
template <int W>
__device__ __forceinline__ float seg_max(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kLanes));
  return v;
}
template <int W, typename V>
__device__ __forceinline__ V seg_sum(V v) {
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
__device__ __forceinline__ float wave_max(float v) { return seg_max<kLanes>(v); }
__device__ __forceinline__ float wave_sum(float v) { return seg_sum<kLanes>(v); }
__device__ __forceinline__ int wave_sum(int v) { return seg_sum<kLanes>(v); }

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }     // jax.nn.sigmoid

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// Host: the launches of one translation unit that reached the stream.
struct LaunchCount {
  std::atomic<int64_t> n{0};
  hipError_t launched() {                         // after a launch: its status, counted on success
    const hipError_t status = hipGetLastError();
    if (status == hipSuccess) n.fetch_add(1, std::memory_order_relaxed);
    return status;
  }
  int64_t value() const { return n.load(std::memory_order_relaxed); }
};

}  // namespace segment
}  // namespace emb
