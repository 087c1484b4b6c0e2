// Running return normaliser (embodied/jax/utils.py:16-91) as ONE launch of one
// workgroup: the batch statistics (mean and mean of squares, or two percentiles
// by exact radix select), the EMA step, the debiased (offset, scale) and,
// optionally, the normalised values.  Nothing returns to the host.
//
// Up to kNormLdsMax values keep their order-preserving integer keys in LDS; more
// values are re-read from global memory by every pass of the same kernel.
#include "wave_util.h"          // LaunchCount
#include "normalize_device.h"   // (float32 operations one by one: fp contract off)
#include "norm_select.h"        // to_key, hist_add, the two-rank radix select

#include <cmath>

namespace emb {
namespace {

constexpr int kWaves = kNormWaves;

// f(valid, key) for every value of x in global memory, in wave-uniform control
// flow (norm_select.h LdsKeys is the form over keys in LDS): what every pass of
// the select re-reads when the values do not fit in LDS.
struct GlobalKeys {
  const float* x;
  template <typename F>
  __device__ __forceinline__ void operator()(uint32_t n, F f) const {
    const uint32_t tid = threadIdx.x;
    const uint32_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (uint32_t base = 0; base < n4; base += kNormThreads) {
      const uint32_t i = base + tid;
      const bool valid = i < n4;
      const float4 v = valid ? x4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      f(valid, to_key(v.x));
      f(valid, to_key(v.y));
      f(valid, to_key(v.z));
      f(valid, to_key(v.w));
    }
    for (uint32_t base = n4 * 4; base < n; base += kNormThreads) {
      const uint32_t i = base + tid;
      const bool valid = i < n;
      f(valid, to_key(valid ? x[i] : 0.f));
    }
  }
};

template <bool kLds>
__global__ __launch_bounds__(kNormThreads) void normalize_kernel(
    const float* x, const float* sub, float* out, float* state, uint32_t n, uint32_t flags,
    float keep, float rate, float limit, uint32_t k_lo, uint32_t k_hi, float frac_lo, float frac_hi) {
  __shared__ uint32_t keys[kLds ? kNormLdsMax : 1];
  __shared__ uint32_t hist[2][kNormBins];
  __shared__ double sums[kWaves][2];
  __shared__ uint32_t sel[2][3];       // per rank: the digit, keys below it, keys in it
  __shared__ uint32_t next_key[2];

  const uint32_t tid = threadIdx.x;
  const uint32_t impl = flags & 3u;
  const bool update = flags & 4u, debias = flags & 8u;

  // Every lane carries the state: read before the first barrier, written by
  // lane 0 after the last one (update = 0 writes only the words nobody reads).
  float v0 = state[0], v1 = state[1], vc = state[2];
  float new0 = 0.f, new1 = 0.f;

  if (update && impl == kNormMeanStd) {
    double s = 0.0, s2 = 0.0;
    const uint32_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (uint32_t i = tid; i < n4; i += kNormThreads) {
      const float4 v = x4[i];
      s += (static_cast<double>(v.x) + static_cast<double>(v.y)) + (static_cast<double>(v.z) + static_cast<double>(v.w));
      s2 += (static_cast<double>(v.x * v.x) + static_cast<double>(v.y * v.y)) +
            (static_cast<double>(v.z * v.z) + static_cast<double>(v.w * v.w));   // squares in float32, as jnp.square
    }
    for (uint32_t i = n4 * 4 + tid; i < n; i += kNormThreads) {
      const float v = x[i];
      s += static_cast<double>(v);
      s2 += static_cast<double>(v * v);
    }
    double both[2] = {s, s2};
    norm_block_sum(both, sums);
    s = both[0], s2 = both[1];
    new0 = static_cast<float>(s / static_cast<double>(n));
    new1 = static_cast<float>(s2 / static_cast<double>(n));
  }

  if (update && impl == kNormPerc) {
    if constexpr (kLds)
      for (uint32_t i = tid; i < n; i += kNormThreads) keys[i] = to_key(x[i]);
    NormPair picked;
    if constexpr (kLds) picked = norm_select2(keys, n, k_lo, k_hi, frac_lo, frac_hi, hist, sel, next_key);
    else picked = norm_select2_over(GlobalKeys{x}, n, k_lo, k_hi, frac_lo, frac_hi, hist, sel, next_key);
    new0 = picked.new0, new1 = picked.new1;
  }

  const NormWords w = norm_step(v0, v1, vc, new0, new1, impl, update, debias, NormParams{keep, rate, limit});
  const float offset = w.offset, scale = w.scale;
  if (tid == 0) norm_store(state, w, update, debias);

  if (out) {       // out may be x: every element is read and written by the same lane
    const bool wide = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) |
                        reinterpret_cast<uintptr_t>(sub)) & 15) == 0;
    const uint32_t n4 = wide ? n / 4 : 0;
    for (uint32_t i = tid; i < n4; i += kNormThreads) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      float4 s = make_float4(offset, offset, offset, offset);
      if (sub) s = reinterpret_cast<const float4*>(sub)[i];
      reinterpret_cast<float4*>(out)[i] =
          make_float4((v.x - s.x) / scale, (v.y - s.y) / scale, (v.z - s.z) / scale, (v.w - s.w) / scale);
    }
    for (uint32_t i = n4 * 4 + tid; i < n; i += kNormThreads) out[i] = (x[i] - (sub ? sub[i] : offset)) / scale;
  }
}

segment::LaunchCount g_count;

}  // namespace

NormRank norm_rank(double q, int64_t n) {
  if (n <= 0) return {0u, 0.f};
  const double last = static_cast<double>(n - 1);
  const double pos = q / 100.0 * last;
  const double below = std::fmin(std::fmax(std::floor(pos), 0.0), last);
  return {static_cast<uint32_t>(below), static_cast<float>(pos - below)};
}

int64_t normalize_launches() { return g_count.value(); }

hipError_t launch_normalize(const float* x, int64_t n, float* state, int impl, bool update,
                            bool debias, float keep, float rate, float limit, NormRank lo, NormRank hi,
                            const float* sub, float* out, hipStream_t stream) {
  const uint32_t flags = static_cast<uint32_t>(impl) | (update ? 4u : 0u) | (debias ? 8u : 0u);
  const uint32_t count = static_cast<uint32_t>(n);
  if (n <= kNormLdsMax)
    hipLaunchKernelGGL(normalize_kernel<true>, dim3(1), dim3(kNormThreads), 0, stream, x, sub, out, state,
                       count, flags, keep, rate, limit, lo.k, hi.k, lo.frac, hi.frac);
  else
    hipLaunchKernelGGL(normalize_kernel<false>, dim3(1), dim3(kNormThreads), 0, stream, x, sub, out, state,
                       count, flags, keep, rate, limit, lo.k, hi.k, lo.frac, hi.frac);
  return g_count.launched();
}

}  // namespace emb
