// Running return normaliser (embodied/jax/utils.py:16-91) as ONE launch of one
// workgroup: the batch statistics (mean and mean of squares, or two percentiles
// by exact radix select), the EMA step, the debiased (offset, scale) and,
// optionally, the normalised values.  Nothing returns to the host.
//
// Up to kNormLdsMax values keep their order-preserving integer keys in LDS; more
// values are re-read from global memory by every pass of the same kernel.
#include "normalize_device.h"   // (float32 operations one by one: fp contract off)

#include <atomic>
#include <cmath>

namespace emb {
namespace {

constexpr int kWave = kNormWave;
constexpr int kWaves = kNormWaves;
constexpr int kBins = 2048;      // digits of 11, 11 and 10 bits, most significant first

// float32 -> uint32 with the same order (-0.0 sorts just below +0.0).
__device__ __forceinline__ uint32_t to_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float from_key(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// f(valid, key) for every value, in wave-uniform control flow: every lane of the
// workgroup makes the same number of calls, `valid` says whether this one counts.
template <bool kLds, typename F>
__device__ __forceinline__ void for_keys(const uint32_t* keys, const float* x, uint32_t n, F f) {
  const uint32_t tid = threadIdx.x;
  if constexpr (kLds) {
    for (uint32_t base = 0; base < n; base += kNormThreads) {
      const uint32_t i = base + tid;
      const bool valid = i < n;
      f(valid, valid ? keys[i] : 0u);
    }
  } else {
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
}

// hist[bin] += 1 for every active lane.  A wave whose active lanes all hit one
// bin (ties, a constant input) adds once instead of serialising 64 atomics.
__device__ __forceinline__ void hist_add(uint32_t* hist, bool active, uint32_t bin) {
  const unsigned long long lanes = __ballot(active);
  if (lanes == 0) return;
  const int first = __ffsll(static_cast<long long>(lanes)) - 1;
  const uint32_t bin0 = __shfl(bin, first);
  if (__all(!active || bin == bin0)) {
    if (static_cast<int>(threadIdx.x % kWave) == first) atomicAdd(&hist[bin0], static_cast<uint32_t>(__popcll(lanes)));
  } else if (active) {
    atomicAdd(&hist[bin], 1u);
  }
}

template <bool kLds>
__global__ __launch_bounds__(kNormThreads) void normalize_kernel(
    const float* x, const float* sub, float* out, float* state, uint32_t n, uint32_t flags,
    float keep, float rate, float limit, uint32_t k_lo, uint32_t k_hi, float frac_lo, float frac_hi) {
  __shared__ uint32_t keys[kLds ? kNormLdsMax : 1];
  __shared__ uint32_t hist[2][kBins];
  __shared__ double sums[kWaves][2];
  __shared__ uint32_t sel[2][3];       // per rank: the digit, keys below it, keys in it
  __shared__ uint32_t next_key[2];

  const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
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
    // Radix select of both ranks at once: after each pass a rank knows one more
    // digit of its key and its position among the keys that share those digits.
    uint32_t prefix0 = 0, prefix1 = 0, mask0 = 0, mask1 = 0, rank0 = k_lo, rank1 = k_hi;
    uint32_t below0 = 0, below1 = 0, same0 = 0, same1 = 0;
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
      const uint32_t bins = pass == 2 ? 1024u : 2048u;
      for (uint32_t i = tid; i < 2 * kBins; i += kNormThreads) (&hist[0][0])[i] = 0;
      __syncthreads();
      for_keys<kLds>(keys, x, n, [&](bool valid, uint32_t key) {
        const uint32_t bin = (key >> shift) & (bins - 1);
        hist_add(hist[0], valid && (key & mask0) == prefix0, bin);
        hist_add(hist[1], valid && (key & mask1) == prefix1, bin);
      });
      __syncthreads();
      if (wave < 2) {      // wave r finds rank r's digit: lane l owns bins [l * per, (l + 1) * per)
        const uint32_t* h = hist[wave];
        const uint32_t want = wave ? rank1 : rank0;
        const uint32_t per = bins / kWave;
        uint32_t mine = 0;
        for (uint32_t j = 0; j < per; ++j) mine += h[lane * per + ((j + lane) & (per - 1))];   // rotated: no bank conflicts
        uint32_t incl = mine;
        for (int o = 1; o < kWave; o <<= 1) {
          const uint32_t up = __shfl_up(incl, o);
          if (static_cast<int>(lane) >= o) incl += up;
        }
        uint32_t cum = incl - mine;
        if (want >= cum && want < incl) {          // one lane: the rank is below the number of keys left
          uint32_t bin = lane * per, count = 0;
          for (uint32_t j = 0; j < per; ++j) {
            count = h[lane * per + j];
            bin = lane * per + j;
            if (want < cum + count) break;
            cum += count;
          }
          sel[wave][0] = bin;
          sel[wave][1] = cum;
          sel[wave][2] = count;
        }
      }
      __syncthreads();
      const uint32_t digits = (bins - 1) << shift;
      prefix0 |= sel[0][0] << shift, mask0 |= digits, rank0 -= sel[0][1], below0 += sel[0][1], same0 = sel[0][2];
      prefix1 |= sel[1][0] << shift, mask1 |= digits, rank1 -= sel[1][1], below1 += sel[1][1], same1 = sel[1][2];
    }
    // prefix = the key of order statistic k.  Statistic k + 1 is the same key
    // while the run of equal keys lasts, else the smallest larger key.
    const bool next0 = frac_lo != 0.f && k_lo + 1 < n && k_lo + 1 >= below0 + same0;
    const bool next1 = frac_hi != 0.f && k_hi + 1 < n && k_hi + 1 >= below1 + same1;
    uint32_t after0 = prefix0, after1 = prefix1;
    if (next0 || next1) {
      if (tid < 2) next_key[tid] = 0xFFFFFFFFu;
      __syncthreads();
      uint32_t m0 = 0xFFFFFFFFu, m1 = 0xFFFFFFFFu;
      for_keys<kLds>(keys, x, n, [&](bool valid, uint32_t key) {
        if (valid && key > prefix0) m0 = min(m0, key);
        if (valid && key > prefix1) m1 = min(m1, key);
      });
      for (int o = kWave / 2; o > 0; o >>= 1) {
        m0 = min(m0, static_cast<uint32_t>(__shfl_xor(m0, o)));
        m1 = min(m1, static_cast<uint32_t>(__shfl_xor(m1, o)));
      }
      if (lane == 0) {
        atomicMin(&next_key[0], m0);
        atomicMin(&next_key[1], m1);
      }
      __syncthreads();
      if (next0) after0 = next_key[0];
      if (next1) after1 = next_key[1];
    }
    const float a0 = from_key(prefix0), b0 = from_key(after0);
    const float a1 = from_key(prefix1), b1 = from_key(after1);
    new0 = after0 == prefix0 ? a0 : a0 + (b0 - a0) * frac_lo;
    new1 = after1 == prefix1 ? a1 : a1 + (b1 - a1) * frac_hi;
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

std::atomic<int64_t> g_launches{0};

}  // namespace

NormRank norm_rank(double q, int64_t n) {
  if (n <= 0) return {0u, 0.f};
  const double last = static_cast<double>(n - 1);
  const double pos = q / 100.0 * last;
  const double below = std::fmin(std::fmax(std::floor(pos), 0.0), last);
  return {static_cast<uint32_t>(below), static_cast<float>(pos - below)};
}

int64_t normalize_launches() { return g_launches.load(std::memory_order_relaxed); }

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
  const hipError_t status = hipGetLastError();
  if (status == hipSuccess) g_launches.fetch_add(1, std::memory_order_relaxed);   // the only launch site of this file
  return status;
}

}  // namespace emb
