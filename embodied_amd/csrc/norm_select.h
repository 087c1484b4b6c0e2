// The exact two-rank radix select of the 'perc' return normaliser
// (embodied/jax/utils.py:76-91 through numpy's "linear" percentile) as a device
// function of one kNormThreads-lane workgroup, run by normalize.hip and
// dreamer_targets.hip.  ONE definition, so that two kernels that select from the
// same values return the same bits.
// Internal linkage: every translation unit gets its own copy.
#pragma once

#include "normalize_device.h"   // (float32 operations one by one: fp contract off)

namespace emb {
namespace {

constexpr int kNormBins = 2048;      // digits of 11, 11 and 10 bits, most significant first

// float32 -> uint32 with the same order (-0.0 sorts just below +0.0).
__device__ __forceinline__ uint32_t to_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float from_key(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// f(valid, key) for every one of n keys in LDS, in wave-uniform control flow:
// every lane of the workgroup makes the same number of calls, `valid` says
// whether this one counts.
struct LdsKeys {
  const uint32_t* keys;
  template <typename F>
  __device__ __forceinline__ void operator()(uint32_t n, F f) const {
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < n; base += kNormThreads) {
      const uint32_t i = base + tid;
      const bool valid = i < n;
      f(valid, valid ? keys[i] : 0u);
    }
  }
};

// hist[bin] += 1 for every active lane.  A wave whose active lanes all hit one
// bin (ties, a constant input) adds once instead of serialising 64 atomics.
__device__ __forceinline__ void hist_add(uint32_t* hist, bool active, uint32_t bin) {
  const unsigned long long lanes = __ballot(active);
  if (lanes == 0) return;
  const int first = __ffsll(static_cast<long long>(lanes)) - 1;
  const uint32_t bin0 = __shfl(bin, first);
  if (__all(!active || bin == bin0)) {
    if (static_cast<int>(threadIdx.x % kNormWave) == first) atomicAdd(&hist[bin0], static_cast<uint32_t>(__popcll(lanes)));
  } else if (active) {
    atomicAdd(&hist[bin], 1u);
  }
}

struct NormPair {
  float new0, new1;
};

// Order statistics k_lo, k_hi (and, where the weight is not zero, their
// successors) of the n keys that `for_keys(n, f)` visits, blended as numpy's
// linear percentile blends them.  Called by every lane of the workgroup; LDS:
// hist[2][kNormBins], sel[2][3] (per rank: the digit, keys below it, keys in
// it), next_key[2].  Every lane returns the same pair.
template <typename ForKeys>
__device__ __forceinline__ NormPair norm_select2_over(ForKeys for_keys, uint32_t n, uint32_t k_lo, uint32_t k_hi,
                                                      float frac_lo, float frac_hi, uint32_t (*hist)[kNormBins],
                                                      uint32_t (*sel)[3], uint32_t* next_key) {
  const uint32_t tid = threadIdx.x, lane = tid % kNormWave, wave = tid / kNormWave;
  // Radix select of both ranks at once: after each pass a rank knows one more
  // digit of its key and its position among the keys that share those digits.
  uint32_t prefix0 = 0, prefix1 = 0, mask0 = 0, mask1 = 0, rank0 = k_lo, rank1 = k_hi;
  uint32_t below0 = 0, below1 = 0, same0 = 0, same1 = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t bins = pass == 2 ? 1024u : 2048u;
    for (uint32_t i = tid; i < 2 * kNormBins; i += kNormThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    for_keys(n, [&](bool valid, uint32_t key) {
      const uint32_t bin = (key >> shift) & (bins - 1);
      hist_add(hist[0], valid && (key & mask0) == prefix0, bin);
      hist_add(hist[1], valid && (key & mask1) == prefix1, bin);
    });
    __syncthreads();
    if (wave < 2) {      // wave r finds rank r's digit: lane l owns bins [l * per, (l + 1) * per)
      const uint32_t* h = hist[wave];
      const uint32_t want = wave ? rank1 : rank0;
      const uint32_t per = bins / kNormWave;
      uint32_t mine = 0;
      for (uint32_t j = 0; j < per; ++j) mine += h[lane * per + ((j + lane) & (per - 1))];   // rotated: no bank conflicts
      uint32_t incl = mine;
      for (int o = 1; o < kNormWave; o <<= 1) {
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
    for_keys(n, [&](bool valid, uint32_t key) {
      if (valid && key > prefix0) m0 = min(m0, key);
      if (valid && key > prefix1) m1 = min(m1, key);
    });
    for (int o = kNormWave / 2; o > 0; o >>= 1) {
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
  return {after0 == prefix0 ? a0 : a0 + (b0 - a0) * frac_lo, after1 == prefix1 ? a1 : a1 + (b1 - a1) * frac_hi};
}

// The select over n <= kNormLdsMax keys that the workgroup has written to LDS
// (the caller's barrier, or the first one in here, orders those writes before
// the first read: the histogram is zeroed between them).
__device__ __forceinline__ NormPair norm_select2(const uint32_t* keys, uint32_t n, uint32_t k_lo, uint32_t k_hi,
                                                 float frac_lo, float frac_hi, uint32_t (*hist)[kNormBins],
                                                 uint32_t (*sel)[3], uint32_t* next_key) {
  return norm_select2_over(LdsKeys{keys}, n, k_lo, k_hi, frac_lo, frac_hi, hist, sel, next_key);
}

}  // namespace
}  // namespace emb
