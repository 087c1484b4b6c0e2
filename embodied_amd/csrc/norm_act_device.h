// Device pieces of Norm followed by the activation (embodied/jax/nets.py:361-399,
// nets.py:26-39) that more than one translation unit runs -- norm_act.hip and
// conv_stage.hip: how the threads of a row share its values, the row statistics,
// the activation and its slope, and the launch that adds the per-workgroup
// column sums.  ONE definition, so that a row comes out of either file by the
// same arithmetic.  Internal linkage: every translation unit gets its own copy.
#pragma once

#include "norm_act.h"
#include "wave_util.h"

// float32 operations one by one, as twohot.hip.  (From here to the end of the
// including translation unit: include the headers whose arithmetic may contract first.)
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kReduceBlock = 256;                 // threads of a workgroup of the reduce launch
constexpr int kReduceCols = 32, kReduceParts = kReduceBlock / kReduceCols;

using namespace segment;

// E = 16 bytes of T, at an address that is a multiple of 16
__device__ __forceinline__ void load16(const float* p, float* v) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void load16(const bf16_t* p, float* v) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = __uint_as_float(w[k] << 16);
    v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
  }
}
__device__ __forceinline__ void store16(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store16(bf16_t* p, const float* v) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = bf16_bits(v[2 * k]) | (static_cast<uint32_t>(bf16_bits(v[2 * k + 1])) << 16);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// Which elements of a row thread t of its TPR holds, T the row's storage type (the
// float32 parameters and partial sums follow the same map): value j is element
//   ((j / E) * TPR + t) * E + j % E,   E = 16 / sizeof(T): chunks of 16 bytes of T,
// moved as one 16-byte access (VEC) or element by element, one address per chunk.
// Elements past `units` read as `fill` and are not written.
template <typename T, int TPR, int PER, bool VEC>
struct Map {
  static constexpr int E = 16 / sizeof(T);
  static_assert(PER % E == 0, "whole chunks");

  static __device__ __forceinline__ int index(int j, int t) {
    return ((j / E) * TPR + t) * E + j % E;
  }

  // values c * E .. c * E + E - 1 of the thread: chunk c, whole (VEC) or by element
  template <typename S>
  static __device__ __forceinline__ void load_part(const S* row, int units, int t, int c, float fill, float (&v)[E]) {
    if constexpr (VEC) {
      const int at = (c * TPR + t) * E;
      if (row && at < units) {                                     // units % E == 0: a chunk is inside or outside
        if constexpr (sizeof(S) == 2) {
          load16(row + at, v);
        } else {
#pragma unroll
          for (int q = 0; q < E; q += 4) load16(row + at + q, &v[q]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = fill;
      }
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int i = (c * TPR + t) * E + k;
        v[k] = row && i < units ? segment::load(row, i) : fill;
      }
    }
  }

  template <typename S>
  static __device__ __forceinline__ void load(const S* row, int units, int t, float fill, float (&v)[PER]) {
#pragma unroll
    for (int c = 0; c < PER / E; ++c) {
      float part[E];
      load_part(row, units, t, c, fill, part);
#pragma unroll
      for (int k = 0; k < E; ++k) v[c * E + k] = part[k];
    }
  }

  template <typename S>
  static __device__ __forceinline__ void store_part(S* row, int units, int t, int c, const float (&v)[E]) {
    if constexpr (VEC) {
      const int at = (c * TPR + t) * E;
      if (at < units) {
        if constexpr (sizeof(S) == 2) {
          store16(row + at, v);
        } else {
#pragma unroll
          for (int q = 0; q < E; q += 4) store16(row + at + q, &v[q]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int i = (c * TPR + t) * E + k;
        if (i < units) segment::store(row, i, v[k]);
      }
    }
  }

  template <typename S>
  static __device__ __forceinline__ void store(S* row, int units, int t, const float (&v)[PER]) {
#pragma unroll
    for (int c = 0; c < PER / E; ++c) {
      float part[E];
#pragma unroll
      for (int k = 0; k < E; ++k) part[k] = v[c * E + k];
      store_part(row, units, t, c, part);
    }
  }
};

constexpr float kSqrt2OverPi = 0.7978845608028654f, kGeluCubic = 0.044715f;                 // jax.nn.gelu, approximate

__device__ __forceinline__ float activate(float y, int32_t act) {                           // nets.py:26-39
  switch (act) {
    case kActSilu: return y * sigmoid(y);
    case kActGelu: return y * (0.5f * (1.f + tanhf(kSqrt2OverPi * (y + kGeluCubic * (y * y * y)))));
    case kActRelu: return y < 0.f ? 0.f : y;                       // a NaN stays one (jnp.maximum)
    default: return y;
  }
}

__device__ __forceinline__ float activate_slope(float y, int32_t act) {
  switch (act) {
    case kActSilu: {
      const float s = sigmoid(y);
      return s * (1.f + y * (1.f - s));
    }
    case kActGelu: {
      const float th = tanhf(kSqrt2OverPi * (y + kGeluCubic * (y * y * y)));
      const float inner = kSqrt2OverPi * (1.f + (3.f * kGeluCubic) * (y * y));
      return 0.5f * (1.f + th) + (0.5f * y) * ((1.f - th * th) * inner);
    }
    case kActRelu: return y > 0.f ? 1.f : (y != y ? y : 0.f);
    default: return 1.f;
  }
}

// nets.py:383-391 from the row's two sums: the mean (0 for rms), rstd and the
// slope of max(0, .) at the variance (1 above 0, 1/2 at the tie, 0 below: what
// jnp.maximum's gradient is).  A row whose mean(x^2) is NaN or infinite: rstd NaN.
struct Stats {
  float mean, rstd, slope;
};

__device__ __forceinline__ Stats stats_of(float sum, float sum2, int32_t units, int32_t impl, float eps) {
  const float n = static_cast<float>(units);
  const float mean2 = sum2 / n;
  Stats s{0.f, 0.f, 1.f};
  float var = mean2;
  if (impl == kNormLayer) {
    s.mean = sum / n;
    const float raw = mean2 - s.mean * s.mean;
    var = raw > 0.f ? raw : (raw != raw ? raw : 0.f);              // jnp.maximum(0, .): a NaN stays one
    s.slope = raw > 0.f ? 1.f : (raw == 0.f ? 0.5f : 0.f);
  }
  s.rstd = mean2 - mean2 == 0.f ? 1.f / sqrtf(var + eps) : quiet_nan();
  return s;
}

// dscale / dshift from the (2, parts, units) partial sums: a workgroup takes
// kReduceCols columns, thread (q, c) adds rows q, q + 8, ... of column c in that
// order, the eight results meet in LDS and are added in the order of q.
__global__ __launch_bounds__(kReduceBlock) void norm_act_reduce_kernel(const float* __restrict__ partials,
                                                                float* __restrict__ dscale, float* __restrict__ dshift,
                                                                int32_t parts, int32_t units) {
  __shared__ float meet[kReduceParts][kReduceCols];
  float* out = blockIdx.y ? dshift : dscale;
  if (!out) return;                                                // uniform over the workgroup
  const float* src = partials + static_cast<int64_t>(blockIdx.y) * parts * units;
  const int lane = threadIdx.x % kReduceCols, q = threadIdx.x / kReduceCols;
  const int c = blockIdx.x * kReduceCols + lane;
  float s = 0.f;
  if (c < units)
    for (int p = q; p < parts; p += kReduceParts) s = s + src[static_cast<int64_t>(p) * units + c];
  meet[q][lane] = s;
  __syncthreads();
  if (q == 0 && c < units) {
    float total = meet[0][lane];
#pragma unroll
    for (int k = 1; k < kReduceParts; ++k) total = total + meet[k][lane];
    out[c] = total;
  }
}

}  // namespace
}  // namespace emb
