// The draw of the RSSM's one-hot latents and of the actor's discrete action
//   stoch = self._dist(logit).sample(seed)        (dreamerv3/rssm.py:87, 100)
//   act   = sample(policy)                        (dreamerv3/agent.py:18, 126, 192)
// over OneHot / Categorical (embodied/jax/outs.py:208-224, 243-254, 265-270), as
// one kernel over the (rows, groups, classes) logits:
//   sample   one read of the logits: softmax, the unimix blend, a Philox draw (or
//            the caller's uniform), the inverse CDF in class order, the index and
//            the straight-through one-hot
//   grad     one more read and the closed form (onehot_sample.h derives it); it
//            does not depend on the draw, nothing the forward wrote is used
//   uniform  the Philox stream alone, for the composed path and the tests
// With torch ops the same is about a dozen passes.
//
// One segment of W lanes per group as onehot_kl.hip (onehot_segment.h), a wave64
// on 64 / W consecutive groups at a time.  The draw depends on (seed, offset, g)
// and on nothing else: every lane of a segment runs the ten Philox rounds on its
// group's counter and holds the same uniform.  The CDF is an inclusive scan
// across the segment's lanes (six shuffles at W = 64); with 2 or 4 values per
// lane the strided layout of onehot_segment.h holds classes 64 j .. 64 j + 63 in
// stripe j, so one scan per stripe plus the totals of the stripes before it is
// the CDF in class order.  The index is a minimum over the lanes whose CDF
// exceeds the threshold: it is compared with the lane's class and never used as
// an address.  No atomics, no traffic between waves: the same bits run to run.
#include "onehot_sample.h"
#include "onehot_segment.h"
#include "philox.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // waves per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups of 4 waves on each of 256 CUs; more groups: grid stride

using namespace segment;
static_assert(kWave == kLanes, "the segment helpers shuffle over one wave64");

// Philox4x32-10, word 0 of the block at counter (g, offset) under key seed.
__device__ __forceinline__ uint32_t philox_word0(uint64_t seed, uint64_t offset, uint64_t g) {
  return philox::block(seed, offset, g).word[0];              // the ten rounds: philox.h
}

__device__ __forceinline__ float to_uniform(uint32_t word) {
  return static_cast<float>(word >> 8) * 0x1p-24f;          // 24 bits: exact, in [0, 1)
}

__global__ __launch_bounds__(kThreads) void philox_uniform_kernel(uint64_t seed, uint64_t offset, uint64_t first,
                                                                  int64_t count, float* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < count;
       i += static_cast<int64_t>(gridDim.x) * kThreads)
    out[i] = to_uniform(philox_word0(seed, offset, first + static_cast<uint64_t>(i)));
}

template <int W>
__device__ __forceinline__ int seg_min(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kLanes));
  return v;
}
template <int W>
__device__ __forceinline__ int seg_imax(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kLanes));
  return v;
}
// Inclusive prefix sum over the W lanes of a segment, lane order.
template <int W>
__device__ __forceinline__ float seg_scan(float v, int sl) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) {
    const float below = __shfl_up(v, o, W);
    if (sl >= o) v = v + below;
  }
  return v;
}

// The group's largest logit with a NaN counted as +inf: +inf or -inf says the
// group is invalid (a NaN or +inf logit, or nothing but -inf).  x[j] are the
// lane's logits, -inf past `classes`.
template <typename T, int W, int NPER>
__device__ __forceinline__ float checked_max(const T* x, bool live, int sl, int classes, float (&v)[NPER]) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    v[j] = i < classes ? (live ? load(x, i) : 0.f) : -INFINITY;
    m = fmaxf(m, v[j] != v[j] ? INFINITY : v[j]);
  }
  return seg_max<W>(m);
}

template <typename T, int W, int NPER, bool PRED>
__global__ __launch_bounds__(kThreads) void onehot_sample_kernel(
    const T* __restrict__ logits, const float* __restrict__ uniform, int32_t* __restrict__ index,
    T* __restrict__ onehot, uint64_t seed, uint64_t offset, int64_t count, int32_t classes, float unimix) {
  constexpr int kSegs = kWave / W;
  constexpr int kNone = 1 << 30;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));     // outs.py:214-215
  const int64_t passes = (count + kSegs - 1) / kSegs;
  for (int64_t pass = static_cast<int64_t>(blockIdx.x) * kWaves + wave; pass < passes;
       pass += static_cast<int64_t>(gridDim.x) * kWaves) {         // uniform over the wave: the shuffles see 64 lanes
    const int64_t g = pass * kSegs + seg;
    const bool live = g < count;
    const T* x = logits + g * classes;
    float v[NPER];
    const float m = checked_max<T, W, NPER>(x, live, sl, classes, v);
    const bool valid = m != INFINITY && m != -INFINITY;
    int k;
    if constexpr (PRED) {                                          // outs.py:219-220, the first on ties
      int first = kNone;
#pragma unroll
      for (int j = NPER - 1; j >= 0; --j)
        if (v[j] == m) first = sl + W * j;                         // (a lane past `classes` holds -inf, m is finite)
      k = seg_min<W>(first);
    } else {
      const Side<NPER> s = side<T, W, NPER>(x, live, sl, classes, unimix, keep, uni);
      // C in class order: stripe j is classes W j .. W j + W - 1, a scan over the lanes plus the stripes before
      float c[NPER], base = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        c[j] = base + seg_scan<W>(s.prob[j], sl);
        base = __shfl(c[j], W - 1, W);
      }
      const int last = classes - 1;
      float total = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j)
        if (last / W == j) total = __shfl(c[j], last % W, W);      // C of the last class (uniform branch)
      const float u = live ? (uniform ? uniform[g] : to_uniform(philox_word0(seed, offset, static_cast<uint64_t>(g))))
                           : 0.f;
      const float threshold = u * total;
      int first = kNone, tail = -1;
#pragma unroll
      for (int j = NPER - 1; j >= 0; --j) {
        const int i = sl + W * j;
        if (i < classes && s.prob[j] > 0.f && c[j] > threshold) first = i;
      }
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        const int i = sl + W * j;
        if (i < classes && s.prob[j] > 0.f) tail = i;
      }
      k = seg_min<W>(first);
      tail = seg_imax<W>(tail);
      if (k == kNone) k = tail;                                    // rounding left no class above the threshold
    }
    if (!valid) k = -1;
    if (live) {
      if (index && sl == 0) index[g] = k;
      if (onehot) {
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
          const int i = sl + W * j;
          if (i < classes)
            store(onehot + g * classes, i, valid ? (i == k ? 1.f : 0.f) : quiet_nan());
        }
      }
    }
  }
}

template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void onehot_sample_grad_kernel(
    const T* __restrict__ logits, const T* __restrict__ gout, T* __restrict__ grad, int64_t count, int32_t classes,
    float unimix) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));
  const int64_t passes = (count + kSegs - 1) / kSegs;
  for (int64_t pass = static_cast<int64_t>(blockIdx.x) * kWaves + wave; pass < passes;
       pass += static_cast<int64_t>(gridDim.x) * kWaves) {         // uniform over the wave
    const int64_t g = pass * kSegs + seg;
    const bool live = g < count;
    const int64_t at = g * classes;
    float v[NPER];
    const float m = checked_max<T, W, NPER>(logits + at, live, sl, classes, v);
    const bool valid = m != INFINITY && m != -INFINITY;
    const Side<NPER> s = side<T, W, NPER>(logits + at, live, sl, classes, unimix, keep, uni);
    float up[NPER], dot = 0.f;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = sl + W * j;
      up[j] = live && i < classes ? load(gout + at, i) : 0.f;
      dot = dot + s.sm[j] * up[j];
    }
    dot = seg_sum<W>(dot);
    if (live) {
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        const int i = sl + W * j;
        if (i < classes)
          store(grad + at, i, valid ? keep * (s.sm[j] * (up[j] - dot)) : quiet_nan());
      }
    }
  }
}

LaunchCount g_count;

bool fits(int64_t rows, int64_t groups, int64_t classes) {
  return rows >= 1 && groups >= 1 && classes >= 1 && classes <= kSampleMaxClasses && groups <= INT32_MAX / classes &&
         rows <= INT32_MAX / (groups * classes);
}

int pass_blocks(int64_t count, int64_t classes) {
  int w = 2;
  while (w < classes && w < kWave) w *= 2;
  const int64_t segs = kWave / w;
  const int64_t passes = (count + segs - 1) / segs;
  const int64_t blocks = (passes + kWaves - 1) / kWaves;
  return static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace

int64_t onehot_sample_launches() { return g_count.value(); }

hipError_t launch_philox_uniform(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, float* out,
                                 hipStream_t stream) {
  if (count < 1 || !out) return hipErrorInvalidValue;
  const int64_t blocks = (count + kThreads - 1) / kThreads;
  const dim3 grid(static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(kThreads);
  hipLaunchKernelGGL(philox_uniform_kernel, grid, block, 0, stream, seed, offset, first, count, out);
  return g_count.launched();
}

hipError_t launch_onehot_sample(const void* logits, bool bf16, int64_t rows, int64_t groups, int64_t classes,
                                float unimix, int mode, uint64_t seed, uint64_t offset, const float* uniform,
                                int32_t* index, void* onehot, hipStream_t stream) {
  if (!fits(rows, groups, classes) || !logits || (!index && !onehot)) return hipErrorInvalidValue;
  if (mode != kSampleDraw && mode != kSamplePred) return hipErrorInvalidValue;
  const int64_t count = rows * groups;
  const dim3 grid(pass_blocks(count, classes)), block(kThreads);
  const int32_t c = static_cast<int32_t>(classes);
  const bool pred = mode == kSamplePred;
#define EMB_KERNEL(T_, W_, NPER_, PRED_)                                                                     \
  hipLaunchKernelGGL((onehot_sample_kernel<T_, W_, NPER_, PRED_>), grid, block, 0, stream,                    \
                     static_cast<const T_*>(logits), uniform, index, static_cast<T_*>(onehot), seed, offset, \
                     count, c, unimix)
#define EMB_FORWARD(W_, NPER_)                                 \
  if (bf16) {                                                  \
    if (pred) EMB_KERNEL(bf16_t, W_, NPER_, true);             \
    else EMB_KERNEL(bf16_t, W_, NPER_, false);                 \
  } else {                                                     \
    if (pred) EMB_KERNEL(float, W_, NPER_, true);              \
    else EMB_KERNEL(float, W_, NPER_, false);                  \
  }
  EMB_SEGMENT_BY_WIDTH(EMB_FORWARD, classes);
#undef EMB_FORWARD
#undef EMB_KERNEL
  return g_count.launched();
}

hipError_t launch_onehot_sample_grad(const void* logits, const void* gout, bool bf16, int64_t rows, int64_t groups,
                                     int64_t classes, float unimix, void* grad, hipStream_t stream) {
  if (!fits(rows, groups, classes) || !logits || !gout || !grad) return hipErrorInvalidValue;
  const int64_t count = rows * groups;
  const dim3 grid(pass_blocks(count, classes)), block(kThreads);
  const int32_t c = static_cast<int32_t>(classes);
#define EMB_GRAD(W_, NPER_)                                                                                    \
  if (bf16)                                                                                                    \
    hipLaunchKernelGGL((onehot_sample_grad_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                 \
                       static_cast<const bf16_t*>(logits), static_cast<const bf16_t*>(gout),                   \
                       static_cast<bf16_t*>(grad), count, c, unimix);                                          \
  else                                                                                                         \
    hipLaunchKernelGGL((onehot_sample_grad_kernel<float, W_, NPER_>), grid, block, 0, stream,                  \
                       static_cast<const float*>(logits), static_cast<const float*>(gout),                     \
                       static_cast<float*>(grad), count, c, unimix)
  EMB_SEGMENT_BY_WIDTH(EMB_GRAD, classes);
#undef EMB_GRAD
  return g_count.launched();
}

}  // namespace emb
