// The actor's loss of DreamerV3's imagination, imag_loss (dreamerv3/agent.py:411-415)
//   logpi = sum_k policy[k].logp(act[k])[:, :-1],  ents = policy[k].entropy()[:, :-1]
//   policy_loss = sg(weight[:, :-1]) * -(logpi * sg(adv_normed) + actent * ents)
// over policy = Agg(Normal(mean, stddev), dims, sum) as Head.bounded_normal and
// Head.normal_logstd build it (embodied/jax/heads.py:146-162, embodied/jax/outs.py:40-76,
// 161-186), as kernels over the (N, T, A) raw head outputs and float32 actions:
//   forward  one read of the inputs: per kept row (n, t), t < T - drop, logpi, the
//            entropy and the loss; a dropped step is not read
//   grad     one more read and the closed form (normal_policy.h), both gradients;
//            a dropped step's rows are written as zeros by the same launch
//   sample   act = mean + std * eps, eps the caller's or a Philox Box-Muller draw
//   normal   the eps stream alone, for the composed path and the tests
// With torch ops the loss is about two dozen elementwise passes and two reductions.
//
// A row of A action dimensions in a segment of W lanes, W the next power of two
// >= A (1 .. 64), so a wave64 works on 64 / W rows at a time (at A = 6 one wave per
// row would idle 58 lanes); 65 .. 256 dimensions: the whole wave on one row with 2
// or 4 values per lane.  The row sums are onehot_segment.h's butterflies inside
// the segment: their order is fixed by A, not by the grid.  No atomics, no traffic
// between waves: the same bits run to run.  Plain per-lane loads, so a pointer at
// any multiple of the element size is as good as an aligned one.
#include "normal_policy.h"
#include "onehot_segment.h"
#include "philox.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // waves per workgroup
constexpr int kThreads = kWave * kWaves;

using namespace segment;
static_assert(kWave == kLanes, "the segment helpers shuffle over one wave64");

constexpr float kHalfLog2Pi = 0.91893853320467274178f;     // log(2 pi) / 2
constexpr float kTwoPi = 6.28318530717958647692f;

// heads.py:151-152 / heads.py:161
__device__ __forceinline__ void moments(bool bounded, float m, float s, float lo, float span, float& mean, float& std) {
  if (bounded) {
    mean = tanhf(m);
    std = span * sigmoid(s + 2.f) + lo;
  } else {
    mean = m;
    std = expf(s);
  }
}

template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void normal_policy_loss_kernel(
    const T* __restrict__ mean_raw, const T* __restrict__ std_raw, const float* __restrict__ act,
    const float* __restrict__ adv, const float* __restrict__ weight, int64_t weight_stride, float* __restrict__ loss,
    float* __restrict__ logpi, float* __restrict__ ent, int32_t rows, int32_t steps, int32_t kept, int32_t dims,
    int32_t bounded, float lo, float span, float actent) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const int64_t passes = (static_cast<int64_t>(rows) + kSegs - 1) / kSegs;
  for (int64_t pass = static_cast<int64_t>(blockIdx.x) * kWaves + wave; pass < passes;
       pass += static_cast<int64_t>(gridDim.x) * kWaves) {         // uniform over the wave: the shuffles see 64 lanes
    const int64_t row = pass * kSegs + seg;
    const bool live = row < rows;
    const int64_t n = live ? row / kept : 0, t = live ? row % kept : 0;      // agent.py:411-413's [:, :-1]
    const int64_t at = (n * steps + t) * dims;
    float lp = 0.f, e = 0.f, flag = 0.f;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = sl + W * j;
      if (live && i < dims) {
        const float m = load(mean_raw, at + i), s = load(std_raw, at + i);
        float mean, std;
        moments(bounded != 0, m, s, lo, span, mean, std);
        if (act) {
          const float a = act[at + i];
          const float z = (a - mean) / std;
          lp = lp + ((-(z * z) * 0.5f - logf(std)) - kHalfLog2Pi);             // outs.py:174-176
          if (a != a) flag = quiet_nan();
        }
        e = e + (0.5f * logf(kTwoPi * (std * std)) + 0.5f);                    // outs.py:178-179
        if (m != m || s != s) flag = quiet_nan();
      }
    }
    lp = seg_sum<W>(lp);                                           // Agg's sum over the action dimensions, outs.py:63-64, 69-71
    e = seg_sum<W>(e);
    flag = seg_sum<W>(flag);
    if (flag != flag) lp = e = flag;                               // a NaN anywhere in the row: all three outputs
    if (live && sl == 0) {
      if (logpi) logpi[row] = lp;
      if (ent) ent[row] = e;
      if (loss) {                                                  // agent.py:413-414
        const float w = weight ? weight[n * weight_stride + t] : 1.f;
        const float advantage = adv ? adv[row] : 1.f;
        // -(a + b) as -a - b, as policy_loss.hip: actent = 0 gives the bits of -logpi; no action and
        // actent = -1 the bits of ent
        loss[row] = w * (-(lp * advantage) - actent * e);
      }
    }
  }
}

template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void normal_policy_loss_grad_kernel(
    const T* __restrict__ mean_raw, const T* __restrict__ std_raw, const float* __restrict__ act,
    const float* __restrict__ adv, const float* __restrict__ weight, int64_t weight_stride,
    const float* __restrict__ gout, T* __restrict__ grad_mean, T* __restrict__ grad_std, int32_t rows_in, int32_t steps,
    int32_t kept, int32_t dims, int32_t bounded, float lo, float span, float actent) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const int64_t passes = (static_cast<int64_t>(rows_in) + kSegs - 1) / kSegs;
  for (int64_t pass = static_cast<int64_t>(blockIdx.x) * kWaves + wave; pass < passes;
       pass += static_cast<int64_t>(gridDim.x) * kWaves) {         // uniform over the wave
    const int64_t row = pass * kSegs + seg;
    const bool live = row < rows_in;
    const int64_t n = live ? row / steps : 0, t = live ? row % steps : 0;
    const bool keep = live && t < kept;                            // a dropped step: zeros, its inputs are not read
    const int64_t at = row * dims;
    float m[NPER], s[NPER], a[NPER], flag = 0.f;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = sl + W * j;
      m[j] = s[j] = a[j] = 0.f;
      if (keep && i < dims) {
        m[j] = load(mean_raw, at + i);
        s[j] = load(std_raw, at + i);
        if (act) a[j] = act[at + i];
        if (m[j] != m[j] || s[j] != s[j] || a[j] != a[j]) flag = quiet_nan();
      }
    }
    flag = seg_sum<W>(flag);                                       // NaN if any element of the row is
    float scale = 0.f, advantage = 0.f;
    if (keep) {
      const int64_t out = n * kept + t;
      scale = gout[out] * (weight ? weight[n * weight_stride + t] : 1.f);
      advantage = adv ? adv[out] : 1.f;
    }
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = sl + W * j;
      if (!live || i >= dims) continue;                            // (the pass's shuffles are behind us)
      float gm = 0.f, gs = 0.f;
      if (keep) {
        float mean, std, dmean, dstd;
        moments(bounded != 0, m[j], s[j], lo, span, mean, std);
        if (bounded) {
          const float q = expf(-2.f * fabsf(m[j]));                // 1 - tanh^2 = 4 q / (1 + q)^2
          dmean = 4.f * q / ((1.f + q) * (1.f + q));
          dstd = span * (sigmoid(s[j] + 2.f) * sigmoid(-(s[j] + 2.f)));
        } else {
          dmean = 1.f;
          dstd = std;
        }
        float of_logp = 0.f;                                       // adv (z^2 - 1); no action: no logpi term
        if (act) {
          const float z = (a[j] - mean) / std;
          gm = -scale * (advantage * (z / std) * dmean);
          of_logp = advantage * (z * z - 1.f);
        }
        gs = -scale * ((of_logp + actent) / std * dstd);
        if (flag != flag) gm = gs = flag;                          // a poisoned row: NaN throughout
      }
      store(grad_mean, at + i, gm);
      store(grad_std, at + i, gs);
    }
  }
}

__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t offset, uint64_t e) {
  const philox::Block b = philox::block(seed, offset, e);
  const float u1 = static_cast<float>((b.word[0] >> 8) + 1u) * 0x1p-24f;       // 24 bits + 1: exact, in (0, 1]
  const float u2 = static_cast<float>(b.word[1] >> 8) * 0x1p-24f;              // in [0, 1)
  return sqrtf(-2.f * logf(u1)) * cosf(kTwoPi * u2);
}

__global__ __launch_bounds__(kThreads) void philox_normal_kernel(uint64_t seed, uint64_t offset, uint64_t first,
                                                                 int64_t count, float* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < count;
       i += static_cast<int64_t>(gridDim.x) * kThreads)
    out[i] = philox_normal(seed, offset, first + static_cast<uint64_t>(i));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void normal_sample_kernel(
    const T* __restrict__ mean_raw, const T* __restrict__ std_raw, const float* __restrict__ eps,
    float* __restrict__ act, int64_t count, int32_t bounded, float lo, float span, uint64_t seed, uint64_t offset) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < count;
       i += static_cast<int64_t>(gridDim.x) * kThreads) {
    float mean, std;
    moments(bounded != 0, load(mean_raw, i), load(std_raw, i), lo, span, mean, std);
    const float noise = eps ? eps[i] : philox_normal(seed, offset, static_cast<uint64_t>(i));
    act[i] = mean + std * noise;                                   // outs.py:170-172
  }
}

LaunchCount g_count;

bool fits(int64_t N, int64_t T, int64_t drop, int64_t A, int kind, float lo, float hi) {
  if (kind != kNormalBounded && kind != kNormalLogstd) return false;
  if (kind == kNormalBounded && !(lo > 0.f && hi >= lo && hi - hi == 0.f)) return false;
  return N >= 1 && T >= 1 && (drop == 0 || drop == 1) && A >= 1 && A <= kNormalMaxActions && T <= INT32_MAX / A &&
         N <= INT32_MAX / (T * A);
}

int segment_width(int64_t A) {
  int w = 1;
  while (w < A && w < kWave) w *= 2;
  return w;
}

int row_blocks(int64_t rows, int64_t A) {
  const int64_t segs = kWave / segment_width(A);
  const int64_t passes = (rows + segs - 1) / segs;
  const int64_t blocks = (passes + kWaves - 1) / kWaves;
  return static_cast<int>(blocks < kNormalMaxBlocks ? blocks : kNormalMaxBlocks);
}

int flat_blocks(int64_t count) {
  const int64_t blocks = (count + kThreads - 1) / kThreads;
  return static_cast<int>(blocks < kNormalMaxBlocks ? blocks : kNormalMaxBlocks);
}

// one lane for a row of one element, else the ladder of onehot_segment.h
#define EMB_NORMAL_BY_WIDTH(CALL, a)                \
  do {                                              \
    if ((a) <= 1) { CALL(1, 1); }                   \
    else EMB_SEGMENT_BY_WIDTH(CALL, a);             \
  } while (0)

}  // namespace

int64_t normal_policy_launches() { return g_count.value(); }

hipError_t launch_normal_policy_loss(const void* mean_raw, const void* std_raw, const float* act, bool bf16, int64_t N,
                                     int64_t T, int64_t drop, int64_t A, int kind, float lo, float hi, float actent,
                                     const float* adv, const float* weight, int64_t weight_stride, float* loss,
                                     float* logpi, float* ent, hipStream_t stream) {
  if (!fits(N, T, drop, A, kind, lo, hi) || T - drop < 1 || !mean_raw || !std_raw || (!loss && !logpi && !ent))
    return hipErrorInvalidValue;
  if (weight && weight_stride < T - drop) return hipErrorInvalidValue;
  const int64_t rows = N * (T - drop);
  const dim3 grid(row_blocks(rows, A)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), steps = static_cast<int32_t>(T), kept = static_cast<int32_t>(T - drop);
  const int32_t dims = static_cast<int32_t>(A), bounded = kind == kNormalBounded ? 1 : 0;
  const float span = hi - lo;
#define EMB_FORWARD(W_, NPER_)                                                                                    \
  if (bf16)                                                                                                       \
    hipLaunchKernelGGL((normal_policy_loss_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                    \
                       static_cast<const bf16_t*>(mean_raw), static_cast<const bf16_t*>(std_raw), act, adv,       \
                       weight, weight_stride, loss, logpi, ent, r, steps, kept, dims, bounded, lo, span, actent); \
  else                                                                                                            \
    hipLaunchKernelGGL((normal_policy_loss_kernel<float, W_, NPER_>), grid, block, 0, stream,                     \
                       static_cast<const float*>(mean_raw), static_cast<const float*>(std_raw), act, adv,         \
                       weight, weight_stride, loss, logpi, ent, r, steps, kept, dims, bounded, lo, span, actent)
  EMB_NORMAL_BY_WIDTH(EMB_FORWARD, A);
#undef EMB_FORWARD
  return g_count.launched();
}

hipError_t launch_normal_policy_loss_grad(const void* mean_raw, const void* std_raw, const float* act, bool bf16,
                                          int64_t N, int64_t T, int64_t drop, int64_t A, int kind, float lo, float hi,
                                          float actent, const float* adv, const float* weight, int64_t weight_stride,
                                          const float* gout, void* grad_mean, void* grad_std, hipStream_t stream) {
  if (!fits(N, T, drop, A, kind, lo, hi) || !mean_raw || !std_raw || !grad_mean || !grad_std)
    return hipErrorInvalidValue;
  if (T - drop >= 1 && !gout) return hipErrorInvalidValue;
  if (weight && weight_stride < T - drop) return hipErrorInvalidValue;
  const int64_t rows = N * T;
  const dim3 grid(row_blocks(rows, A)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), steps = static_cast<int32_t>(T), kept = static_cast<int32_t>(T - drop);
  const int32_t dims = static_cast<int32_t>(A), bounded = kind == kNormalBounded ? 1 : 0;
  const float span = hi - lo;
#define EMB_GRAD(W_, NPER_)                                                                                       \
  if (bf16)                                                                                                       \
    hipLaunchKernelGGL((normal_policy_loss_grad_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,               \
                       static_cast<const bf16_t*>(mean_raw), static_cast<const bf16_t*>(std_raw), act, adv,       \
                       weight, weight_stride, gout, static_cast<bf16_t*>(grad_mean),                              \
                       static_cast<bf16_t*>(grad_std), r, steps, kept, dims, bounded, lo, span, actent);          \
  else                                                                                                            \
    hipLaunchKernelGGL((normal_policy_loss_grad_kernel<float, W_, NPER_>), grid, block, 0, stream,                \
                       static_cast<const float*>(mean_raw), static_cast<const float*>(std_raw), act, adv,         \
                       weight, weight_stride, gout, static_cast<float*>(grad_mean), static_cast<float*>(grad_std),\
                       r, steps, kept, dims, bounded, lo, span, actent)
  EMB_NORMAL_BY_WIDTH(EMB_GRAD, A);
#undef EMB_GRAD
  return g_count.launched();
}

hipError_t launch_philox_normal(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, float* out,
                                hipStream_t stream) {
  if (count < 1 || !out) return hipErrorInvalidValue;
  const dim3 grid(flat_blocks(count)), block(kThreads);
  hipLaunchKernelGGL(philox_normal_kernel, grid, block, 0, stream, seed, offset, first, count, out);
  return g_count.launched();
}

hipError_t launch_normal_sample(const void* mean_raw, const void* std_raw, bool bf16, int64_t rows, int64_t A, int kind,
                                float lo, float hi, uint64_t seed, uint64_t offset, const float* eps, float* act,
                                hipStream_t stream) {
  if (kind != kNormalBounded && kind != kNormalLogstd) return hipErrorInvalidValue;
  if (kind == kNormalBounded && !(lo > 0.f && hi >= lo && hi - hi == 0.f)) return hipErrorInvalidValue;
  if (rows < 1 || A < 1 || rows > INT32_MAX / A || !mean_raw || !std_raw || !act) return hipErrorInvalidValue;
  const int64_t count = rows * A;
  const dim3 grid(flat_blocks(count)), block(kThreads);
  const int32_t bounded = kind == kNormalBounded ? 1 : 0;
  const float span = hi - lo;
  if (bf16)
    hipLaunchKernelGGL(normal_sample_kernel<bf16_t>, grid, block, 0, stream, static_cast<const bf16_t*>(mean_raw),
                       static_cast<const bf16_t*>(std_raw), eps, act, count, bounded, lo, span, seed, offset);
  else
    hipLaunchKernelGGL(normal_sample_kernel<float>, grid, block, 0, stream, static_cast<const float*>(mean_raw),
                       static_cast<const float*>(std_raw), eps, act, count, bounded, lo, span, seed, offset);
  return g_count.launched();
}

}  // namespace emb
