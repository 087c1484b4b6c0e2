// The actor's loss of DreamerV3's imagination, imag_loss (dreamerv3/agent.py:411-415)
//   logpi = sum_k policy[k].logp(act[k])[:, :-1],  ents = policy[k].entropy()[:, :-1]
//   policy_loss = sg(weight[:, :-1]) * -(logpi * sg(adv_normed) + actent * ents)
// over policy = Agg(Categorical(logits, unimix), dims, sum) (embodied/jax/heads.py:90-91,
// 101-110, embodied/jax/outs.py:40-76, 208-234), as two kernels over the
// (N, T, groups, classes) logits and the (N, T, groups) int32 actions:
//   forward  one read of the logits: per kept row (n, t), t < T - drop, logpi, the
//            entropy and the loss; the [:, :-1] is taken here, a dropped step's
//            logits are not read and nothing is sliced or copied
//   grad     one more read and the closed form, nothing saved by the forward is
//            used; a dropped step's rows are written as zeros by the same launch
// With torch ops the same is a few dozen passes and a materialised one-hot.
//
// One wave64 per row, a group of `classes` logits in a segment of W lanes as
// onehot_kl.hip (onehot_segment.h).  The action is compared with the lane's
// class index and never used as an address: one outside [0, classes) matches no
// lane and adds 0, as jax.nn.one_hot's row of zeros does.  A row's sums over its
// groups are each segment's running sums in the order of the groups, then one
// butterfly across the segments.  No atomics, no traffic between waves: the
// same bits run to run.
#include "policy_loss.h"
#include "onehot_segment.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // rows per workgroup at a time
constexpr int kThreads = kWave * kWaves;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups of 4 waves on each of 256 CUs; more rows: grid stride

using namespace segment;
static_assert(kWave == kLanes, "the segment helpers shuffle over one wave64");

template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void policy_loss_kernel(
    const T* __restrict__ logits, const int32_t* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ weight, int64_t weight_stride, float* __restrict__ loss, float* __restrict__ logpi,
    float* __restrict__ ent, int32_t rows, int32_t steps, int32_t kept, int32_t groups, int32_t classes, float unimix,
    float actent) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));     // outs.py:214-215
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave: the shuffles see 64 lanes
    const int64_t n = row / kept, t = row % kept;                  // agent.py:411-413's [:, :-1]
    const int64_t arow = (n * steps + t) * groups;
    float row_lp = 0.f, row_ent = 0.f;
    for (int g0 = 0; g0 < groups; g0 += kSegs) {
      const int g = g0 + seg;
      const bool live = g < groups;
      const Side<NPER> s = side<T, W, NPER>(logits + (arow + g) * classes, live, sl, classes, unimix, keep, uni);
      const int a = live && act ? act[arow + g] : -1;
      float lp = 0.f, e = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        const int i = sl + W * j;
        lp = lp + s.logp[j] * (i < classes && i == a ? 1.f : 0.f);  // outs.py:227-228, the one-hot by comparison
        e = e + s.prob[j] * s.logp[j];                              // outs.py:231-233
      }
      lp = seg_sum<W>(lp);
      e = seg_sum<W>(e);
      if (live) {                                                  // Agg's sum over the groups, outs.py:63-64, 69-71
        row_lp = row_lp + lp;
        row_ent = row_ent - e;
      }
    }
    row_lp = across_sum<W>(row_lp);
    row_ent = across_sum<W>(row_ent);
    if (lane == 0) {
      logpi[row] = row_lp;
      ent[row] = row_ent;
      if (loss) {                                                  // agent.py:413-414
        const float w = weight ? weight[n * weight_stride + t] : 1.f;
        const float advantage = adv ? adv[row] : 1.f;
        // -(a + b) as -a - b: the same rounding, and a zero keeps the sign that makes the facade's
        // two uses exact -- actent = 0: the bits of -logpi; no action, actent = -1: the bits of ent,
        // +0 included (-(0 + -0) would be -0)
        loss[row] = w * (-(row_lp * advantage) - actent * row_ent);
      }
    }
  }
}

// NaN where the lane's group holds a NaN or +inf logit or nothing but -inf (what
// makes its softmax NaN), else 0: the gradient's first pass over a row.
template <typename T, int W, int NPER>
__device__ __forceinline__ float poison(const T* x, bool live, int sl, int classes) {
  float m = -INFINITY;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    if (live && i < classes) {
      const float v = load(x, i);
      bad = bad || v != v || v == INFINITY;
      m = fmaxf(m, v);
    }
  }
  m = seg_max<W>(m);
  return bad || (live && m == -INFINITY) ? quiet_nan() : 0.f;
}

// With a = softmax(x), p = keep a + uni, logp = log p, i the group's action,
// e = sum_k a_k logp_k and s = gout * weight, per group:
//   d logp_i / d x_j = keep a_i (delta_ij - a_j) / p_i
//   d ent / d x_j    = -keep a_j (logp_j - e)        (sum_k a_k (delta_kj - a_j) (logp_k + 1))
//   d loss / d x_j   = -s keep [adv q (delta_ij - a_j) - actent a_j (logp_j - e)],  q = a_i / p_i
// unimix == 0: keep = 1, q = 1 and e = -ent of the group.  An action outside
// [0, classes): q = 0, the entropy's term alone.
template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void policy_loss_grad_kernel(
    const T* __restrict__ logits, const int32_t* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ weight, int64_t weight_stride, const float* __restrict__ gout, T* __restrict__ grad,
    int32_t rows_in, int32_t steps, int32_t kept, int32_t groups, int32_t classes, float unimix, float actent) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows_in;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave
    const int64_t n = row / steps, t = row % steps;
    const int64_t arow = row * groups;
    if (t >= kept) {                                               // a dropped step: no gradient, its logits are not read
      const int64_t count = static_cast<int64_t>(groups) * classes;
      for (int64_t i = lane; i < count; i += kWave) store(grad + arow * classes, i, 0.f);
      continue;
    }
    float flag = 0.f;
    for (int g0 = 0; g0 < groups; g0 += kSegs) {
      const int g = g0 + seg;
      flag = flag + poison<T, W, NPER>(logits + (arow + g) * classes, g < groups, sl, classes);
    }
    flag = seg_sum<kWave>(flag);                                   // over all 64 lanes: NaN if any group's is
    const int64_t out = n * kept + t;
    const float scale = gout[out] * (weight ? weight[n * weight_stride + t] : 1.f);
    const float s = flag != flag ? flag : scale;                   // a poisoned row: NaN throughout
    const float advantage = adv ? adv[out] : 1.f;
    for (int g0 = 0; g0 < groups; g0 += kSegs) {
      const int g = g0 + seg;
      const bool live = g < groups;
      const int64_t at = (arow + g) * classes;
      const Side<NPER> p = side<T, W, NPER>(logits + at, live, sl, classes, unimix, keep, uni);
      const int a = live && act ? act[arow + g] : -1;
      float e = 0.f, q = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        const int i = sl + W * j;
        e = e + p.sm[j] * p.logp[j];
        if (i < classes && i == a) q = unimix != 0.f ? p.sm[j] / p.prob[j] : 1.f;
      }
      e = seg_sum<W>(e);
      q = seg_sum<W>(q);                                           // one lane of the segment at the most holds it
      if (live) {
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
          const int i = sl + W * j;
          if (i < classes) {
            const float hit = i == a ? 1.f : 0.f;
            const float of_logp = advantage * (q * (hit - p.sm[j]));
            const float of_ent = actent * (p.sm[j] * (p.logp[j] - e));
            store(grad + at, i, -s * (keep * (of_logp - of_ent)));
          }
        }
      }
    }
  }
}

LaunchCount g_count;

bool fits(int64_t N, int64_t T, int64_t drop, int64_t groups, int64_t classes) {
  return N >= 1 && T >= 1 && (drop == 0 || drop == 1) && groups >= 1 && classes >= 1 && classes <= kPolicyMaxClasses &&
         groups <= INT32_MAX / classes && T <= INT32_MAX / (groups * classes) &&
         N <= INT32_MAX / (T * groups * classes);
}

int row_blocks(int64_t rows) {
  const int64_t blocks = (rows + kWaves - 1) / kWaves;
  return static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

// the ladder of onehot_kl.hip's EMB_ONEHOT_BY_WIDTH: the narrowest segment that
// holds a group, then 2 or 4 values per lane of the whole wave
// (EMB_SEGMENT_BY_WIDTH of onehot_segment.h, spelled here because the sweep's cases module reads it from this file)
#define EMB_POLICY_BY_WIDTH(CALL, c)     \
  do {                                   \
    if ((c) <= 2) { CALL(2, 1); }        \
    else if ((c) <= 4) { CALL(4, 1); }   \
    else if ((c) <= 8) { CALL(8, 1); }   \
    else if ((c) <= 16) { CALL(16, 1); } \
    else if ((c) <= 32) { CALL(32, 1); } \
    else if ((c) <= 64) { CALL(64, 1); } \
    else if ((c) <= 128) { CALL(64, 2); }\
    else { CALL(64, 4); }                \
  } while (0)

}  // namespace

int64_t policy_loss_launches() { return g_count.value(); }

hipError_t launch_policy_loss(const void* logits, const int32_t* act, bool bf16, int64_t N, int64_t T, int64_t drop,
                              int64_t groups, int64_t classes, float unimix, float actent, const float* adv,
                              const float* weight, int64_t weight_stride, float* loss, float* logpi, float* ent,
                              hipStream_t stream) {
  if (!fits(N, T, drop, groups, classes) || T - drop < 1 || !logits || !logpi || !ent) return hipErrorInvalidValue;
  if (weight && weight_stride < T - drop) return hipErrorInvalidValue;
  const int64_t rows = N * (T - drop);
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), steps = static_cast<int32_t>(T), kept = static_cast<int32_t>(T - drop);
  const int32_t g = static_cast<int32_t>(groups), c = static_cast<int32_t>(classes);
#define EMB_FORWARD(W_, NPER_)                                                                                  \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((policy_loss_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                         \
                       static_cast<const bf16_t*>(logits), act, adv, weight, weight_stride, loss, logpi, ent,   \
                       r, steps, kept, g, c, unimix, actent);                                                   \
  else                                                                                                          \
    hipLaunchKernelGGL((policy_loss_kernel<float, W_, NPER_>), grid, block, 0, stream,                          \
                       static_cast<const float*>(logits), act, adv, weight, weight_stride, loss, logpi, ent,    \
                       r, steps, kept, g, c, unimix, actent)
  EMB_POLICY_BY_WIDTH(EMB_FORWARD, classes);
#undef EMB_FORWARD
  return g_count.launched();
}

hipError_t launch_policy_loss_grad(const void* logits, const int32_t* act, bool bf16, int64_t N, int64_t T,
                                   int64_t drop, int64_t groups, int64_t classes, float unimix, float actent,
                                   const float* adv, const float* weight, int64_t weight_stride, const float* gout,
                                   void* grad, hipStream_t stream) {
  if (!fits(N, T, drop, groups, classes) || !logits || !grad) return hipErrorInvalidValue;
  if (T - drop >= 1 && !gout) return hipErrorInvalidValue;
  if (weight && weight_stride < T - drop) return hipErrorInvalidValue;
  const int64_t rows = N * T;
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), steps = static_cast<int32_t>(T), kept = static_cast<int32_t>(T - drop);
  const int32_t g = static_cast<int32_t>(groups), c = static_cast<int32_t>(classes);
#define EMB_GRAD(W_, NPER_)                                                                                     \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((policy_loss_grad_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                    \
                       static_cast<const bf16_t*>(logits), act, adv, weight, weight_stride, gout,               \
                       static_cast<bf16_t*>(grad), r, steps, kept, g, c, unimix, actent);                       \
  else                                                                                                          \
    hipLaunchKernelGGL((policy_loss_grad_kernel<float, W_, NPER_>), grid, block, 0, stream,                     \
                       static_cast<const float*>(logits), act, adv, weight, weight_stride, gout,                \
                       static_cast<float*>(grad), r, steps, kept, g, c, unimix, actent)
  EMB_POLICY_BY_WIDTH(EMB_GRAD, classes);
#undef EMB_GRAD
  return g_count.launched();
}

}  // namespace emb
