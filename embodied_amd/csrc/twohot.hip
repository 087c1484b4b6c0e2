// The symexp_twohot head of DreamerV3's reward and value networks
// (embodied/jax/outs.py:273-330) as three kernels over the (rows, n) logits:
//   stats  one pass: the row's log-sum-exp and pred(), the symmetric weighted
//          average of outs.py:285-309
//   loss   two logits per row and target (the rest of the row is in lse):
//          outs.py:311-330 for up to four targets, summed with their coefficients
//   grad   one read of the logits, one write of the gradient of that sum
// With torch ops the same is a dozen passes over the logits, 16.7 MB each at the
// imagination shape (16384, 255).
//
// stats and grad: one wave64 per row, the lanes stride the row (coalesced
// dwords; a 255-float row is 1020 bytes, so rows are not 16-byte aligned and
// nothing wider is attempted), the row's values stay in registers across the
// max, sum-exp and product passes, the wave reduces by shuffles.  No atomics,
// no traffic between waves: the same bits run to run.
#include "twohot.h"
#include "wave_util.h"

// float32 operations one by one: pred()'s mirrored pair p[i] * b[i] + p[j] * b[j]
// is exactly 0 for equal p and antisymmetric bins only if neither product is
// fused into the addition.
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // rows per workgroup at a time
constexpr int kThreads = kWave * kWaves;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups of 4 waves on each of 256 CUs; more rows: grid stride

using namespace segment;                          // bf16 load / store, wave_max, wave_sum
static_assert(kWave == kLanes, "the wave helpers shuffle over one wave64");

// outs.py:314-324 from the two counts: c_le = #(bins <= t), c_gt = #(bins > t).
// A NaN target counts nothing on either side: below = 0, above = n - 1 and NaN
// weights; a target beyond an outer bin lands on it, both indices equal.
struct Spot { int below, above; float w_below, w_above; };
__device__ __forceinline__ Spot spot(int c_le, int c_gt, int n, float t, const float* bins) {
  Spot s;
  s.below = min(max(c_le - 1, 0), n - 1);
  s.above = min(max(n - c_gt, 0), n - 1);
  const bool equal = s.below == s.above;
  const float to_below = equal ? 1.f : fabsf(bins[s.below] - t);
  const float to_above = equal ? 1.f : fabsf(bins[s.above] - t);
  const float total = to_below + to_above;
  s.w_below = to_above / total;
  s.w_above = to_below / total;
  return s;
}

// NPER values per lane: n <= 64 * NPER.
template <typename T, int NPER>
__global__ __launch_bounds__(kThreads) void twohot_stats_kernel(const T* __restrict__ logits,
                                                                const float* __restrict__ bins,
                                                                float* __restrict__ lse, float* __restrict__ pred,
                                                                int32_t rows, int32_t n) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int half = n / 2;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave: the shuffles see 64 lanes
    const T* x = logits + row * n;
    float v[NPER];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = lane + kWave * j;
      v[j] = i < n ? load(x, i) : -INFINITY;
      m = fmaxf(m, v[j]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = lane + kWave * j;
      v[j] = i < n ? expf(v[j] - m) : 0.f;
      s = s + v[j];
    }
    s = wave_sum(s);
    // outs.py:292-309: every mirrored pair is formed before any other addition.
    // The partner's logit is read again (this wave has just pulled the row
    // through the cache) and its probability formed by the same operations as
    // its owner's, so equal logits give equal probabilities.
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = lane + kWave * j;
      if (i < half) {
        const int k = n - 1 - i;
        const float p = v[j] / s, q = expf(load(x, k) - m) / s;
        acc = acc + (p * bins[i] + q * bins[k]);
      }
    }
    acc = wave_sum(acc);
    if (n & 1) acc = (expf(load(x, half) - m) / s) * bins[half] + acc;
    if (lane == 0) {
      lse[row] = m + logf(s);
      pred[row] = acc;
    }
  }
}

// Four lanes per row, lane j of them target j; the bins in LDS.
template <typename T>
__global__ __launch_bounds__(kThreads) void twohot_loss_kernel(const T* __restrict__ logits,
                                                               const float* __restrict__ bins,
                                                               const float* __restrict__ lse, const TwoHotTargets tg,
                                                               float* __restrict__ loss, int32_t rows, int32_t n) {
  __shared__ float sbins[kTwoHotMaxBins];
  for (int i = threadIdx.x; i < n; i += kThreads) sbins[i] = bins[i];       // n <= kTwoHotMaxBins
  __syncthreads();
  const int sub = threadIdx.x % kTwoHotMaxTargets;
  const int first = (threadIdx.x % kWave) - sub;                            // lane of this row's target 0
  const int64_t slots = static_cast<int64_t>(rows) * kTwoHotMaxTargets;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kThreads; base < slots;
       base += static_cast<int64_t>(gridDim.x) * kThreads) {                // uniform over the workgroup
    const int64_t row = (base + threadIdx.x) / kTwoHotMaxTargets;
    float term = 0.f;
    if (row < rows && sub < tg.k) {
      const float t = tg.target[sub][row];
      int c_le = 0, c_gt = 0;
      for (int i = 0; i < n; ++i) {
        const float b = sbins[i];
        c_le += b <= t;
        c_gt += b > t;
      }
      const Spot s = spot(c_le, c_gt, n, t, sbins);
      const float l = lse[row];
      const float lo = load(logits, row * n + s.below) - l, hi = load(logits, row * n + s.above) - l;
      term = tg.coef[sub] * -(s.w_below * lo + s.w_above * hi);
    }
    float total = __shfl(term, first, kWave);
#pragma unroll
    for (int j = 1; j < kTwoHotMaxTargets; ++j) {
      const float other = __shfl(term, first + j, kWave);
      if (j < tg.k) total = total + other;
    }
    if (row < rows && sub == 0) loss[row] = total;
  }
}

template <typename T, int NPER>
__global__ __launch_bounds__(kThreads) void twohot_grad_kernel(const T* __restrict__ logits,
                                                               const float* __restrict__ bins,
                                                               const float* __restrict__ lse, const TwoHotTargets tg,
                                                               float coef_sum, const float* __restrict__ gout,
                                                               T* __restrict__ grad, int32_t rows, int32_t n) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave
    const T* x = logits + row * n;
    float v[NPER];
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = lane + kWave * j;
      v[j] = i < n ? load(x, i) : 0.f;
    }
    // where each target falls: every lane counts over its own bins, both counts
    // (each <= 1024) in one word through one reduction
    Spot spots[kTwoHotMaxTargets];
#pragma unroll
    for (int k = 0; k < kTwoHotMaxTargets; ++k) {
      if (k < tg.k) {
        const float t = tg.target[k][row];
        int counts = 0;
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
          const int i = lane + kWave * j;
          if (i < n) {
            const float b = bins[i];
            counts += (b <= t ? 1 : 0) + (b > t ? 1 << 16 : 0);
          }
        }
        counts = wave_sum(counts);
        spots[k] = spot(counts & 0xffff, counts >> 16, n, t, bins);
      }
    }
    const float l = lse[row], g = gout[row];
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = lane + kWave * j;
      if (i < n) {
        // the two-hot target as outs.py:325-327 forms it, one_hot * weight: a NaN
        // weight (a NaN target) is NaN in every bin
        float hot = 0.f;
#pragma unroll
        for (int k = 0; k < kTwoHotMaxTargets; ++k)
          if (k < tg.k) {
            const float two = (i == spots[k].below ? 1.f : 0.f) * spots[k].w_below +
                              (i == spots[k].above ? 1.f : 0.f) * spots[k].w_above;
            hot = hot + tg.coef[k] * two;
          }
        store(grad + row * n, i, g * (coef_sum * expf(v[j] - l) - hot));
      }
    }
  }
}

LaunchCount g_count;

bool fits(int64_t rows, int64_t n) {
  return rows >= 1 && n >= 1 && n <= kTwoHotMaxBins && rows <= INT32_MAX / n;
}

bool fits(const TwoHotTargets& tg) {
  if (tg.k < 1 || tg.k > kTwoHotMaxTargets) return false;
  for (int k = 0; k < tg.k; ++k)
    if (!tg.target[k]) return false;
  return true;
}

int row_blocks(int64_t rows) {
  const int64_t blocks = (rows + kWaves - 1) / kWaves;
  return static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

// the smallest of 1, 2, 4, 8, 16 values per lane that holds the row
#define EMB_TWOHOT_BY_WIDTH(CALL, n)     \
  do {                                   \
    if ((n) <= 64) { CALL(1); }          \
    else if ((n) <= 128) { CALL(2); }    \
    else if ((n) <= 256) { CALL(4); }    \
    else if ((n) <= 512) { CALL(8); }    \
    else { CALL(16); }                   \
  } while (0)

}  // namespace

int64_t twohot_launches() { return g_count.value(); }

hipError_t launch_twohot_stats(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                               float* lse, float* pred, hipStream_t stream) {
  if (!fits(rows, n) || !logits || !bins || !lse || !pred) return hipErrorInvalidValue;
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), w = static_cast<int32_t>(n);
#define EMB_STATS(NPER_)                                                                                        \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((twohot_stats_kernel<bf16_t, NPER_>), grid, block, 0, stream,                            \
                       static_cast<const bf16_t*>(logits), bins, lse, pred, r, w);                              \
  else                                                                                                          \
    hipLaunchKernelGGL((twohot_stats_kernel<float, NPER_>), grid, block, 0, stream,                             \
                       static_cast<const float*>(logits), bins, lse, pred, r, w)
  EMB_TWOHOT_BY_WIDTH(EMB_STATS, n);
#undef EMB_STATS
  return g_count.launched();
}

hipError_t launch_twohot_loss(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                              const float* lse, const TwoHotTargets& targets, float* loss, hipStream_t stream) {
  if (!fits(rows, n) || !fits(targets) || !logits || !bins || !lse || !loss) return hipErrorInvalidValue;
  const int64_t blocks = (rows * kTwoHotMaxTargets + kThreads - 1) / kThreads;
  const dim3 grid(static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), w = static_cast<int32_t>(n);
  if (bf16)
    hipLaunchKernelGGL((twohot_loss_kernel<bf16_t>), grid, block, 0, stream, static_cast<const bf16_t*>(logits), bins,
                       lse, targets, loss, r, w);
  else
    hipLaunchKernelGGL((twohot_loss_kernel<float>), grid, block, 0, stream, static_cast<const float*>(logits), bins,
                       lse, targets, loss, r, w);
  return g_count.launched();
}

hipError_t launch_twohot_grad(const void* logits, bool bf16, int64_t rows, int64_t n, const float* bins,
                              const float* lse, const TwoHotTargets& targets, const float* gout, void* grad,
                              hipStream_t stream) {
  if (!fits(rows, n) || !fits(targets) || !logits || !bins || !lse || !gout || !grad) return hipErrorInvalidValue;
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), w = static_cast<int32_t>(n);
  float coef_sum = targets.coef[0];
  for (int k = 1; k < targets.k; ++k) coef_sum = coef_sum + targets.coef[k];
#define EMB_GRAD(NPER_)                                                                                         \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((twohot_grad_kernel<bf16_t, NPER_>), grid, block, 0, stream,                             \
                       static_cast<const bf16_t*>(logits), bins, lse, targets, coef_sum, gout,                  \
                       static_cast<bf16_t*>(grad), r, w);                                                       \
  else                                                                                                          \
    hipLaunchKernelGGL((twohot_grad_kernel<float, NPER_>), grid, block, 0, stream,                              \
                       static_cast<const float*>(logits), bins, lse, targets, coef_sum, gout,                   \
                       static_cast<float*>(grad), r, w)
  EMB_TWOHOT_BY_WIDTH(EMB_GRAD, n);
#undef EMB_GRAD
  return g_count.launched();
}

}  // namespace emb
