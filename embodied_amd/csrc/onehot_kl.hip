// The KL pair of DreamerV3's world model, RSSM.loss (dreamerv3/rssm.py:123-132)
// over _dist = Agg(OneHot(logits, unimix), 1, sum) (rssm.py:173-176,
// embodied/jax/outs.py:40-76, 208-263), as two kernels over the two
// (rows, stoch, classes) logit tensors:
//   forward  one read of post and prior: per row the raw kl (dyn and rep have
//            the same value, sg only routes gradients), max(kl, free_nats) and
//            both entropies
//   grad     one more read, the closed-form gradients of rep with respect to
//            post and of dyn with respect to prior, the maximum's gradient
//            taken from the saved kl
// With torch ops the same is several dozen passes over both tensors.
//
// One wave64 per row.  A group of `classes` logits occupies a segment of W
// lanes, W the next power of two >= classes (2 .. 64), so a wave works on
// 64 / W groups at a time; 65 .. 256 classes: the whole wave on one group with 2
// or 4 values per lane.  Lanes past `classes` and segments past `stoch`
// contribute nothing.  Reductions are butterflies inside a segment; a row's sum
// over its groups is each segment's running sum in the order of the groups,
// then one butterfly across the segments.  No atomics, no traffic between
// waves: the same bits run to run.
#include "onehot_kl.h"
#include "onehot_segment.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // rows per workgroup at a time
constexpr int kThreads = kWave * kWaves;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups of 4 waves on each of 256 CUs; more rows: grid stride

// bf16_t, load / store, seg_max / seg_sum / across_sum, Side and side(): onehot_segment.h
using namespace segment;
static_assert(kWave == kLanes, "the segment helpers shuffle over one wave64");

template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void onehot_kl_kernel(const T* __restrict__ post, const T* __restrict__ prior,
                                                             float* __restrict__ kl, float* __restrict__ ent_post,
                                                             float* __restrict__ ent_prior, float* __restrict__ dyn,
                                                             float* __restrict__ rep, int32_t rows, int32_t stoch,
                                                             int32_t classes, float unimix, float free_nats) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));     // outs.py:214-215
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave: the shuffles see 64 lanes
    const int64_t base = row * stoch * classes;
    float row_kl = 0.f, row_ep = 0.f, row_eq = 0.f;
    for (int g0 = 0; g0 < stoch; g0 += kSegs) {
      const int g = g0 + seg;
      const bool live = g < stoch;
      const int64_t at = base + static_cast<int64_t>(g) * classes;
      const Side<NPER> p = side<T, W, NPER>(post + at, live, sl, classes, unimix, keep, uni);
      const Side<NPER> q = side<T, W, NPER>(prior + at, live, sl, classes, unimix, keep, uni);
      float k = 0.f, ep = 0.f, eq = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        k = k + p.prob[j] * (p.logp[j] - q.logp[j]);               // outs.py:236-240
        ep = ep + p.prob[j] * p.logp[j];                           // outs.py:230-234
        eq = eq + q.prob[j] * q.logp[j];
      }
      k = seg_sum<W>(k);
      ep = seg_sum<W>(ep);
      eq = seg_sum<W>(eq);
      if (live) {                                                  // Agg's sum over the groups, outs.py:69-76
        row_kl = row_kl + k;
        row_ep = row_ep - ep;
        row_eq = row_eq - eq;
      }
    }
    row_kl = across_sum<W>(row_kl);
    row_ep = across_sum<W>(row_ep);
    row_eq = across_sum<W>(row_eq);
    if (lane == 0) {
      kl[row] = row_kl;
      ent_post[row] = row_ep;
      ent_prior[row] = row_eq;
      // rssm.py:127-129; a NaN stays one, as jnp.maximum keeps it
      const float loss = free_nats != 0.f && row_kl == row_kl ? fmaxf(row_kl, free_nats) : row_kl;
      if (dyn) dyn[row] = loss;
      if (rep) rep[row] = loss;
    }
  }
}

// With a = softmax(post), b = softmax(prior), p = keep a + uni, q = keep b + uni,
// d = log p - log q, per group:
//   d kl / d post_j  = keep a_j (d_j - sum_k a_k d_k)
//   d kl / d prior_j = keep b_j (sum_k b_k p_k / q_k - p_j / q_j)
// (the chain through log((1 - u) softmax + u / c); each is "t_j - softmax_j sum t").
// unimix == 0: a_j (d_j - kl) and b_j - a_j, which needs no quotient.
template <typename T, int W, int NPER>
__global__ __launch_bounds__(kThreads) void onehot_kl_grad_kernel(
    const T* __restrict__ post, const T* __restrict__ prior, const float* __restrict__ kl,
    const float* __restrict__ g_rep, const float* __restrict__ g_dyn, T* __restrict__ grad_post,
    T* __restrict__ grad_prior, int32_t rows, int32_t stoch, int32_t classes, float unimix, float free_nats) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % W, seg = lane / W;
  const float keep = 1.f - unimix, uni = unimix * (1.f / static_cast<float>(classes));
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {          // uniform over the wave
    // the gradient of rssm.py:127-129's maximum, from the kl the forward saved;
    // a NaN kl (a poisoned row) is on neither side: the whole row's gradient is NaN
    const float k = kl[row];
    float f = k == k ? 1.f : k;
    if (free_nats != 0.f) f = k > free_nats ? 1.f : k < free_nats ? 0.f : k == free_nats ? 0.5f : k;
    const float gp = grad_post ? g_rep[row] * f : 0.f;
    const float gq = grad_prior ? g_dyn[row] * f : 0.f;
    const int64_t base = row * stoch * classes;
    for (int g0 = 0; g0 < stoch; g0 += kSegs) {
      const int g = g0 + seg;
      const bool live = g < stoch;
      const int64_t at = base + static_cast<int64_t>(g) * classes;
      const Side<NPER> p = side<T, W, NPER>(post + at, live, sl, classes, unimix, keep, uni);
      const Side<NPER> q = side<T, W, NPER>(prior + at, live, sl, classes, unimix, keep, uni);
      float d[NPER], r[NPER];
      float sum_ad = 0.f, sum_br = 0.f;
#pragma unroll
      for (int j = 0; j < NPER; ++j) {
        const bool ok = sl + W * j < classes;
        d[j] = p.logp[j] - q.logp[j];
        r[j] = ok && unimix != 0.f ? p.prob[j] / q.prob[j] : 0.f;
        sum_ad = sum_ad + p.sm[j] * d[j];
        sum_br = sum_br + q.sm[j] * r[j];
      }
      sum_ad = seg_sum<W>(sum_ad);
      sum_br = seg_sum<W>(sum_br);
      if (live) {
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
          const int i = sl + W * j;
          if (i < classes) {
            if (grad_post) store(grad_post + at, i, gp * (keep * (p.sm[j] * (d[j] - sum_ad))));
            if (grad_prior)
              store(grad_prior + at, i,
                    gq * (unimix != 0.f ? keep * (q.sm[j] * (sum_br - r[j])) : q.sm[j] - p.sm[j]));
          }
        }
      }
    }
  }
}

LaunchCount g_count;

bool fits(int64_t rows, int64_t stoch, int64_t classes) {
  return rows >= 1 && stoch >= 1 && classes >= 1 && classes <= kOneHotMaxClasses &&
         stoch <= INT32_MAX / classes && rows <= INT32_MAX / (stoch * classes);
}

int row_blocks(int64_t rows) {
  const int64_t blocks = (rows + kWaves - 1) / kWaves;
  return static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

// the narrowest segment that holds a group, then 2 or 4 values per lane of the whole wave
// (EMB_SEGMENT_BY_WIDTH of onehot_segment.h, spelled here because the sweep's cases module reads it from this file)
#define EMB_ONEHOT_BY_WIDTH(CALL, c)     \
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

int64_t onehot_kl_launches() { return g_count.value(); }

hipError_t launch_onehot_kl(const void* post, const void* prior, bool bf16, int64_t rows, int64_t stoch,
                            int64_t classes, float unimix, float free_nats, float* kl, float* ent_post,
                            float* ent_prior, float* dyn, float* rep, hipStream_t stream) {
  if (!fits(rows, stoch, classes) || !post || !prior || !kl || !ent_post || !ent_prior) return hipErrorInvalidValue;
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), s = static_cast<int32_t>(stoch), c = static_cast<int32_t>(classes);
#define EMB_FORWARD(W_, NPER_)                                                                                  \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((onehot_kl_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                           \
                       static_cast<const bf16_t*>(post), static_cast<const bf16_t*>(prior), kl, ent_post,       \
                       ent_prior, dyn, rep, r, s, c, unimix, free_nats);                                        \
  else                                                                                                          \
    hipLaunchKernelGGL((onehot_kl_kernel<float, W_, NPER_>), grid, block, 0, stream,                            \
                       static_cast<const float*>(post), static_cast<const float*>(prior), kl, ent_post,         \
                       ent_prior, dyn, rep, r, s, c, unimix, free_nats)
  EMB_ONEHOT_BY_WIDTH(EMB_FORWARD, classes);
#undef EMB_FORWARD
  return g_count.launched();
}

hipError_t launch_onehot_kl_grad(const void* post, const void* prior, bool bf16, int64_t rows, int64_t stoch,
                                 int64_t classes, float unimix, float free_nats, const float* kl,
                                 const float* g_rep, const float* g_dyn, void* grad_post, void* grad_prior,
                                 hipStream_t stream) {
  if (!fits(rows, stoch, classes) || !post || !prior || !kl) return hipErrorInvalidValue;
  if ((!grad_post && !grad_prior) || (grad_post && !g_rep) || (grad_prior && !g_dyn)) return hipErrorInvalidValue;
  const dim3 grid(row_blocks(rows)), block(kThreads);
  const int32_t r = static_cast<int32_t>(rows), s = static_cast<int32_t>(stoch), c = static_cast<int32_t>(classes);
#define EMB_GRAD(W_, NPER_)                                                                                     \
  if (bf16)                                                                                                     \
    hipLaunchKernelGGL((onehot_kl_grad_kernel<bf16_t, W_, NPER_>), grid, block, 0, stream,                      \
                       static_cast<const bf16_t*>(post), static_cast<const bf16_t*>(prior), kl, g_rep, g_dyn,   \
                       static_cast<bf16_t*>(grad_post), static_cast<bf16_t*>(grad_prior), r, s, c, unimix,      \
                       free_nats);                                                                              \
  else                                                                                                          \
    hipLaunchKernelGGL((onehot_kl_grad_kernel<float, W_, NPER_>), grid, block, 0, stream,                       \
                       static_cast<const float*>(post), static_cast<const float*>(prior), kl, g_rep, g_dyn,     \
                       static_cast<float*>(grad_post), static_cast<float*>(grad_prior), r, s, c, unimix,        \
                       free_nats)
  EMB_ONEHOT_BY_WIDTH(EMB_GRAD, classes);
#undef EMB_GRAD
  return g_count.launched();
}

}  // namespace emb
