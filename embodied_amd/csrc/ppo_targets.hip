// The top of ppo_loss (ppo/agent.py:188-210) as ONE launch of one workgroup:
// de-normalise the critic's prediction with valnorm's statistics, GAE, both
// mean-std normalisers' EMA step (embodied/jax/utils.py:44-74), the clipped and
// padded normalised target and the normalised advantage.  With the library's
// separate pieces that is three dependent launches (scans.hip's GAE, two of
// normalize.hip) and four torch ops; at PPO's sizes each of them is launch
// latency.  Nothing returns to the host.
//
// One workgroup is the right shape while B * T is small (the statistics are
// four sums, so nothing has to cross workgroups); the kernel stays correct at
// every size, it just stops being fast (scans.py holds the crossover).
#include "wave_util.h"          // LaunchCount; sets no fp-contract mode
#include "scan_segment.h"       // the scan keeps scans.hip's arithmetic (its multiply-adds may contract)
#include "ppo_targets.h"
#include "normalize_device.h"   // from here on float32 operations one by one, as normalize.hip

namespace emb {
namespace {

// More than the 64 bytes of the kernel-argument preload whatever is done: the
// block travels by value, as lambda_multi_kernel's.
struct PpoArgs {
  const float* rew; const float* pred; const uint8_t* last; const uint8_t* term;
  float* adv; float* tar; float* tar_normed; float* adv_normed;
  float* vstate; float* astate;
  int32_t B, T;
  float live_scale, lam, tarclip;
  uint32_t flags;              // 1: update, 2: valnorm debiases, 4: advnorm debiases
  NormParams v, a;
};

// The scan op of the PPO targets: GaeOp's maps (scan_segment.h gae_coef4) over
// val = pred * vscale + voffset, formed while loading as two float32
// operations (ppo/agent.py:192).  What a scan op of this kernel provides:
// seed, coef4, and store4 that also hands back the second stored array.
struct GaeTargets {
  const float* rew; const float* pred; const uint8_t* last; const uint8_t* term;
  float* adv; float* tar;
  int32_t T;
  float live_scale, lam, voffset, vscale;
  __device__ GaeTargets(const PpoArgs& p, float voffset_, float vscale_)
      : rew(p.rew), pred(p.pred), last(p.last), term(p.term), adv(p.adv), tar(p.tar), T(p.T),
        live_scale(p.live_scale), lam(p.lam), voffset(voffset_), vscale(vscale_) {}
  __device__ float seed(int64_t) const { return 0.f; }
  __device__ void coef4(int64_t b, int64_t t0, int valid, float* a, float* bc, float* keep) const {
    const int64_t i = b * T + t0;
    const float offset = voffset, scale = vscale;
    gae_coef4(pred, i, rew, i, term, last, i, valid, live_scale, lam,
              [offset, scale](float p) { return p * scale + offset; }, a, bc, keep);
  }
  // adv = y and tar = y + val (keep), each (B, T-1); z receives tar.
  __device__ void store4(int64_t b, int64_t t0, int valid, const float* y, const float* keep, float* z) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = y[k] + keep[k];
    emb::store4(adv + b * (T - 1) + t0, valid, y);
    emb::store4(tar + b * (T - 1) + t0, valid, z);
  }
};

// W lanes per row segment, four steps per lane: kNormThreads / W rows at a time,
// rows longer than 4 W steps walked right to left with y carried in a register.
template <typename Op, int W>
__global__ __launch_bounds__(kNormThreads) void ppo_targets_kernel(const PpoArgs p) {
  __shared__ double sums[kNormWaves][4];
  const uint32_t tid = threadIdx.x;
  const bool update = p.flags & 1u, vdebias = p.flags & 2u, adebias = p.flags & 4u;

  // 1. Every lane carries both states: read before the first barrier, written by
  // lane 0 after it.  (voffset, vscale) as stats() forms them BEFORE the step.
  const float v0 = p.vstate[0], v1 = p.vstate[1], vc = p.vstate[2];
  const float a0 = p.astate[0], a1 = p.astate[1], ac = p.astate[2];
  const NormWords before = norm_step(v0, v1, vc, 0.f, 0.f, kNormMeanStd, false, vdebias, p.v);
  const Op op(p, before.offset, before.scale);

  // 2. The scan.  Every loop bound is uniform over the workgroup (the shuffles
  // need whole segments); `valid` says what a lane owns.
  constexpr int kSegments = kNormThreads / W, kSpan = 4 * W;
  const int64_t n = p.T - 1;
  const int sl = static_cast<int>(tid % W);
  const int64_t segment = tid / W;
  double s[4] = {0.0, 0.0, 0.0, 0.0};        // sums of adv, adv^2, tar, tar^2
  for (int64_t b0 = 0; b0 < p.B; b0 += kSegments) {
    const int64_t b = b0 + segment;
    const bool row_ok = b < p.B;
    float carry = row_ok ? op.seed(b) : 0.f;
    for (int64_t base = ((n - 1) / kSpan) * kSpan; base >= 0; base -= kSpan) {
      const int64_t t0 = base + 4 * sl;
      const int64_t left = n - t0;
      const int valid = row_ok ? (left >= 4 ? 4 : (left > 0 ? static_cast<int>(left) : 0)) : 0;
      float y[4], z[4] = {0.f, 0.f, 0.f, 0.f}, keep[4] = {0.f, 0.f, 0.f, 0.f};
      scan_piece4<W>(op, b, t0, valid, sl, [&] { return carry; }, y, keep);
      if (valid > 0) op.store4(b, t0, valid, y, keep, z);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < valid) {
          s[0] += static_cast<double>(y[k]);
          s[1] += static_cast<double>(y[k] * y[k]);        // squares in float32, as jnp.square
          s[2] += static_cast<double>(z[k]);
          s[3] += static_cast<double>(z[k] * z[k]);
        }
      carry = __shfl(y[0], 0, W);            // y at `base`: the seed of the piece to the left
    }
  }

  // 3. The batch means and both normalisers' step.  The barrier inside the
  // reduction also puts every store of adv and tar before the reads of phase 4.
  norm_block_sum(s, sums);
  const double count = static_cast<double>(p.B) * static_cast<double>(n);
  const NormWords vw = norm_step(v0, v1, vc, static_cast<float>(s[2] / count), static_cast<float>(s[3] / count),
                                 kNormMeanStd, update, vdebias, p.v);
  const NormWords aw = norm_step(a0, a1, ac, static_cast<float>(s[0] / count), static_cast<float>(s[1] / count),
                                 kNormMeanStd, update, adebias, p.a);
  if (tid == 0) {
    norm_store(p.vstate, vw, update, vdebias);
    norm_store(p.astate, aw, update, adebias);
  }

  // 4. Normalise what this workgroup stored (B * T <= INT32_MAX: 32-bit indices).
  const uint32_t total = static_cast<uint32_t>(p.B) * static_cast<uint32_t>(n);
  {
    const float offset = aw.offset, scale = aw.scale;
    const bool wide = ((reinterpret_cast<uintptr_t>(p.adv) | reinterpret_cast<uintptr_t>(p.adv_normed)) & 15) == 0;
    const uint32_t n4 = wide ? total / 4 : 0;
    for (uint32_t i = tid; i < n4; i += kNormThreads) {
      const float4 x = reinterpret_cast<const float4*>(p.adv)[i];
      reinterpret_cast<float4*>(p.adv_normed)[i] = make_float4(
          (x.x - offset) / scale, (x.y - offset) / scale, (x.z - offset) / scale, (x.w - offset) / scale);
    }
    for (uint32_t i = n4 * 4 + tid; i < total; i += kNormThreads) p.adv_normed[i] = (p.adv[i] - offset) / scale;
  }
  {
    // (B, T) with a zero last column: cell i = (b, t) reads tar[b * (T-1) + t] = tar[i - b]
    const float offset = vw.offset, scale = vw.scale, clip = p.tarclip;
    const uint32_t T = static_cast<uint32_t>(p.T), cells = static_cast<uint32_t>(p.B) * T;
    for (uint32_t i = tid; i < cells; i += kNormThreads) {
      const uint32_t b = i / T, t = i - b * T;
      float out = 0.f;
      if (t + 1 < T) {
        out = (p.tar[i - b] - offset) / scale;
        if (clip != 0.f) out = out < -clip ? -clip : (out > clip ? clip : out);     // NaN stays NaN, as jnp.clip
      }
      p.tar_normed[i] = out;
    }
  }
}

segment::LaunchCount g_count;

}  // namespace

int64_t ppo_targets_launches() { return g_count.value(); }

hipError_t launch_ppo_targets(const float* rew, const float* pred, const uint8_t* last, const uint8_t* term,
                              int64_t B, int64_t T, float live_scale, float lam, float tarclip, bool update,
                              float* adv, float* tar, float* tar_normed, float* adv_normed,
                              const PpoNorm& valnorm, const PpoNorm& advnorm, hipStream_t stream) {
  if (B < 1 || T < 2 || T > INT32_MAX || B > INT32_MAX / T) return hipErrorInvalidValue;
  PpoArgs p;
  p.rew = rew; p.pred = pred; p.last = last; p.term = term;
  p.adv = adv; p.tar = tar; p.tar_normed = tar_normed; p.adv_normed = adv_normed;
  p.vstate = valnorm.state; p.astate = advnorm.state;
  p.B = static_cast<int32_t>(B); p.T = static_cast<int32_t>(T);
  p.live_scale = live_scale; p.lam = lam; p.tarclip = tarclip;
  p.flags = (update ? 1u : 0u) | (valnorm.debias ? 2u : 0u) | (advnorm.debias ? 4u : 0u);
  p.v = NormParams{valnorm.keep, valnorm.rate, valnorm.limit};
  p.a = NormParams{advnorm.keep, advnorm.rate, advnorm.limit};
  const int64_t n = T - 1;
  // the segment widths of scans.hip's launch_scan; longer rows are walked in pieces of 256 steps
  const int W = n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64;
#define EMB_PPO_TARGETS(W_) \
  hipLaunchKernelGGL((ppo_targets_kernel<GaeTargets, W_>), dim3(1), dim3(kNormThreads), 0, stream, p)
  switch (W) {
    case 4: EMB_PPO_TARGETS(4); break;
    case 8: EMB_PPO_TARGETS(8); break;
    case 16: EMB_PPO_TARGETS(16); break;
    case 32: EMB_PPO_TARGETS(32); break;
    default: EMB_PPO_TARGETS(64); break;
  }
#undef EMB_PPO_TARGETS
  return g_count.launched();
}

}  // namespace emb
