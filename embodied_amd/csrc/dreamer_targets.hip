// imag_loss's targets (dreamerv3/agent.py:397-419) as ONE launch of one
// workgroup: de-normalise the critic's prediction with valnorm's statistics, the
// lambda-return over float continuation probabilities, the trajectory weight,
// retnorm's percentile step (the exact radix select of norm_select.h over the
// returns' keys in LDS), the advantage, advnorm's and valnorm's mean-std steps,
// the normalised advantage and the normalised, padded target.  With the
// library's separate pieces that is about a dozen dependent device operations
// for 15 360 values at the shipped shape (1024, 16); each of them is launch
// latency.  Nothing returns to the host.
//
// One workgroup, because the select wants every key in one LDS: the launch
// takes N * (T-1) <= kNormLdsMax values (scans.py composes larger ones).
#include "wave_util.h"          // LaunchCount; sets no fp-contract mode
#include "scan_segment.h"       // the scan keeps scans.hip's arithmetic (its multiply-adds may contract)
#include "dreamer_targets.h"
#include "normalize_device.h"   // from here on float32 operations one by one, as normalize.hip
#include "norm_select.h"

namespace emb {
namespace {

enum : uint32_t {
  kUpdate = 1u, kRetDebias = 2u, kValDebias = 4u, kAdvDebias = 8u, kHasVal = 16u, kHasAdv = 32u,
};

// More than the 64 bytes of the kernel-argument preload whatever is done: the
// block travels by value, as ppo_targets_kernel's.
struct DreamerArgs {
  const float* rew; const float* con; const float* pred;
  float* ret; float* weight; float* adv; float* adv_normed; float* tar_padded;
  float* rstate; float* vstate; float* astate;      // vstate / astate: null = no such normaliser
  int32_t N, T;
  float disc, lam;
  uint32_t flags;
  uint32_t k_lo, k_hi;
  float frac_lo, frac_hi;
  NormParams r, v, a;
};

// impl 'none': (offset, scale) = (0, 1)
__device__ __forceinline__ NormWords no_norm() { return {0.f, 0.f, 0.f, 0.f, 1.f}; }

// The scan op: lambda_cont_coef4's maps over tarval = pred * vscale + voffset,
// formed while loading as two float32 operations (agent.py:398-400).
struct ContTargets {
  const float* rew; const float* con; const float* pred;
  int32_t T;
  float disc, lam, voffset, vscale;
  __device__ float value(float p) const { return p * vscale + voffset; }
  __device__ float seed(int64_t b) const { return value(pred[b * T + T - 1]); }
  __device__ void coef4(int64_t b, int64_t t0, int valid, float* a, float* bc, float*) const {
    const float offset = voffset, scale = vscale;
    lambda_cont_coef4(rew, con, pred, b * T + t0, valid, disc, lam,
                      [offset, scale](float p) { return p * scale + offset; }, a, bc);
  }
};

// W lanes per row segment, four steps per lane: kNormThreads / W rows at a time,
// rows longer than 4 W steps walked in pieces with the running value carried in
// a register (the scan right to left, the weight left to right).
template <int W>
__global__ __launch_bounds__(kNormThreads) void dreamer_targets_kernel(const DreamerArgs p) {
  __shared__ uint32_t keys[kNormLdsMax];
  __shared__ uint32_t hist[2][kNormBins];
  __shared__ double sums[kNormWaves][2];
  __shared__ uint32_t sel[2][3];
  __shared__ uint32_t next_key[2];

  const uint32_t tid = threadIdx.x;
  const bool update = p.flags & kUpdate, has_val = p.flags & kHasVal, has_adv = p.flags & kHasAdv;
  const bool rdebias = p.flags & kRetDebias, vdebias = p.flags & kValDebias, adebias = p.flags & kAdvDebias;

  // 1. Every lane carries the states: read before the first barrier, written by
  // lane 0 at the end.  (voffset, vscale) as stats() forms them BEFORE the step.
  const float r0 = p.rstate[0], r1 = p.rstate[1], rc = p.rstate[2];
  float v0 = 0.f, v1 = 0.f, vc = 0.f, a0 = 0.f, a1 = 0.f, ac = 0.f;
  if (has_val) v0 = p.vstate[0], v1 = p.vstate[1], vc = p.vstate[2];
  if (has_adv) a0 = p.astate[0], a1 = p.astate[1], ac = p.astate[2];
  const NormWords before = has_val ? norm_step(v0, v1, vc, 0.f, 0.f, kNormMeanStd, false, vdebias, p.v) : no_norm();
  const ContTargets op{p.rew, p.con, p.pred, p.T, p.disc, p.lam, before.offset, before.scale};

  // 2. The scan.  Every loop bound is uniform over the workgroup (the shuffles
  // need whole segments); `valid` says what a lane owns.  ret goes to global
  // memory and, as its order-preserving key, to LDS in the same pass.
  constexpr int kSegments = kNormThreads / W, kSpan = 4 * W;
  const int64_t n = p.T - 1;
  const int sl = static_cast<int>(tid % W);
  const int64_t segment = tid / W;
  double s[2] = {0.0, 0.0};                  // sums of ret, ret^2
  for (int64_t b0 = 0; b0 < p.N; b0 += kSegments) {
    const int64_t b = b0 + segment;
    const bool row_ok = b < p.N;
    float carry = row_ok ? op.seed(b) : 0.f;
    for (int64_t base = ((n - 1) / kSpan) * kSpan; base >= 0; base -= kSpan) {
      const int64_t t0 = base + 4 * sl;
      const int64_t left = n - t0;
      const int valid = row_ok ? (left >= 4 ? 4 : (left > 0 ? static_cast<int>(left) : 0)) : 0;
      float y[4], keep[4];
      scan_piece4<W>(op, b, t0, valid, sl, [&] { return carry; }, y, keep);
      if (valid > 0) emb::store4(p.ret + b * n + t0, valid, y);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < valid) {
          keys[b * n + t0 + k] = to_key(y[k]);               // b < N, t0 + k < n: below N * n <= kNormLdsMax
          s[0] += static_cast<double>(y[k]);
          s[1] += static_cast<double>(y[k] * y[k]);          // squares in float32, as jnp.square
        }
      carry = __shfl(y[0], 0, W);            // y at `base`: the seed of the piece to the left
    }
  }

  // 3. weight = cumprod(disc * con, 1) / disc: a left-to-right product, one
  // rounding per multiply, in numpy.cumprod's order.  The lanes of a segment
  // take their turn one after the other: all of them multiply the running
  // product `run` into their own four factors, the lane whose turn it is keeps
  // the result and hands its last product on.  (Factors right of the row's end
  // are 1, so the fourth product is always the last valid one.)  Independent of
  // the scan; it re-reads what the scan has just pulled through the cache.
  for (int64_t b0 = 0; b0 < p.N; b0 += kSegments) {
    const int64_t b = b0 + segment;
    const bool row_ok = b < p.N;
    float run = 1.f;
    for (int64_t base = 0; base < p.T; base += kSpan) {
      const int64_t t0 = base + 4 * sl;
      const int64_t left = p.T - t0;
      const int valid = row_ok ? (left >= 4 ? 4 : (left > 0 ? static_cast<int>(left) : 0)) : 0;
      float x[4] = {1.f, 1.f, 1.f, 1.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
      if (valid > 0) {
        float c[4];
        load4(p.con + b * p.T + t0, valid, c);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < valid) x[k] = p.disc * c[k];
      }
      // (not unrolled all the way: the W shuffle addresses of a full unroll are
      // hoisted into W registers, which spills at W >= 32)
#pragma unroll 4
      for (int turn = 0; turn < W; ++turn) {
        const float o0 = run * x[0], o1 = o0 * x[1], o2 = o1 * x[2], o3 = o2 * x[3];
        if (sl == turn) w[0] = o0, w[1] = o1, w[2] = o2, w[3] = o3;
        run = __shfl(o3, turn, W);
      }
      if (valid > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = w[k] / p.disc;
        emb::store4(p.weight + b * p.T + t0, valid, w);
      }
    }
  }

  // 4. valnorm takes its step from ret (agent.py:417).  The barrier (the
  // reduction's, or the bare one) also puts every key write of phase 2 before
  // the reads of phases 5 and 6.
  const uint32_t total = static_cast<uint32_t>(p.N) * static_cast<uint32_t>(n);
  const double count = static_cast<double>(total);
  NormWords vw = before;
  if (has_val && update) {
    norm_block_sum(s, sums);
    vw = norm_step(v0, v1, vc, static_cast<float>(s[0] / count), static_cast<float>(s[1] / count),
                   kNormMeanStd, true, vdebias, p.v);
  } else {
    __syncthreads();
  }

  // 5. retnorm: two percentiles of the keys in LDS, then the EMA step:
  // (roffset, rscale) AFTER the update, as agent.py:407-408 uses them.  (The
  // select's barriers also separate the two uses of `sums`.)
  NormPair picked = {0.f, 0.f};
  if (update) picked = norm_select2(keys, total, p.k_lo, p.k_hi, p.frac_lo, p.frac_hi, hist, sel, next_key);
  const NormWords rw = norm_step(r0, r1, rc, picked.new0, picked.new1, kNormPerc, update, rdebias, p.r);

  // 6. Over the (N, T) cells: cell i = (b, t) owns ret[b * (T-1) + t] = ret[i - b]
  // (out of LDS: key -> float is exact) and pred[i].  adv = (ret - tarval) / rscale;
  // tar_padded with its zero last column; adv_normed too where advnorm's
  // statistics do not wait for this batch (none, or no update).
  const bool adv_late = has_adv && update;
  NormWords aw = has_adv ? norm_step(a0, a1, ac, 0.f, 0.f, kNormMeanStd, false, adebias, p.a) : no_norm();
  {
    const uint32_t T = static_cast<uint32_t>(p.T), cells = static_cast<uint32_t>(p.N) * T;
    const float rscale = rw.scale, voffset = vw.offset, vscale = vw.scale;
    const float aoffset = aw.offset, ascale = aw.scale;
    double sa[2] = {0.0, 0.0};               // sums of adv, adv^2
    for (uint32_t i = tid; i < cells; i += kNormThreads) {
      const uint32_t b = i / T, t = i - b * T;
      float padded = 0.f;
      if (t + 1 < T) {
        const uint32_t j = i - b;
        const float r = from_key(keys[j]);
        const float a = (r - op.value(p.pred[i])) / rscale;
        p.adv[j] = a;
        if (adv_late) {
          sa[0] += static_cast<double>(a);
          sa[1] += static_cast<double>(a * a);
        } else {
          p.adv_normed[j] = (a - aoffset) / ascale;
        }
        padded = (r - voffset) / vscale;
      }
      p.tar_padded[i] = padded;
    }
    // 7. advnorm's step from adv, then the normalised advantage.  The barrier
    // inside the reduction puts every store of adv before the reads below.
    if (adv_late) {
      norm_block_sum(sa, sums);
      aw = norm_step(a0, a1, ac, static_cast<float>(sa[0] / count), static_cast<float>(sa[1] / count),
                     kNormMeanStd, true, adebias, p.a);
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
  }

  // 8. The states.
  if (tid == 0) {
    norm_store(p.rstate, rw, update, rdebias);
    if (has_val) norm_store(p.vstate, vw, update, vdebias);
    if (has_adv) norm_store(p.astate, aw, update, adebias);
  }
}

segment::LaunchCount g_count;

}  // namespace

int64_t dreamer_targets_launches() { return g_count.value(); }

hipError_t launch_dreamer_targets(const float* rew, const float* con, const float* pred, int64_t N, int64_t T,
                                  float disc, float lam, bool update, float* ret, float* weight, float* adv,
                                  float* adv_normed, float* tar_padded, const DreamerNorm& retnorm,
                                  const DreamerNorm& valnorm, const DreamerNorm& advnorm, hipStream_t stream) {
  if (N < 1 || T < 2 || T - 1 > kNormLdsMax || N > kNormLdsMax / (T - 1)) return hipErrorInvalidValue;
  if (retnorm.impl != kNormPerc || !retnorm.state) return hipErrorInvalidValue;
  for (const DreamerNorm* norm : {&valnorm, &advnorm})
    if (norm->impl != 0 && (norm->impl != kNormMeanStd || !norm->state)) return hipErrorInvalidValue;
  const int64_t n = T - 1;
  if (retnorm.lo.k >= N * n || retnorm.hi.k >= N * n) return hipErrorInvalidValue;    // ranks index the keys
  DreamerArgs p;
  p.rew = rew; p.con = con; p.pred = pred;
  p.ret = ret; p.weight = weight; p.adv = adv; p.adv_normed = adv_normed; p.tar_padded = tar_padded;
  p.rstate = retnorm.state;
  p.vstate = valnorm.impl ? valnorm.state : nullptr;
  p.astate = advnorm.impl ? advnorm.state : nullptr;
  p.N = static_cast<int32_t>(N); p.T = static_cast<int32_t>(T);
  p.disc = disc; p.lam = lam;
  p.flags = (update ? kUpdate : 0u) | (retnorm.debias ? kRetDebias : 0u) | (valnorm.debias ? kValDebias : 0u) |
            (advnorm.debias ? kAdvDebias : 0u) | (valnorm.impl ? kHasVal : 0u) | (advnorm.impl ? kHasAdv : 0u);
  p.k_lo = retnorm.lo.k; p.k_hi = retnorm.hi.k;
  p.frac_lo = retnorm.lo.frac; p.frac_hi = retnorm.hi.frac;
  p.r = NormParams{retnorm.keep, retnorm.rate, retnorm.limit};
  p.v = NormParams{valnorm.keep, valnorm.rate, valnorm.limit};
  p.a = NormParams{advnorm.keep, advnorm.rate, advnorm.limit};
  // the segment widths of scans.hip's launch_scan; longer rows are walked in pieces of 256 steps
  const int W = n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64;
#define EMB_DREAMER_TARGETS(W_) \
  hipLaunchKernelGGL((dreamer_targets_kernel<W_>), dim3(1), dim3(kNormThreads), 0, stream, p)
  switch (W) {
    case 4: EMB_DREAMER_TARGETS(4); break;
    case 8: EMB_DREAMER_TARGETS(8); break;
    case 16: EMB_DREAMER_TARGETS(16); break;
    case 32: EMB_DREAMER_TARGETS(32); break;
    default: EMB_DREAMER_TARGETS(64); break;
  }
#undef EMB_DREAMER_TARGETS
  return g_count.launched();
}

}  // namespace emb
