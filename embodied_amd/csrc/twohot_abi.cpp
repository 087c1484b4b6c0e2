// emb_twohot_*: the symexp_twohot head (embodied/jax/outs.py:273-330) -- the
// rows' log-sum-exp and pred(), the loss of up to four targets, its gradient --
// as one kernel launch each (twohot.hip).  Its own translation unit, as
// dreamer_targets_abi.cpp: kernels_abi.cpp is also linked into the host
// sanitizer soak, against stand-in launchers that know nothing of this head.
#include "abi_common.h"
#include "twohot.h"

using namespace emb_abi;

namespace {

// What every entry point checks before any HIP call; false: rows == 0, nothing to do.
bool shape_ok(const char* who, int32_t dtype, int64_t rows, int64_t n) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(rows >= 0, say("negative rows"));
  need(n >= 1 && n <= emb::kTwoHotMaxBins, say("n outside 1 .. 1024, the bins one wave keeps in registers"));
  need(rows <= INT32_MAX / n, say("more than 2^31 - 1 logits"));
  return rows > 0;
}

emb::TwoHotTargets targets_of(const char* who, const void* const* targets, const float* coefs, int32_t k,
                              bool live) {
  const Who say{who};
  need(k >= 1 && k <= emb::kTwoHotMaxTargets, say("k outside 1 .. 4 targets"));
  need(targets && coefs, say("the targets or the coefs array is null"));
  emb::TwoHotTargets out{};
  out.k = k;
  for (int32_t i = 0; i < k; ++i) {
    need(!live || targets[i], say("a target is null"));
    out.target[i] = static_cast<const float*>(targets[i]);
    out.coef[i] = coefs[i];
  }
  return out;
}

}  // namespace

extern "C" {

int32_t emb_twohot_stats(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins, void* lse,
                         void* pred, void* stream) {
  return guarded([&] {
    if (!shape_ok("twohot_stats", dtype, rows, n)) return;
    need(logits && bins && lse && pred, "twohot_stats: a pointer is null");
    HIP_OK(emb::launch_twohot_stats(logits, dtype == EMB_BF16, rows, n, static_cast<const float*>(bins),
                                    static_cast<float*>(lse), static_cast<float*>(pred),
                                    static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_twohot_loss(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins,
                        const void* lse, const void* const* targets, const float* coefs, int32_t k, void* loss,
                        void* stream) {
  return guarded([&] {
    const bool live = shape_ok("twohot_loss", dtype, rows, n);
    const emb::TwoHotTargets tg = targets_of("twohot_loss", targets, coefs, k, live);
    if (!live) return;
    need(logits && bins && lse && loss, "twohot_loss: a pointer is null");
    HIP_OK(emb::launch_twohot_loss(logits, dtype == EMB_BF16, rows, n, static_cast<const float*>(bins),
                                   static_cast<const float*>(lse), tg, static_cast<float*>(loss),
                                   static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_twohot_grad(const void* logits, int32_t dtype, int64_t rows, int64_t n, const void* bins,
                        const void* lse, const void* const* targets, const float* coefs, int32_t k, const void* gout,
                        void* grad, void* stream) {
  return guarded([&] {
    const bool live = shape_ok("twohot_grad", dtype, rows, n);
    const emb::TwoHotTargets tg = targets_of("twohot_grad", targets, coefs, k, live);
    if (!live) return;
    need(logits && bins && lse && gout && grad, "twohot_grad: a pointer is null");
    HIP_OK(emb::launch_twohot_grad(logits, dtype == EMB_BF16, rows, n, static_cast<const float*>(bins),
                                   static_cast<const float*>(lse), tg, static_cast<const float*>(gout), grad,
                                   static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_twohot_launches(int64_t* count) {
  return guarded([&] {
    need(count, "twohot_launches: count is null");
    *count = emb::twohot_launches();
  });
}

}  // extern "C"
