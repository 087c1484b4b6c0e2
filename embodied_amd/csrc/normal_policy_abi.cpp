// emb_normal_policy_loss*, emb_normal_sample, emb_philox_normal: the actor's loss
// of imag_loss (dreamerv3/agent.py:411-415) over Agg(Normal(mean, stddev), dims, sum)
// (embodied/jax/outs.py:40-76, 161-186) as Head.bounded_normal / Head.normal_logstd
// build it (embodied/jax/heads.py:146-162) -- the rows' logpi, entropy and policy
// loss in one kernel launch, both gradients in one more, the draw in one
// (normal_policy.hip).  Its own translation unit, as policy_loss_abi.cpp:
// kernels_abi.cpp is also linked into the host sanitizer soak, against stand-in
// launchers that know nothing of these kernels.
#include "abi_common.h"
#include "normal_policy.h"

using namespace emb_abi;

namespace {

int kind_of(int32_t kind) { return kind == EMB_NORMAL_LOGSTD ? emb::kNormalLogstd : emb::kNormalBounded; }

void head_ok(const char* who, int32_t dtype, int32_t kind, float lo, float hi) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(kind == EMB_NORMAL_BOUNDED || kind == EMB_NORMAL_LOGSTD, say("kind must be EMB_NORMAL_BOUNDED or EMB_NORMAL_LOGSTD"));
  if (kind == EMB_NORMAL_BOUNDED)
    need(lo > 0.f && hi >= lo && hi - hi == 0.f, say("bounded needs finite hi >= lo > 0"));
}

// What both loss entry points check before any HIP call; returns the number of output rows.
int64_t shape_ok(const char* who, int32_t dtype, int64_t N, int64_t T, int32_t drop, int64_t A, int32_t kind, float lo,
                 float hi, float actent) {
  const Who say{who};
  head_ok(who, dtype, kind, lo, hi);
  need(N >= 0 && T >= 0, say("negative N or T"));
  need(drop == 0 || drop == 1, say("drop must be 0 or 1"));
  need(A >= 1 && A <= emb::kNormalMaxActions, say("A outside 1 .. 256, the row one wave keeps in registers"));
  need(T == 0 || (T <= INT32_MAX / A && N <= INT32_MAX / (T * A)), say("more than 2^31 - 1 elements"));
  need(actent - actent == 0.f, say("actent must be finite"));                   // a NaN or an infinity fails
  return T > drop ? N * (T - drop) : 0;
}

}  // namespace

extern "C" {

int32_t emb_normal_policy_loss(const void* mean_raw, const void* std_raw, const void* act, int32_t dtype, int64_t N,
                               int64_t T, int32_t drop, int64_t A, int32_t kind, float lo, float hi, float actent,
                               const void* adv, const void* weight, int64_t weight_stride, void* loss, void* logpi,
                               void* ent, void* stream) {
  return guarded([&] {
    if (!shape_ok("normal_policy_loss", dtype, N, T, drop, A, kind, lo, hi, actent)) return;
    need(mean_raw && std_raw, "normal_policy_loss: a pointer is null");
    need(loss || logpi || ent, "normal_policy_loss: loss, logpi and ent are all null");
    need(!weight || weight_stride >= T - drop, "normal_policy_loss: weight_stride below T - drop");
    HIP_OK(emb::launch_normal_policy_loss(mean_raw, std_raw, static_cast<const float*>(act), dtype == EMB_BF16, N, T,
                                          drop, A, kind_of(kind), lo, hi, actent, static_cast<const float*>(adv),
                                          static_cast<const float*>(weight), weight_stride, static_cast<float*>(loss),
                                          static_cast<float*>(logpi), static_cast<float*>(ent),
                                          static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_normal_policy_loss_grad(const void* mean_raw, const void* std_raw, const void* act, int32_t dtype,
                                    int64_t N, int64_t T, int32_t drop, int64_t A, int32_t kind, float lo, float hi,
                                    float actent, const void* adv, const void* weight, int64_t weight_stride,
                                    const void* gout, void* grad_mean, void* grad_std, void* stream) {
  return guarded([&] {
    const int64_t rows = shape_ok("normal_policy_loss_grad", dtype, N, T, drop, A, kind, lo, hi, actent);
    if (N * T == 0) return;                                  // no inputs, no gradient
    need(mean_raw && std_raw && grad_mean && grad_std, "normal_policy_loss_grad: a pointer is null");
    need(rows == 0 || gout, "normal_policy_loss_grad: gout is null");
    need(!weight || weight_stride >= T - drop, "normal_policy_loss_grad: weight_stride below T - drop");
    HIP_OK(emb::launch_normal_policy_loss_grad(mean_raw, std_raw, static_cast<const float*>(act), dtype == EMB_BF16, N,
                                               T, drop, A, kind_of(kind), lo, hi, actent,
                                               static_cast<const float*>(adv), static_cast<const float*>(weight),
                                               weight_stride, static_cast<const float*>(gout), grad_mean, grad_std,
                                               static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_normal_sample(const void* mean_raw, const void* std_raw, int32_t dtype, int64_t rows, int64_t A,
                          int32_t kind, float lo, float hi, uint64_t seed, uint64_t offset, const void* eps, void* act,
                          void* stream) {
  return guarded([&] {
    head_ok("normal_sample", dtype, kind, lo, hi);
    need(rows >= 0, "normal_sample: negative rows");
    need(A >= 1, "normal_sample: A must be at least 1");
    need(rows <= INT32_MAX / A, "normal_sample: more than 2^31 - 1 elements");
    if (rows == 0) return;
    need(mean_raw && std_raw && act, "normal_sample: a pointer is null");
    HIP_OK(emb::launch_normal_sample(mean_raw, std_raw, dtype == EMB_BF16, rows, A, kind_of(kind), lo, hi, seed, offset,
                                     static_cast<const float*>(eps), static_cast<float*>(act),
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_philox_normal(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, void* out, void* stream) {
  return guarded([&] {
    need(count >= 0, "philox_normal: negative count");
    if (count == 0) return;
    need(out, "philox_normal: out is null");
    HIP_OK(emb::launch_philox_normal(seed, offset, first, count, static_cast<float*>(out),
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_normal_policy_launches(int64_t* count) {
  return guarded([&] {
    need(count, "normal_policy_launches: count is null");
    *count = emb::normal_policy_launches();
  });
}

}  // extern "C"
