// emb_policy_loss*: the actor's loss of imag_loss (dreamerv3/agent.py:411-415)
// over Agg(Categorical(logits, unimix), dims, sum) (embodied/jax/outs.py:40-76,
// 208-234) -- the rows' logpi, entropy and policy loss in one kernel launch, the
// gradient in one more (policy_loss.hip).  Its own translation unit, as
// onehot_kl_abi.cpp: kernels_abi.cpp is also linked into the host sanitizer soak,
// against stand-in launchers that know nothing of these kernels.
#include "abi_common.h"
#include "policy_loss.h"

using namespace emb_abi;

namespace {

// What both entry points check before any HIP call; returns the number of output rows.
int64_t shape_ok(const char* who, int32_t dtype, int64_t N, int64_t T, int32_t drop, int64_t groups, int64_t classes,
                 float unimix, float actent) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(N >= 0 && T >= 0, say("negative N or T"));
  need(drop == 0 || drop == 1, say("drop must be 0 or 1"));
  need(groups >= 1, say("groups must be at least 1"));
  need(classes >= 1 && classes <= emb::kPolicyMaxClasses,
       say("classes outside 1 .. 256, the group one wave keeps in registers"));
  need(groups <= INT32_MAX / classes && (T == 0 || (T <= INT32_MAX / (groups * classes) &&
                                                     N <= INT32_MAX / (T * groups * classes))),
       say("more than 2^31 - 1 logits"));
  need(unimix >= 0.f && unimix < 1.f, say("unimix outside [0, 1)"));
  need(actent - actent == 0.f, say("actent must be finite"));                   // a NaN or an infinity fails
  return T > drop ? N * (T - drop) : 0;
}

}  // namespace

extern "C" {

int32_t emb_policy_loss(const void* logits, const void* act, int32_t dtype, int64_t N, int64_t T, int32_t drop,
                        int64_t groups, int64_t classes, float unimix, float actent, const void* adv,
                        const void* weight, int64_t weight_stride, void* loss, void* logpi, void* ent, void* stream) {
  return guarded([&] {
    if (!shape_ok("policy_loss", dtype, N, T, drop, groups, classes, unimix, actent)) return;
    need(logits && logpi && ent, "policy_loss: a pointer is null");
    need(!weight || weight_stride >= T - drop, "policy_loss: weight_stride below T - drop");
    HIP_OK(emb::launch_policy_loss(logits, static_cast<const int32_t*>(act), dtype == EMB_BF16, N, T, drop, groups,
                                   classes, unimix, actent, static_cast<const float*>(adv),
                                   static_cast<const float*>(weight), weight_stride, static_cast<float*>(loss),
                                   static_cast<float*>(logpi), static_cast<float*>(ent),
                                   static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_policy_loss_grad(const void* logits, const void* act, int32_t dtype, int64_t N, int64_t T, int32_t drop,
                             int64_t groups, int64_t classes, float unimix, float actent, const void* adv,
                             const void* weight, int64_t weight_stride, const void* gout, void* grad, void* stream) {
  return guarded([&] {
    const int64_t rows = shape_ok("policy_loss_grad", dtype, N, T, drop, groups, classes, unimix, actent);
    if (N * T == 0) return;                                  // no logits, no gradient
    need(logits && grad, "policy_loss_grad: a pointer is null");
    need(rows == 0 || gout, "policy_loss_grad: gout is null");
    need(!weight || weight_stride >= T - drop, "policy_loss_grad: weight_stride below T - drop");
    HIP_OK(emb::launch_policy_loss_grad(logits, static_cast<const int32_t*>(act), dtype == EMB_BF16, N, T, drop,
                                        groups, classes, unimix, actent, static_cast<const float*>(adv),
                                        static_cast<const float*>(weight), weight_stride,
                                        static_cast<const float*>(gout), grad, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_policy_loss_launches(int64_t* count) {
  return guarded([&] {
    need(count, "policy_loss_launches: count is null");
    *count = emb::policy_loss_launches();
  });
}

}  // extern "C"
