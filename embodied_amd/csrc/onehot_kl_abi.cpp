// emb_onehot_kl*: the KL pair of RSSM.loss (dreamerv3/rssm.py:123-132) -- the
// rows' kl, max(kl, free_nats) and both entropies in one kernel launch, both
// gradients in one more (onehot_kl.hip).  Its own translation unit, as
// twohot_abi.cpp: kernels_abi.cpp is also linked into the host sanitizer soak,
// against stand-in launchers that know nothing of these kernels.
#include "abi_common.h"
#include "onehot_kl.h"

using namespace emb_abi;

namespace {

// What both entry points check before any HIP call; false: rows == 0, nothing to do.
bool shape_ok(const char* who, int32_t dtype, int64_t rows, int64_t stoch, int64_t classes, float unimix,
              float free_nats) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(rows >= 0, say("negative rows"));
  need(stoch >= 1, say("stoch must be at least 1"));
  need(classes >= 1 && classes <= emb::kOneHotMaxClasses,
       say("classes outside 1 .. 256, the group one wave keeps in registers"));
  need(stoch <= INT32_MAX / classes && rows <= INT32_MAX / (stoch * classes), say("more than 2^31 - 1 logits"));
  need(unimix >= 0.f && unimix < 1.f, say("unimix outside [0, 1)"));
  need(free_nats >= 0.f, say("free_nats must be >= 0 (0: no maximum)"));      // a NaN fails both
  return rows > 0;
}

}  // namespace

extern "C" {

int32_t emb_onehot_kl(const void* post, const void* prior, int32_t dtype, int64_t rows, int64_t stoch,
                      int64_t classes, float unimix, float free_nats, void* kl, void* ent_post, void* ent_prior,
                      void* dyn, void* rep, void* stream) {
  return guarded([&] {
    if (!shape_ok("onehot_kl", dtype, rows, stoch, classes, unimix, free_nats)) return;
    need(post && prior && kl && ent_post && ent_prior, "onehot_kl: a pointer is null");
    HIP_OK(emb::launch_onehot_kl(post, prior, dtype == EMB_BF16, rows, stoch, classes, unimix, free_nats,
                                 static_cast<float*>(kl), static_cast<float*>(ent_post),
                                 static_cast<float*>(ent_prior), static_cast<float*>(dyn), static_cast<float*>(rep),
                                 static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_onehot_kl_grad(const void* post, const void* prior, int32_t dtype, int64_t rows, int64_t stoch,
                           int64_t classes, float unimix, float free_nats, const void* kl, const void* g_rep,
                           const void* g_dyn, void* grad_post, void* grad_prior, void* stream) {
  return guarded([&] {
    if (!shape_ok("onehot_kl_grad", dtype, rows, stoch, classes, unimix, free_nats)) return;
    need(post && prior && kl, "onehot_kl_grad: a pointer is null");
    need(grad_post || grad_prior, "onehot_kl_grad: both gradients are null, nothing to write");
    need(!grad_post || g_rep, "onehot_kl_grad: grad_post without g_rep");
    need(!grad_prior || g_dyn, "onehot_kl_grad: grad_prior without g_dyn");
    HIP_OK(emb::launch_onehot_kl_grad(post, prior, dtype == EMB_BF16, rows, stoch, classes, unimix, free_nats,
                                      static_cast<const float*>(kl), static_cast<const float*>(g_rep),
                                      static_cast<const float*>(g_dyn), grad_post, grad_prior,
                                      static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_onehot_kl_launches(int64_t* count) {
  return guarded([&] {
    need(count, "onehot_kl_launches: count is null");
    *count = emb::onehot_kl_launches();
  });
}

}  // extern "C"
