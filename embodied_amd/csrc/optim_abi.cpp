// emb_optim_*: the reference's optimizer chain (embodied/jax/opt.py:109-164 under
// dreamerv3/agent.py:342-379) over every parameter tensor in two kernel launches,
// its metrics (opt.py:64-79) in a third one when asked (optim.hip); and the PPO
// learner's chain (ppo/agent.py:114-124) on the same tables, emb_optim_grad_norms
// and emb_optim_adam_update.  Its own
// translation unit, as policy_loss_abi.cpp: kernels_abi.cpp is also linked into
// the host sanitizer soak, against stand-in launchers that know nothing of these
// kernels.
#include "abi_common.h"
#include "optim.h"

using namespace emb_abi;

namespace {

bool finite(float x) { return x - x == 0.f; }                   // a NaN or an infinity fails

void tables_ok(const char* who, const void* table, const void* chunks, int64_t n_chunks, const void* partials) {
  const Who say{who};
  need(n_chunks >= 0 && n_chunks <= INT32_MAX, say("the number of chunks is outside 0 .. 2^31 - 1"));
  need(n_chunks == 0 || (table && chunks && partials), say("a pointer is null"));
}

}  // namespace

extern "C" {

int32_t emb_optim_table(const int64_t* addrs, const int64_t* counts, const int32_t* flags, int64_t tensors,
                        void* table, void* chunks, int64_t chunk_capacity, int64_t* n_chunks, int64_t* chunk_size,
                        int64_t* record_bytes) {
  return guarded([&] {
    if (chunk_size) *chunk_size = emb::kOptimChunk;
    if (record_bytes) *record_bytes = sizeof(emb::OptimTensor);
    const char* wrong = emb::optim_plan(addrs, counts, flags, tensors, static_cast<emb::OptimTensor*>(table),
                                        static_cast<emb::OptimChunk*>(chunks), chunk_capacity, n_chunks);
    need(!wrong, wrong);
  });
}

int32_t emb_optim_norms(const void* table, const void* chunks, int64_t n_chunks, void* partials, void* stream) {
  return guarded([&] {
    tables_ok("optim_norms", table, chunks, n_chunks, partials);
    if (n_chunks == 0) return;
    HIP_OK(emb::launch_optim_norms(static_cast<const emb::OptimTensor*>(table),
                                   static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                   static_cast<float*>(partials), static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_update(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr, float beta1,
                         float omb1, float c1, float beta2, float omb2, float c2, float eps, float agc, float pmin,
                         float wd, int32_t nesterov, void* stream) {
  return guarded([&] {
    tables_ok("optim_update", table, chunks, n_chunks, partials);
    need(finite(lr), "optim_update: lr must be finite");
    need(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "optim_update: a beta outside [0, 1)");
    need(omb1 > 0.f && omb1 <= 1.f && omb2 > 0.f && omb2 <= 1.f, "optim_update: 1 - beta outside (0, 1]");
    need(c1 > 0.f && c1 <= 1.f && c2 > 0.f && c2 <= 1.f, "optim_update: a bias correction outside (0, 1]");
    need(eps >= 0.f && finite(eps) && agc >= 0.f && finite(agc) && pmin >= 0.f && finite(pmin) && wd >= 0.f &&
             finite(wd),
         "optim_update: eps, agc, pmin and wd must be finite and not negative");
    need(nesterov == 0 || nesterov == 1, "optim_update: nesterov must be 0 or 1");
    if (n_chunks == 0) return;
    const emb::OptimStep step{lr, beta1, omb1, c1, beta2, omb2, c2, eps, agc, pmin, wd, nesterov};
    HIP_OK(emb::launch_optim_update(static_cast<const emb::OptimTensor*>(table),
                                    static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                    static_cast<float*>(partials), step, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_grad_norms(const void* table, const void* chunks, int64_t n_chunks, void* partials, void* stream) {
  return guarded([&] {
    need(n_chunks >= 1 && n_chunks <= INT32_MAX, "optim_grad_norms: the number of chunks is outside 1 .. 2^31 - 1");
    need(table && chunks && partials, "optim_grad_norms: a pointer is null");
    HIP_OK(emb::launch_optim_grad_norms(static_cast<const emb::OptimTensor*>(table),
                                        static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                        static_cast<float*>(partials), static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_adam_update(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                              float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps,
                              float clip, float wd, void* stream) {
  return guarded([&] {
    need(n_chunks >= 1 && n_chunks <= INT32_MAX, "optim_adam_update: the number of chunks is outside 1 .. 2^31 - 1");
    need(table && chunks && partials, "optim_adam_update: a pointer is null");
    need(finite(lr), "optim_adam_update: lr must be finite");
    need(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "optim_adam_update: a beta outside [0, 1)");
    need(omb1 > 0.f && omb1 <= 1.f && omb2 > 0.f && omb2 <= 1.f, "optim_adam_update: 1 - beta outside (0, 1]");
    need(c1 > 0.f && c1 <= 1.f && c2 > 0.f && c2 <= 1.f, "optim_adam_update: a bias correction outside (0, 1]");
    need(eps >= 0.f && finite(eps) && clip >= 0.f && finite(clip) && wd >= 0.f && finite(wd),
         "optim_adam_update: eps, clip and wd must be finite and not negative");
    const emb::AdamStep step{lr, beta1, omb1, c1, beta2, omb2, c2, eps, clip, wd};
    HIP_OK(emb::launch_optim_adam_update(static_cast<const emb::OptimTensor*>(table),
                                         static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                         static_cast<float*>(partials), step, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_metrics(const void* partials, int64_t n_chunks, int64_t count, void* out, void* stream) {
  return guarded([&] {
    need(n_chunks >= 0 && n_chunks <= INT32_MAX, "optim_metrics: the number of chunks is outside 0 .. 2^31 - 1");
    need(count >= 0, "optim_metrics: a negative parameter count");
    need(out && (n_chunks == 0 || partials), "optim_metrics: a pointer is null");
    HIP_OK(emb::launch_optim_metrics(static_cast<const float*>(partials), n_chunks, count, static_cast<float*>(out),
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_launches(int64_t* count) {
  return guarded([&] {
    need(count, "optim_launches: count is null");
    *count = emb::optim_launches();
  });
}

}  // extern "C"
