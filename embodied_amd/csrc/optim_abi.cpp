// emb_optim_*: the reference's optimizer chain (embodied/jax/opt.py:109-164 under
// dreamerv3/agent.py:342-379) over every parameter tensor in two kernel launches,
// its metrics (opt.py:64-79) in a third one when asked (optim.hip); and the PPO
// learner's chain (ppo/agent.py:114-124) on the same tables, emb_optim_grad_norms
// and emb_optim_adam_update; the slow (EMA) copy of embodied/jax/utils.py:94-127 in a
// launch of its own (emb_slow_table, emb_slow_update) or inside either update
// launch (emb_optim_update_slow, emb_optim_adam_update_slow).  Its own
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

// The refusals emb_optim_update and emb_optim_update_slow share, and the step they launch with.
emb::OptimStep update_step(const char* who, const void* table, const void* chunks, int64_t n_chunks,
                           const void* partials, float lr, float beta1, float omb1, float c1, float beta2, float omb2,
                           float c2, float eps, float agc, float pmin, float wd, int32_t nesterov) {
  const Who say{who};
  tables_ok(who, table, chunks, n_chunks, partials);
  need(finite(lr), say("lr must be finite"));
  need(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, say("a beta outside [0, 1)"));
  need(omb1 > 0.f && omb1 <= 1.f && omb2 > 0.f && omb2 <= 1.f, say("1 - beta outside (0, 1]"));
  need(c1 > 0.f && c1 <= 1.f && c2 > 0.f && c2 <= 1.f, say("a bias correction outside (0, 1]"));
  need(eps >= 0.f && finite(eps) && agc >= 0.f && finite(agc) && pmin >= 0.f && finite(pmin) && wd >= 0.f &&
           finite(wd),
       say("eps, agc, pmin and wd must be finite and not negative"));
  need(nesterov == 0 || nesterov == 1, say("nesterov must be 0 or 1"));
  return emb::OptimStep{lr, beta1, omb1, c1, beta2, omb2, c2, eps, agc, pmin, wd, nesterov};
}

// The same for emb_optim_adam_update and emb_optim_adam_update_slow.
emb::AdamStep adam_step(const char* who, const void* table, const void* chunks, int64_t n_chunks, const void* partials,
                        float lr, float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps,
                        float clip, float wd) {
  const Who say{who};
  need(n_chunks >= 1 && n_chunks <= INT32_MAX, say("the number of chunks is outside 1 .. 2^31 - 1"));
  need(table && chunks && partials, say("a pointer is null"));
  need(finite(lr), say("lr must be finite"));
  need(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, say("a beta outside [0, 1)"));
  need(omb1 > 0.f && omb1 <= 1.f && omb2 > 0.f && omb2 <= 1.f, say("1 - beta outside (0, 1]"));
  need(c1 > 0.f && c1 <= 1.f && c2 > 0.f && c2 <= 1.f, say("a bias correction outside (0, 1]"));
  need(eps >= 0.f && finite(eps) && clip >= 0.f && finite(clip) && wd >= 0.f && finite(wd),
       say("eps, clip and wd must be finite and not negative"));
  return emb::AdamStep{lr, beta1, omb1, c1, beta2, omb2, c2, eps, clip, wd};
}

// What the three entry points that write a slow copy refuse alike: the reference
// mixes with a rate of 1 or below 0.5 and its float32 complement (utils.py:97, 118).
void mix_ok(const char* who, float mix, float omm) {
  const Who say{who};
  need(mix >= 0.f && mix <= 1.f, say("mix is outside [0, 1]"));
  need(finite(omm) && omm >= 0.f && omm <= 1.f, say("omm must be finite and in [0, 1]"));
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
    const emb::OptimStep step = update_step("optim_update", table, chunks, n_chunks, partials, lr, beta1, omb1, c1,
                                            beta2, omb2, c2, eps, agc, pmin, wd, nesterov);
    if (n_chunks == 0) return;
    HIP_OK(emb::launch_optim_update(static_cast<const emb::OptimTensor*>(table),
                                    static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                    static_cast<float*>(partials), step, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_update_slow(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                              float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps, float agc,
                              float pmin, float wd, int32_t nesterov, const void* slow, float mix, float omm,
                              void* stream) {
  return guarded([&] {
    const emb::OptimStep step = update_step("optim_update_slow", table, chunks, n_chunks, partials, lr, beta1, omb1,
                                            c1, beta2, omb2, c2, eps, agc, pmin, wd, nesterov);
    need(slow, "optim_update_slow: slow is null");
    mix_ok("optim_update_slow", mix, omm);
    if (n_chunks == 0) return;
    HIP_OK(emb::launch_optim_update_slow(static_cast<const emb::OptimTensor*>(table),
                                         static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                         static_cast<float*>(partials), step, static_cast<const uint64_t*>(slow), mix,
                                         omm, static_cast<hipStream_t>(stream)));
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
    const emb::AdamStep step = adam_step("optim_adam_update", table, chunks, n_chunks, partials, lr, beta1, omb1, c1,
                                         beta2, omb2, c2, eps, clip, wd);
    HIP_OK(emb::launch_optim_adam_update(static_cast<const emb::OptimTensor*>(table),
                                         static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                         static_cast<float*>(partials), step, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_optim_adam_update_slow(const void* table, const void* chunks, int64_t n_chunks, void* partials, float lr,
                                   float beta1, float omb1, float c1, float beta2, float omb2, float c2, float eps,
                                   float clip, float wd, const void* slow, float mix, float omm, void* stream) {
  return guarded([&] {
    const emb::AdamStep step = adam_step("optim_adam_update_slow", table, chunks, n_chunks, partials, lr, beta1, omb1,
                                         c1, beta2, omb2, c2, eps, clip, wd);
    need(slow, "optim_adam_update_slow: slow is null");
    mix_ok("optim_adam_update_slow", mix, omm);
    HIP_OK(emb::launch_optim_adam_update_slow(static_cast<const emb::OptimTensor*>(table),
                                              static_cast<const emb::OptimChunk*>(chunks), n_chunks,
                                              static_cast<float*>(partials), step, static_cast<const uint64_t*>(slow),
                                              mix, omm, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_slow_table(const int64_t* addrs, const int64_t* counts, int64_t tensors, void* table, void* chunks,
                       int64_t chunk_capacity, int64_t* n_chunks, int64_t* record_bytes) {
  return guarded([&] {
    if (record_bytes) *record_bytes = sizeof(emb::SlowTensor);
    const char* wrong = emb::slow_plan(addrs, counts, tensors, static_cast<emb::SlowTensor*>(table),
                                       static_cast<emb::OptimChunk*>(chunks), chunk_capacity, n_chunks);
    need(!wrong, wrong);
  });
}

int32_t emb_slow_update(const void* table, const void* chunks, int64_t n_chunks, float mix, float omm, void* stream) {
  return guarded([&] {
    const Who say{"slow_update"};
    need(n_chunks >= 0 && n_chunks <= INT32_MAX, say("the number of chunks is outside 0 .. 2^31 - 1"));
    need(n_chunks == 0 || (table && chunks), say("a pointer is null"));
    mix_ok("slow_update", mix, omm);
    if (n_chunks == 0) return;
    HIP_OK(emb::launch_slow_update(static_cast<const emb::SlowTensor*>(table),
                                   static_cast<const emb::OptimChunk*>(chunks), n_chunks, mix, omm,
                                   static_cast<hipStream_t>(stream)));
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
