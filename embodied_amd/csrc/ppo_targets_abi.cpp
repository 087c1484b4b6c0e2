// emb_ppo_targets: the top of the PPO loss -- de-normalise, GAE, both return
// normalisers, the normalised target and advantage -- as one kernel launch
// (ppo_targets.hip).  Its own translation unit, as normalize_abi.cpp.
#include "abi_common.h"
#include "ppo_targets.h"

using namespace emb_abi;

namespace {

emb::PpoNorm norm_of(const emb_normalize_config_t* config, void* state) {
  return emb::PpoNorm{static_cast<float*>(state), static_cast<float>(1.0 - config->rate),
                      static_cast<float>(config->rate), static_cast<float>(config->limit), config->debias != 0};
}

}  // namespace

extern "C" {

int32_t emb_ppo_targets(const emb_normalize_config_t* valnorm, const emb_normalize_config_t* advnorm,
                        const void* rew, const void* pred, const void* last, const void* term, int64_t B,
                        int64_t T, float live_scale, float lam, float tarclip, int32_t update, void* adv,
                        void* tar, void* tar_normed, void* adv_normed, void* valnorm_state,
                        void* advnorm_state, void* stream) {
  return guarded([&] {
    need(valnorm && advnorm, "ppo_targets: a config is null");
    need(valnorm_state && advnorm_state, "ppo_targets: a state is null");
    need(valnorm_state != advnorm_state, "ppo_targets: the two normalisers share one state");
    need(B >= 0, "ppo_targets: negative B");
    need(B == 0 || T >= 2, "ppo_targets: T < 2 (a row needs two steps)");
    need(B == 0 || (T <= INT32_MAX && B <= INT32_MAX / T), "ppo_targets: more than 2^31 - 1 values");
    need(B == 0 || (rew && pred && last && term), "ppo_targets: an input is null");
    need(B == 0 || (adv && tar && tar_normed && adv_normed), "ppo_targets: an output is null");
    need(valnorm->impl == EMB_NORM_MEANSTD && advnorm->impl == EMB_NORM_MEANSTD,
         "ppo_targets: both normalisers must be EMB_NORM_MEANSTD (others: emb_scan_gae + emb_normalize)");
    for (const emb_normalize_config_t* config : {valnorm, advnorm})
      need(config->rate >= 0.0 && config->rate <= 1.0, "ppo_targets: rate outside [0, 1]");
    need(tarclip >= 0.f, "ppo_targets: negative tarclip (0 = no clip)");
    if (B == 0) return;
    HIP_OK(emb::launch_ppo_targets(
        static_cast<const float*>(rew), static_cast<const float*>(pred), static_cast<const uint8_t*>(last),
        static_cast<const uint8_t*>(term), B, T, live_scale, lam, tarclip, update != 0,
        static_cast<float*>(adv), static_cast<float*>(tar), static_cast<float*>(tar_normed),
        static_cast<float*>(adv_normed), norm_of(valnorm, valnorm_state), norm_of(advnorm, advnorm_state),
        static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_ppo_targets_launches(int64_t* count) {
  return guarded([&] {
    need(count, "ppo_targets_launches: count is null");
    *count = emb::ppo_targets_launches();
  });
}

}  // extern "C"
