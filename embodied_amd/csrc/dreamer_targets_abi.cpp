// emb_dreamer_targets: imag_loss's targets -- de-normalise, the lambda-return
// over float continuation probabilities, the weight, retnorm's percentile step,
// the advantage, advnorm's and valnorm's steps, the normalised advantage and
// target -- as one kernel launch (dreamer_targets.hip); and emb_scan_lambda_cont,
// that lambda-return as a scan of its own (scans.hip).  Its own translation
// unit, as ppo_targets_abi.cpp.  (emb_scan_lambda_cont lives here and not beside
// emb_scan_lambda: kernels_abi.cpp is also linked into the host sanitizer soak,
// against stand-in launchers that know nothing of this scan.)
#include "abi_common.h"
#include "dreamer_targets.h"
#include "kernels.h"

using namespace emb_abi;

namespace {

emb::DreamerNorm norm_of(const emb_normalize_config_t* config, void* state, int64_t values) {
  if (!config || config->impl == EMB_NORM_NONE) return emb::DreamerNorm{0, nullptr, 0.f, 0.f, 0.f, false, {}, {}};
  return emb::DreamerNorm{config->impl, static_cast<float*>(state), static_cast<float>(1.0 - config->rate),
                          static_cast<float>(config->rate), static_cast<float>(config->limit), config->debias != 0,
                          emb::norm_rank(config->perclo, values), emb::norm_rank(config->perchi, values)};
}

bool present(const emb_normalize_config_t* config) { return config && config->impl != EMB_NORM_NONE; }

}  // namespace

extern "C" {

int32_t emb_scan_lambda_cont(const void* rew, const void* con, const void* boot, int64_t B, int64_t T,
                             float disc, float lam, void* ret, void* stream) {
  return guarded([&] {
    need(rew && con && boot && ret, "scan_lambda_cont: a pointer is null");
    need(B >= 0, "scan_lambda_cont: negative B");
    need(B == 0 || T >= 2, "scan_lambda_cont: T < 2 (a row needs two steps)");
    need(B == 0 || (T <= INT32_MAX && B <= INT32_MAX / T), "scan_lambda_cont: more than 2^31 - 1 values");
    if (B == 0) return;
    HIP_OK(emb::launch_lambda_return_cont(static_cast<const float*>(rew), static_cast<const float*>(con),
                                          static_cast<const float*>(boot), B, T, disc, lam,
                                          static_cast<float*>(ret), static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_dreamer_targets(const emb_normalize_config_t* retnorm, const emb_normalize_config_t* valnorm,
                            const emb_normalize_config_t* advnorm, const void* rew, const void* con,
                            const void* pred, int64_t N, int64_t T, float disc, float lam, int32_t update,
                            void* ret, void* weight, void* adv, void* adv_normed, void* tar_padded,
                            void* ret_state, void* val_state, void* adv_state, void* stream) {
  return guarded([&] {
    need(retnorm, "dreamer_targets: the retnorm config is null");
    need(ret_state, "dreamer_targets: the retnorm state is null");
    need(retnorm->impl == EMB_NORM_PERC,
         "dreamer_targets: retnorm must be EMB_NORM_PERC (others: emb_scan_lambda_cont + emb_normalize)");
    need(!present(valnorm) || valnorm->impl == EMB_NORM_MEANSTD,
         "dreamer_targets: valnorm must be EMB_NORM_MEANSTD or none (others: emb_scan_lambda_cont + emb_normalize)");
    need(!present(advnorm) || advnorm->impl == EMB_NORM_MEANSTD,
         "dreamer_targets: advnorm must be EMB_NORM_MEANSTD or none (others: emb_scan_lambda_cont + emb_normalize)");
    need(!present(valnorm) || val_state, "dreamer_targets: the valnorm state is null");
    need(!present(advnorm) || adv_state, "dreamer_targets: the advnorm state is null");
    // a state that is not read (none) may be anything, the same address included
    void* const vstate = present(valnorm) ? val_state : nullptr;
    void* const astate = present(advnorm) ? adv_state : nullptr;
    need(ret_state != vstate && ret_state != astate && (!vstate || vstate != astate),
         "dreamer_targets: two normalisers share one state");
    need(N >= 0, "dreamer_targets: negative N");
    need(T >= 2, "dreamer_targets: T < 2 (a row needs two steps)");
    need(N == 0 || (rew && con && pred), "dreamer_targets: an input is null");
    need(N == 0 || (ret && weight && adv && adv_normed && tar_padded), "dreamer_targets: an output is null");
    need(T - 1 <= emb::kNormLdsMax && N <= emb::kNormLdsMax / (T - 1),
         "dreamer_targets: more than 16384 returns, the keys one workgroup holds (larger: emb_scan_lambda_cont + "
         "emb_normalize)");
    for (const emb_normalize_config_t* config : {retnorm, valnorm, advnorm})
      need(!present(config) || (config->rate >= 0.0 && config->rate <= 1.0), "dreamer_targets: rate outside [0, 1]");
    need(retnorm->perclo >= 0.0 && retnorm->perclo <= 100.0 && retnorm->perchi >= 0.0 && retnorm->perchi <= 100.0,
         "dreamer_targets: percentile outside [0, 100]");
    if (N == 0) return;
    const int64_t values = N * (T - 1);
    HIP_OK(emb::launch_dreamer_targets(
        static_cast<const float*>(rew), static_cast<const float*>(con), static_cast<const float*>(pred), N, T,
        disc, lam, update != 0, static_cast<float*>(ret), static_cast<float*>(weight), static_cast<float*>(adv),
        static_cast<float*>(adv_normed), static_cast<float*>(tar_padded), norm_of(retnorm, ret_state, values),
        norm_of(valnorm, vstate, values), norm_of(advnorm, astate, values), static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_dreamer_targets_launches(int64_t* count) {
  return guarded([&] {
    need(count, "dreamer_targets_launches: count is null");
    *count = emb::dreamer_targets_launches();
  });
}

}  // extern "C"
