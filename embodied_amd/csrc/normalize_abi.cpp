// emb_normalize: the running return normaliser, one kernel launch per call
// (normalize.hip).  Its own translation unit: it needs nothing of the replay's
// handles, rings or stream ordering.
#include "abi_common.h"
#include "normalize.h"

using namespace emb_abi;

extern "C" {

int32_t emb_normalize(const emb_normalize_config_t* config, const void* x, int64_t n, void* state,
                      int32_t update, const void* sub, void* out, void* stream) {
  return guarded([&] {
    need(config, "normalize: config is null");
    need(state, "normalize: state is null");
    need(n >= 0, "normalize: negative n");
    need(n <= INT32_MAX, "normalize: more than 2^31 - 1 values");
    need(x || n == 0, "normalize: x is null");
    need(config->impl == EMB_NORM_MEANSTD || config->impl == EMB_NORM_PERC,
         "normalize: unknown impl (EMB_NORM_MEANSTD or EMB_NORM_PERC)");
    need(config->rate >= 0.0 && config->rate <= 1.0, "normalize: rate outside [0, 1]");
    if (config->impl == EMB_NORM_PERC)
      need(config->perclo >= 0.0 && config->perclo <= 100.0 && config->perchi >= 0.0 &&
               config->perchi <= 100.0, "normalize: percentile outside [0, 100]");
    need(!(update && n == 0), "normalize: update needs at least one value");
    need(out || !sub, "normalize: sub without out");
    HIP_OK(emb::launch_normalize(
        static_cast<const float*>(x), n, static_cast<float*>(state), config->impl, update != 0,
        config->debias != 0, static_cast<float>(1.0 - config->rate), static_cast<float>(config->rate),
        static_cast<float>(config->limit), emb::norm_rank(config->perclo, n),
        emb::norm_rank(config->perchi, n), static_cast<const float*>(sub), static_cast<float*>(out),
        static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_normalize_launches(int64_t* count) {
  return guarded([&] {
    need(count, "normalize_launches: count is null");
    *count = emb::normalize_launches();
  });
}

}  // extern "C"
