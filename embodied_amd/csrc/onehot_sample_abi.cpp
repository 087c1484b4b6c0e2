// emb_philox_uniform, emb_onehot_sample*: the draw of OneHot / Categorical
// (embodied/jax/outs.py:208-224, 243-254, 265-270) behind dreamerv3/rssm.py:87, 100
// and dreamerv3/agent.py:18, 126, 192 -- the Philox uniform, the index and the
// straight-through one-hot in one kernel launch, the gradient in one more
// (onehot_sample.hip).  Its own translation unit, as policy_loss_abi.cpp:
// kernels_abi.cpp is also linked into the host sanitizer soak, against stand-in
// launchers that know nothing of these kernels.
#include "abi_common.h"
#include "onehot_sample.h"

using namespace emb_abi;

namespace {

// What both entry points check before any HIP call; returns the number of groups.
int64_t shape_ok(const char* who, int32_t dtype, int64_t rows, int64_t groups, int64_t classes, float unimix) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(rows >= 0, say("negative rows"));
  need(groups >= 1, say("groups must be at least 1"));
  need(classes >= 1 && classes <= emb::kSampleMaxClasses,
       say("classes outside 1 .. 256, the group one wave keeps in registers"));
  need(groups <= INT32_MAX / classes && rows <= INT32_MAX / (groups * classes), say("more than 2^31 - 1 logits"));
  need(unimix >= 0.f && unimix < 1.f, say("unimix outside [0, 1)"));
  return rows * groups;
}

}  // namespace

extern "C" {

int32_t emb_philox_uniform(uint64_t seed, uint64_t offset, uint64_t first, int64_t count, void* out, void* stream) {
  return guarded([&] {
    need(count >= 0, "philox_uniform: negative count");
    if (count == 0) return;
    need(out, "philox_uniform: out is null");
    HIP_OK(emb::launch_philox_uniform(seed, offset, first, count, static_cast<float*>(out),
                                      static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_onehot_sample(const void* logits, int32_t dtype, int64_t rows, int64_t groups, int64_t classes,
                          float unimix, int32_t mode, uint64_t seed, uint64_t offset, const void* uniform,
                          void* index, void* onehot, void* stream) {
  return guarded([&] {
    need(mode == EMB_SAMPLE_DRAW || mode == EMB_SAMPLE_PRED, "onehot_sample: mode must be EMB_SAMPLE_DRAW or EMB_SAMPLE_PRED");
    if (!shape_ok("onehot_sample", dtype, rows, groups, classes, unimix)) return;
    need(logits, "onehot_sample: logits is null");
    need(index || onehot, "onehot_sample: index and onehot are both null");
    HIP_OK(emb::launch_onehot_sample(logits, dtype == EMB_BF16, rows, groups, classes, unimix,
                                     mode == EMB_SAMPLE_PRED ? emb::kSamplePred : emb::kSampleDraw, seed, offset,
                                     static_cast<const float*>(uniform), static_cast<int32_t*>(index), onehot,
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_onehot_sample_grad(const void* logits, const void* gout, int32_t dtype, int64_t rows, int64_t groups,
                               int64_t classes, float unimix, void* grad, void* stream) {
  return guarded([&] {
    if (!shape_ok("onehot_sample_grad", dtype, rows, groups, classes, unimix)) return;
    need(logits && gout && grad, "onehot_sample_grad: a pointer is null");
    HIP_OK(emb::launch_onehot_sample_grad(logits, gout, dtype == EMB_BF16, rows, groups, classes, unimix, grad,
                                          static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_onehot_sample_launches(int64_t* count) {
  return guarded([&] {
    need(count, "onehot_sample_launches: count is null");
    *count = emb::onehot_sample_launches();
  });
}

}  // extern "C"
