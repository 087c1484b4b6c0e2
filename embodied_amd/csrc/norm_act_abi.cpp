// emb_norm_act*: Norm followed by the activation (embodied/jax/nets.py:361-399,
// nets.py:26-39) in one kernel launch, the gradient in one or two more
// (norm_act.hip).  Its own translation unit, as policy_loss_abi.cpp:
// kernels_abi.cpp is also linked into the host sanitizer soak, against stand-in
// launchers that know nothing of these kernels.
#include "abi_common.h"
#include "norm_act.h"

using namespace emb_abi;

namespace {

// What both entry points check before any HIP call.
void shape_ok(const char* who, int32_t dtype, int64_t rows, int64_t units, int32_t impl, int32_t act, float eps) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(rows >= 0, say("negative rows"));
  need(units >= 1 && units <= emb::kNormActMaxUnits,
       say("units outside 1 .. 16384, the row one workgroup keeps in registers"));
  need(rows <= INT32_MAX / units, say("more than 2^31 - 1 elements"));
  need(impl == EMB_NORM_RMS || impl == EMB_NORM_LAYER, say("impl must be EMB_NORM_RMS or EMB_NORM_LAYER"));
  need(act == EMB_ACT_NONE || act == EMB_ACT_SILU || act == EMB_ACT_GELU || act == EMB_ACT_RELU,
       say("act must be EMB_ACT_NONE, EMB_ACT_SILU, EMB_ACT_GELU or EMB_ACT_RELU"));
  need(eps >= 0.f && eps - eps == 0.f, say("eps must be finite and not negative"));
}

}  // namespace

static_assert(EMB_NORM_RMS == emb::kNormRms && EMB_NORM_LAYER == emb::kNormLayer, "the header's codes");
static_assert(EMB_ACT_NONE == emb::kActNone && EMB_ACT_SILU == emb::kActSilu && EMB_ACT_GELU == emb::kActGelu &&
                  EMB_ACT_RELU == emb::kActRelu, "the header's codes");

extern "C" {

int32_t emb_norm_act(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t rows, int64_t units,
                     int32_t impl, int32_t act, float eps, void* out, void* stream) {
  return guarded([&] {
    shape_ok("norm_act", dtype, rows, units, impl, act, eps);
    if (rows == 0) return;
    need(x && out, "norm_act: a pointer is null");
    HIP_OK(emb::launch_norm_act(x, static_cast<const float*>(scale), static_cast<const float*>(shift),
                                dtype == EMB_BF16, rows, units, impl, act, eps, out,
                                static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_norm_act_grad(const void* x, const void* scale, const void* shift, const void* gout, int32_t dtype,
                          int64_t rows, int64_t units, int32_t impl, int32_t act, float eps, void* dx, void* dscale,
                          void* dshift, void* partials, int64_t partial_floats, void* stream) {
  return guarded([&] {
    shape_ok("norm_act_grad", dtype, rows, units, impl, act, eps);
    need(dx || dscale || dshift, "norm_act_grad: no output");
    if (rows == 0) return;                                   // no rows: nothing is launched or written
    need(x && gout, "norm_act_grad: a pointer is null");
    if (dscale || dshift) {
      static thread_local std::string msg;
      const int64_t floats = 2 * emb::norm_act_partials(rows, units) * units;
      msg = "norm_act_grad: partials must hold " + std::to_string(floats) + " float32";
      need(partials && partial_floats >= floats, msg.c_str());
    }
    HIP_OK(emb::launch_norm_act_grad(x, static_cast<const float*>(scale), static_cast<const float*>(shift), gout,
                                     dtype == EMB_BF16, rows, units, impl, act, eps, dx, static_cast<float*>(dscale),
                                     static_cast<float*>(dshift), static_cast<float*>(partials),
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_norm_act_launches(int64_t* count) {
  return guarded([&] {
    need(count, "norm_act_launches: count is null");
    *count = emb::norm_act_launches();
  });
}

}  // extern "C"
