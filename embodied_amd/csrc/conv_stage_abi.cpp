// emb_pool_norm_act*, emb_norm_act_upsample*: the tails of DreamerV3's convolution
// stages (dreamerv3/rssm.py:238-241 and :327, 336-338, 346) in one kernel launch
// each, the gradients in one or two more (conv_stage.hip).  Its own translation
// unit, as norm_act_abi.cpp.
#include "abi_common.h"
#include "conv_stage.h"

using namespace emb_abi;

namespace {

// What every entry point checks before any HIP call.  Returns the Norm rows
// (pool: images * H/2 * W/2, upsample: images * H * W).
int64_t shape_ok(const char* who, bool pool, int32_t dtype, int64_t images, int64_t H, int64_t W, int64_t C,
                 int32_t impl, int32_t act, float eps) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(images >= 0, say("negative images"));
  need(H >= 1 && W >= 1, say("H and W must be at least 1"));
  need(!pool || H % 2 == 0, say("odd H: the 2x2 windows need an even height (rssm.py:239)"));
  need(!pool || W % 2 == 0, say("odd W: the 2x2 windows need an even width (rssm.py:239)"));
  need(C >= 1 && C <= emb::kConvStageMaxUnits, say("C outside 1 .. 1024, the pixel one wave keeps in registers"));
  int64_t room = INT32_MAX / (C * (pool ? 1 : 4));                 // the larger tensor: x of the pool, out of the upsample
  bool fits = images <= room;
  if (fits && images > 0) {
    room /= images;
    fits = H <= room && W <= room / H;
  }
  need(fits, say("more than 2^31 - 1 elements in the larger tensor"));
  need(impl == EMB_NORM_RMS || impl == EMB_NORM_LAYER, say("impl must be EMB_NORM_RMS or EMB_NORM_LAYER"));
  need(act == EMB_ACT_NONE || act == EMB_ACT_SILU || act == EMB_ACT_GELU || act == EMB_ACT_RELU,
       say("act must be EMB_ACT_NONE, EMB_ACT_SILU, EMB_ACT_GELU or EMB_ACT_RELU"));
  need(eps >= 0.f && eps - eps == 0.f, say("eps must be finite and not negative"));
  return pool ? images * (H / 2) * (W / 2) : images * H * W;
}

template <typename Launch>
void forward(const char* who, bool pool, Launch launch, const void* x, const void* scale, const void* shift,
             int32_t dtype, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps,
             void* out, void* stream) {
  const Who say{who};
  const int64_t pixels = shape_ok(who, pool, dtype, images, H, W, C, impl, act, eps);
  if (pixels == 0) return;
  need(x && out, say("a pointer is null"));
  HIP_OK(launch(x, static_cast<const float*>(scale), static_cast<const float*>(shift), dtype == EMB_BF16, images, H, W,
                C, impl, act, eps, out, static_cast<hipStream_t>(stream)));
}

template <typename Launch>
void backward(const char* who, bool pool, Launch launch, const void* x, const void* scale, const void* shift,
              const void* gout, int32_t dtype, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl,
              int32_t act, float eps, void* dx, void* dscale, void* dshift, void* partials, int64_t partial_floats,
              void* stream) {
  const Who say{who};
  const int64_t pixels = shape_ok(who, pool, dtype, images, H, W, C, impl, act, eps);
  need(dx || dscale || dshift, say("no output"));
  if (pixels == 0) return;                                   // no images: nothing is launched or written
  need(x && gout, say("a pointer is null"));
  if (dscale || dshift) {
    static thread_local std::string msg;
    const int64_t floats = 2 * emb::conv_stage_partials(pixels, C) * C;
    msg = std::string(who) + ": partials must hold " + std::to_string(floats) + " float32";
    need(partials && partial_floats >= floats, msg.c_str());
  }
  HIP_OK(launch(x, static_cast<const float*>(scale), static_cast<const float*>(shift), gout, dtype == EMB_BF16, images,
                H, W, C, impl, act, eps, dx, static_cast<float*>(dscale), static_cast<float*>(dshift),
                static_cast<float*>(partials), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int32_t emb_pool_norm_act(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t images, int64_t H,
                          int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out, void* stream) {
  return guarded([&] {
    forward("pool_norm_act", true, emb::launch_pool_norm_act, x, scale, shift, dtype, images, H, W, C, impl, act, eps,
            out, stream);
  });
}

int32_t emb_pool_norm_act_grad(const void* x, const void* scale, const void* shift, const void* gout, int32_t dtype,
                               int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps,
                               void* dx, void* dscale, void* dshift, void* partials, int64_t partial_floats,
                               void* stream) {
  return guarded([&] {
    backward("pool_norm_act_grad", true, emb::launch_pool_norm_act_grad, x, scale, shift, gout, dtype, images, H, W, C,
             impl, act, eps, dx, dscale, dshift, partials, partial_floats, stream);
  });
}

int32_t emb_norm_act_upsample(const void* x, const void* scale, const void* shift, int32_t dtype, int64_t images,
                              int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                              void* stream) {
  return guarded([&] {
    forward("norm_act_upsample", false, emb::launch_norm_act_upsample, x, scale, shift, dtype, images, H, W, C, impl,
            act, eps, out, stream);
  });
}

int32_t emb_norm_act_upsample_grad(const void* x, const void* scale, const void* shift, const void* gout,
                                   int32_t dtype, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl,
                                   int32_t act, float eps, void* dx, void* dscale, void* dshift, void* partials,
                                   int64_t partial_floats, void* stream) {
  return guarded([&] {
    backward("norm_act_upsample_grad", false, emb::launch_norm_act_upsample_grad, x, scale, shift, gout, dtype, images,
             H, W, C, impl, act, eps, dx, dscale, dshift, partials, partial_floats, stream);
  });
}

int32_t emb_conv_stage_launches(int64_t* count) {
  return guarded([&] {
    need(count, "conv_stage_launches: count is null");
    *count = emb::conv_stage_launches();
  });
}

}  // extern "C"
