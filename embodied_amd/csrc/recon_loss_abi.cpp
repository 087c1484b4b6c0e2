// emb_recon_loss*: the reconstruction terms of the world-model loss
// (dreamerv3/agent.py:170-182) -- the image MSE from uint8 frames behind the
// decoder's sigmoid (dreamerv3/rssm.py:349, 353-356), the symlog MSE
// (embodied/jax/heads.py:127-130, embodied/jax/outs.py:129-141) and the Binary
// continue head (outs.py:189-201) -- one kernel launch forward, one backward
// (recon_loss.hip).  Its own translation unit, as onehot_sample_abi.cpp:
// kernels_abi.cpp is also linked into the host sanitizer soak, against stand-in
// launchers that know nothing of these kernels.
#include "abi_common.h"
#include "recon_loss.h"

using namespace emb_abi;

namespace {

int element_type(int32_t dtype) {
  return dtype == EMB_F32 ? emb::kReconF32 : dtype == EMB_BF16 ? emb::kReconBf16 : emb::kReconU8;
}

size_t element_size(int32_t dtype) { return dtype == EMB_F32 ? 4 : dtype == EMB_BF16 ? 2 : 1; }

// What both entry points check before any HIP call; returns the number of rows.
int64_t shape_ok(const char* who, int32_t x_dtype, int32_t target_dtype, float div, int64_t rows, int64_t units,
                 int32_t op) {
  const Who say{who};
  need(x_dtype == EMB_F32 || x_dtype == EMB_BF16, say("x_dtype must be EMB_F32 or EMB_BF16"));
  need(target_dtype == EMB_F32 || target_dtype == EMB_BF16 || target_dtype == EMB_U8,
       say("target_dtype must be EMB_F32, EMB_BF16 or EMB_U8"));
  need(op == EMB_RECON_MSE || op == EMB_RECON_MSE_SYMLOG || op == EMB_RECON_SIGMOID_MSE || op == EMB_RECON_BINARY,
       say("op must be one of EMB_RECON_MSE, _MSE_SYMLOG, _SIGMOID_MSE, _BINARY"));
  need(div > 0.f && div < INFINITY, say("div must be positive and finite"));
  need(rows >= 0, say("negative rows"));
  need(units >= 1, say("units must be at least 1"));
  need(rows <= INT32_MAX / units, say("more than 2^31 - 1 elements"));
  return rows;
}

void aligned(const char* who, const void* pointer, int32_t dtype, const char* what) {
  static thread_local std::string msg;
  need(reinterpret_cast<uintptr_t>(pointer) % element_size(dtype) == 0,
       (msg = std::string(who) + ": " + what + " is not aligned to its element size").c_str());
}

}  // namespace

extern "C" {

int32_t emb_recon_loss(const void* x, int32_t x_dtype, const void* target, int32_t target_dtype, float div,
                       int64_t rows, int64_t units, int32_t op, void* loss, void* stream) {
  return guarded([&] {
    if (!shape_ok("recon_loss", x_dtype, target_dtype, div, rows, units, op)) return;
    need(x && target && loss, "recon_loss: a pointer is null");
    aligned("recon_loss", x, x_dtype, "x");
    aligned("recon_loss", target, target_dtype, "target");
    aligned("recon_loss", loss, EMB_F32, "loss");
    HIP_OK(emb::launch_recon_loss(x, element_type(x_dtype), target, element_type(target_dtype), div, rows, units, op,
                                  static_cast<float*>(loss), static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_recon_loss_grad(const void* x, int32_t x_dtype, const void* target, int32_t target_dtype, float div,
                            int64_t rows, int64_t units, int32_t op, const void* gout, void* grad, void* stream) {
  return guarded([&] {
    if (!shape_ok("recon_loss_grad", x_dtype, target_dtype, div, rows, units, op)) return;
    need(x && target && gout && grad, "recon_loss_grad: a pointer is null");
    aligned("recon_loss_grad", x, x_dtype, "x");
    aligned("recon_loss_grad", target, target_dtype, "target");
    aligned("recon_loss_grad", gout, EMB_F32, "gout");
    aligned("recon_loss_grad", grad, x_dtype, "grad");
    HIP_OK(emb::launch_recon_loss_grad(x, element_type(x_dtype), target, element_type(target_dtype), div, rows, units,
                                       op, static_cast<const float*>(gout), grad, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_recon_loss_launches(int64_t* count) {
  return guarded([&] {
    need(count, "recon_loss_launches: count is null");
    *count = emb::recon_loss_launches();
  });
}

}  // extern "C"
