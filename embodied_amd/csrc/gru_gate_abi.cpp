// emb_gru_gate*: the gate at the end of RSSM._core (dreamerv3/rssm.py:152-159) in
// one kernel launch, its gradient in one more (gru_gate.hip).  Its own
// translation unit, as policy_loss_abi.cpp: kernels_abi.cpp is also linked into
// the host sanitizer soak, against stand-in launchers that know nothing of these
// kernels.
#include "abi_common.h"
#include "gru_gate.h"

using namespace emb_abi;

namespace {

// What both entry points check before any HIP call.
void shape_ok(const char* who, int32_t dtype, int64_t rows, int64_t deter, int64_t blocks) {
  const Who say{who};
  need(dtype == EMB_F32 || dtype == EMB_BF16, say("dtype must be EMB_F32 or EMB_BF16"));
  need(rows >= 0, say("negative rows"));
  need(deter >= 1, say("deter must be at least 1"));
  need(blocks >= 1 && deter % blocks == 0, say("blocks must divide deter"));
  need(deter <= INT32_MAX / 3 && rows <= INT32_MAX / (3 * deter), say("more than 2^31 - 1 elements of x"));
}

}  // namespace

extern "C" {

int32_t emb_gru_gate(const void* x, const void* deter, int32_t dtype, int64_t rows, int64_t width, int64_t blocks,
                     void* out, void* stream) {
  return guarded([&] {
    shape_ok("gru_gate", dtype, rows, width, blocks);
    if (rows == 0) return;
    need(x && deter && out, "gru_gate: a pointer is null");
    HIP_OK(emb::launch_gru_gate(x, deter, dtype == EMB_BF16, rows, width, blocks, out,
                                static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_gru_gate_grad(const void* x, const void* deter, const void* gout, int32_t dtype, int64_t rows,
                          int64_t width, int64_t blocks, void* dx, void* ddeter, void* stream) {
  return guarded([&] {
    shape_ok("gru_gate_grad", dtype, rows, width, blocks);
    need(dx || ddeter, "gru_gate_grad: no output");
    if (rows == 0) return;
    need(x && deter && gout, "gru_gate_grad: a pointer is null");
    HIP_OK(emb::launch_gru_gate_grad(x, deter, gout, dtype == EMB_BF16, rows, width, blocks, dx, ddeter,
                                     static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_gru_gate_launches(int64_t* count) {
  return guarded([&] {
    need(count, "gru_gate_launches: count is null");
    *count = emb::gru_gate_launches();
  });
}

}  // extern "C"
