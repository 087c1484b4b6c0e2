// emb_block_linear_plan: the launch plan of BlockLinear (embodied/jax/nets.py:254-281)
// from block_linear.h.  Host code only, no HIP call.  Its own translation unit, as
// gru_gate_abi.cpp: kernels_abi.cpp is also linked into the host sanitizer soak.
#include "abi_common.h"
#include "block_linear.h"

using namespace emb_abi;

namespace {

// block_linear.h states the index rule: more than 2^31 - 1 elements of any buffer are refused.
void shape_ok(const char* who, int64_t rows, int64_t g, int64_t I, int64_t O, int32_t outputs) {
  static thread_local std::string msg;
  const char* why = emb::block_linear_shape_error(rows, g, I, O, outputs);
  if (why) need(false, (msg = std::string(who) + ": " + why).c_str());
}

}  // namespace

extern "C" {

int32_t emb_block_linear_plan(int64_t rows, int64_t g, int64_t I, int64_t O, int32_t outputs,
                              emb_block_linear_plan_t* plan) {
  return guarded([&] {
    need(plan, "block_linear_plan: plan is null");
    need(outputs >= 0 && outputs < 16, "block_linear_plan: outputs is a mask of EMB_BLOCK_LINEAR_*");
    shape_ok("block_linear_plan", rows, g, I, O, outputs);
    *plan = rows == 0 ? emb_block_linear_plan_t{} : emb::block_linear_plan(rows, g, I, O, outputs);
  });
}

}  // extern "C"
