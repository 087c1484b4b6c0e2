// Host side of the device env's step launches (synth_env.hip): the blocks they
// read from device memory, and for the fused step (step + obs stack + early
// insert) the checks that decide whether it can be launched and the layout of
// its device block.  Plain C++ -- no HIP -- so that tests/fused_host/check.cpp
// runs it against tests/fake_hip without a GPU.
#pragma once

#include "kernels.h"

#include <cstdint>
#include <cstring>

namespace emb {
namespace synth_host {

// Mask job: the env's launch stores `act * !reset[e]` (the policy's raw actions
// times the flags the step itself restarts on: the Driver passes the previous
// step's is_last as `reset`) to `out`, the Driver's masked-action buffer -- the
// env's input as driver.py:72-75 defines it -- so that no launch of its own has
// to make that copy.  src == null: no job.
//
// Where the job travels.  The preload covers 14 dwords (16 user SGPRs less the
// two of the kernel-argument pointer; `.amdhsa_user_sgpr_kernarg_preload_length
// 14` for synth_env_kernel) and the step's own arguments fill them: two more
// pointers and the key's size would be fetched with s_load by EVERY wave, frame
// workgroups included (the compiler puts the kernel-argument loads in front of
// the first branch) -- with host-resident arguments a PCIe read in front of
// every frame store.  So the masked form takes ONE pointer to a block in device
// memory (written through the BAR like step.hip's PreTable) in place of the
// three flag offsets, which move into the block: 56 bytes, all preloaded, and only
// workgroup 0 of an env -- the one that stores the masked values and the flags --
// reads the block.  The frame workgroups run the same instructions as before.
struct alignas(16) SynthMaskJob {
  const uint8_t* src;         // (n, rowbytes) raw actions
  uint8_t* out;               // (n, rowbytes) masked actions
  int32_t rowbytes, dtype, elem;
  int32_t off_first, off_last, off_terminal;   // bytes from `reward` (masked form only)
};
static_assert(sizeof(SynthMaskJob) == kSynthJobBytes, "kernels.h states the size of the block");

// Head of the fused step's device block (written through the BAR with the early
// insert's table behind it): what the 14 preloaded dwords of
// synth_env_fused_kernel have no room for.  Only an env's narrow workgroup reads
// the job and the pointers; a frame workgroup reads env0, scale and offset (one
// scalar load, beside the loads of the env's state and its row).
struct alignas(16) SynthFusedHead {
  SynthMaskJob job;             // (with the flag offsets from `reward`)
  float* reward;
  int32_t* counters;            // both generations
  int32_t env0, len_turn;       // episode length | turn << 31, as synth_env_masked_kernel's
  float scale, offset;
  int32_t n_narrow, pad[3];
};
static_assert(sizeof(SynthFusedHead) == kSynthFusedHeadBytes, "kernels.h states the size of the head");
static_assert(kSynthFusedHeadBytes % 16 == 0, "the early insert's table (16-byte aligned) follows the head");

// What every form of the step asks of its sizes and addresses.
inline bool shape_ok(const uint8_t* image, int64_t n, int64_t frame_bytes, int64_t env0, int64_t episode_len) {
  return !(frame_bytes % 16 != 0 || reinterpret_cast<uint64_t>(image) % 16 != 0 || n > (1 << 29) ||
           frame_bytes > INT32_MAX || env0 > INT32_MAX || episode_len > INT32_MAX);
}

// The flag buffers as 32-bit offsets from `reward`; false when one does not fit.
inline bool offsets(const float* reward, const uint8_t* is_first, const uint8_t* is_last,
                    const uint8_t* is_terminal, int32_t* of, int32_t* ol, int32_t* ot) {
  const int64_t base = reinterpret_cast<int64_t>(reward);
  const int64_t f = reinterpret_cast<int64_t>(is_first) - base, l = reinterpret_cast<int64_t>(is_last) - base,
                t = reinterpret_cast<int64_t>(is_terminal) - base;
  auto fits = [](int64_t x) { return x >= INT32_MIN && x <= INT32_MAX; };
  if (!fits(f) || !fits(l) || !fits(t)) return false;
  *of = static_cast<int32_t>(f);
  *ol = static_cast<int32_t>(l);
  *ot = static_cast<int32_t>(t);
  return true;
}

// Why the fused launch cannot take this step (null = it can).
inline const char* fused_refusal(const SynthStepArgs& env, const PrewritePlan& plan) {
  if (!prewrite_supported(plan)) return "the early insert does not take this plan (prewrite_supported)";
  if (plan.channels != 4 || plan.frames != env.image || plan.n != env.n ||
      plan.pixels * plan.channels != env.frame_bytes)
    return "the plan's frames are not the env's 4-channel image buffer";
  if (!(plan.out_dtype == kU8 || plan.out_dtype == kF16 || plan.out_dtype == kBF16 || plan.out_dtype == kF32) ||
      !(plan.layout == kLayoutSame || plan.layout == kLayoutChannelsFirst))
    return "the policy batch's dtype or layout is not one the launch writes";
  if (!env.act || !env.masked_out || !env.reset || !carry_supported(env.row_bytes, env.dtype))
    return "the mask job needs 1..256 action elements of a known dtype and the reset flags";
  if (!env.image || !env.reward || !env.is_first || !env.is_last || !env.is_terminal || !env.counters ||
      env.n <= 0 || env.episode_len < 1 || !shape_ok(env.image, env.n, env.frame_bytes, env.env0, env.episode_len))
    return "bad env arguments";
  for (int k = 0; k < plan.n_narrow; ++k) {
    const uint8_t* src = plan.narrow[k].src;
    const bool reward = src == reinterpret_cast<const uint8_t*>(env.reward) && plan.narrow[k].rowbytes == 4;
    const bool flag = (src == env.is_first || src == env.is_last || src == env.is_terminal) &&
                      plan.narrow[k].rowbytes == 1;
    if (!reward && !flag) return "a narrow key's source is not one of the env's four output buffers";
  }
  int32_t f, l, t;
  if (!offsets(env.reward, env.is_first, env.is_last, env.is_terminal, &f, &l, &t))
    return "the flag buffers are too far from the reward buffer for 32-bit offsets";
  return nullptr;
}

inline size_t fused_block_bytes(int64_t n) { return kSynthFusedHeadBytes + prewrite_table_bytes(n); }

// `elem`: bytes of one action element (dtype_size(env.dtype)).
inline void fused_fill(void* dst, const SynthStepArgs& env, int elem, const PrewritePlan& plan,
                       const int32_t* rows, const uint8_t* stepids) {
  // (dst may be write-combined device memory behind the BAR: written once, front to back.)
  SynthFusedHead head;
  std::memset(&head, 0, sizeof(head));
  head.job = SynthMaskJob{static_cast<const uint8_t*>(env.act), static_cast<uint8_t*>(env.masked_out),
                          static_cast<int32_t>(env.row_bytes), env.dtype, elem > 0 ? elem : 1, 0, 0, 0};
  offsets(env.reward, env.is_first, env.is_last, env.is_terminal, &head.job.off_first, &head.job.off_last,
          &head.job.off_terminal);
  head.reward = env.reward;
  head.counters = env.counters;
  head.env0 = static_cast<int32_t>(env.env0);
  head.len_turn = static_cast<int32_t>(static_cast<uint32_t>(env.episode_len) |
                                       (static_cast<uint32_t>(env.turn & 1) << 31));
  head.scale = plan.scale;
  head.offset = plan.offset;
  head.n_narrow = plan.n_narrow;
  std::memcpy(dst, &head, sizeof(head));
  prewrite_fill_table(static_cast<uint8_t*>(dst) + sizeof(head), plan, rows, stepids);
}

}  // namespace synth_host
}  // namespace emb
