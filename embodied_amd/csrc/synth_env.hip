#include "device_util.h"
#include "step_device.h"
#include "synth_fused.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstring>

namespace emb {
namespace {

// ------------------------------------------------------------ synthetic env --

// Device-resident stand-in for N simulators: the episode logic
// of envs/dummy.py:38-48 with counter-hash frames, so gathers are verifiable.
//
// 56 bytes of arguments, passed as scalars so that the kernel-argument preload
// takes them (14 dwords; a by-value struct is not preloaded at all -- with
// host-resident arguments every wave would start with a PCIe read): the three
// flag outputs travel as 32-bit offsets from the reward pointer (the launcher
// falls back to the five-pointer form when they do not fit), the env count is
// the grid's y size, the generation bit rides in the sign bit of the episode
// length.  The per-env state is read from one half of `counters` and written to
// the other (`turn`), so that every workgroup of an env may read it while the
// last one writes: a frame is cut over gridDim.x workgroups instead of one.
struct SynthArgs {
  int32_t* counters;          // 2 x int32[2n]: {count, done} per env, two generations
  const uint8_t* reset;
  uint8_t* image;
  float* reward;
  int32_t off_first, off_last, off_terminal;   // bytes from `reward`
  int32_t frame_bytes, env0, episode_len, n_turn;   // n << 1 | turn
};
static_assert(sizeof(SynthArgs) <= 64, "synth_env_kernel's arguments (passed one by one, n from the grid) are preloaded");

using synth_host::SynthMaskJob;      // (the blocks in device memory and their host side: synth_fused.h)
using synth_host::SynthFusedHead;

struct SynthStep {
  int32_t count;
  bool restart, done;
};

__device__ __forceinline__ SynthStep synth_step(const SynthArgs& a, int64_t e) {
  const int32_t n = a.n_turn >> 1, turn = a.n_turn & 1;
  const int32_t* __restrict__ in = a.counters + turn * 2 * n;
  int32_t count = in[2 * e];
  const bool was_done = in[2 * e + 1] != 0;
  const bool restart = (a.reset && a.reset[e]) || was_done;
  const int64_t length = a.episode_len + ((a.env0 + e) % 8) * 13;
  count = restart ? 0 : count + 1;
  return {count, restart, !restart && count >= length};
}

__device__ __forceinline__ uint32_t synth_salt(int64_t env0, int64_t e, int32_t count) {
  return static_cast<uint32_t>((env0 + e) * 131 + static_cast<int64_t>(count) * 7);
}
// The four frame bytes from `byte0` on as one little-endian word.
__device__ __forceinline__ uint32_t synth_word(uint32_t salt, int64_t byte0) {
  const uint32_t x = salt + static_cast<uint32_t>(byte0);
  return (x & 0xFF) | (((x + 1) & 0xFF) << 8) | (((x + 2) & 0xFF) << 16) | (((x + 3) & 0xFF) << 24);
}

// byte i of the frame = (salt + i) & 0xFF, written 16 bytes per lane.
__device__ __forceinline__ void synth_frame(const SynthArgs& a, int64_t e, int32_t count, uint32_t blocks) {
  const uint32_t salt = synth_salt(a.env0, e, count);
  u32x4* out = reinterpret_cast<u32x4*>(a.image + e * a.frame_bytes);
  const int64_t vecs = a.frame_bytes >> 4;
  auto word = [salt](int64_t byte0) { return synth_word(salt, byte0); };
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < vecs;
       i += static_cast<int64_t>(blocks) * kThreads)
    __builtin_nontemporal_store(
        u32x4{word(i * 16), word(i * 16 + 4), word(i * 16 + 8), word(i * 16 + 12)}, out + i);
}

// Masked element `threadIdx.x` of env e's action row: stored to the job's `out`
// and returned (bits, zero-extended) -- what a simulator goes on with; this
// generator reads no action.  Called by workgroup 0 of the env only; one element
// per lane (rowbytes / elem <= kThreads: carry_supported, step.hip).
__device__ __forceinline__ uint64_t synth_masked_action(const SynthMaskJob& j, const uint8_t* reset, int64_t e) {
  const int64_t off = static_cast<int64_t>(threadIdx.x) * j.elem;
  if (!j.src || off >= j.rowbytes) return 0;
  const bool keep = !reset || gload<uint8_t>(reset + e) == 0;
  return put_masked_as(j.dtype, j.src + e * j.rowbytes + off, nullptr, j.out + e * j.rowbytes + off, keep);
}

__device__ __forceinline__ void synth_bookkeeping(const SynthArgs& a, int64_t e, const SynthStep& s,
                                                  uint8_t* is_first, uint8_t* is_last, uint8_t* is_terminal) {
  const int32_t n = a.n_turn >> 1, turn = a.n_turn & 1;
  int32_t* next = a.counters + (1 - turn) * 2 * n;
  next[2 * e] = s.count;
  next[2 * e + 1] = s.done ? 1 : 0;
  a.reward[e] = s.restart ? 0.f : static_cast<float>(s.count % 7);
  is_first[e] = s.restart ? 1 : 0;
  is_last[e] = s.done ? 1 : 0;
  is_terminal[e] = s.done ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void synth_env_kernel(
    int32_t* counters, const uint8_t* reset, uint8_t* image, float* reward, int32_t off_first,
    int32_t off_last, int32_t off_terminal, int32_t frame_bytes, int32_t env0, int32_t len_turn) {
  // 56 bytes = the 14 dwords the preload covers: the env count is the grid's y
  // size, the generation bit rides in the sign bit of the episode length.
  const SynthArgs a{counters, reset, image, reward, off_first, off_last, off_terminal,
                    frame_bytes, env0, len_turn & 0x7FFFFFFF,
                    static_cast<int32_t>(gridDim.y << 1 | (static_cast<uint32_t>(len_turn) >> 31))};
  const int64_t e = blockIdx.y;
  const SynthStep s = synth_step(a, e);
  synth_frame(a, e, s.count, gridDim.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    uint8_t* flags = reinterpret_cast<uint8_t*>(a.reward);
    synth_bookkeeping(a, e, s, flags + a.off_first, flags + a.off_last, flags + a.off_terminal);
  }
}

// The step with a mask job (see SynthMaskJob): 56 bytes of arguments, preloaded.
// The grid's size travels in them too -- the env count as the 14th dword, the
// workgroups per frame (1..4) less one in the low bits of the frame size, a
// multiple of 16: gridDim is itself a (hidden) kernel argument behind the
// preloaded ones, an s_load per wave in synth_env_kernel that this form does
// not have.
// `job` is DEVICE memory; workgroup 0 of an env reads it (uniform: scalar loads,
// issued beside the loads of the env's state), stores its frame share, then the
// masked action elements, one per lane, then the flags.
__global__ __launch_bounds__(kThreads) void synth_env_masked_kernel(
    int32_t* counters, const uint8_t* reset, uint8_t* image, float* reward,
    const SynthMaskJob* __restrict__ job, int32_t frame_bytes, int32_t env0, int32_t len_turn, int32_t n_envs) {
  const SynthArgs a{counters, reset, image, reward, 0, 0, 0,
                    frame_bytes & ~15, env0, len_turn & 0x7FFFFFFF,
                    static_cast<int32_t>(static_cast<uint32_t>(n_envs) << 1 | (static_cast<uint32_t>(len_turn) >> 31))};
  const uint32_t blocks = (static_cast<uint32_t>(frame_bytes) & 15u) + 1;     // = gridDim.x
  const int64_t e = blockIdx.y;
  if (blockIdx.x != 0) {
    synth_frame(a, e, synth_step(a, e).count, blocks);
    return;
  }
  const SynthMaskJob j = *job;
  const SynthStep s = synth_step(a, e);
  synth_frame(a, e, s.count, blocks);
  synth_masked_action(j, a.reset, e);
  if (threadIdx.x == 0) {
    uint8_t* flags = reinterpret_cast<uint8_t*>(a.reward);
    synth_bookkeeping(a, e, s, flags + j.off_first, flags + j.off_last, flags + j.off_terminal);
  }
}

// The same step when the flag buffers are too far from `reward` for 32-bit
// offsets (80 bytes of arguments + the mask job by value: nothing here is
// preloaded, every wave fetches its arguments).
__global__ __launch_bounds__(kThreads) void synth_env_far_kernel(
    const SynthArgs a, uint8_t* is_first, uint8_t* is_last, uint8_t* is_terminal, const SynthMaskJob j) {
  const int64_t e = blockIdx.y;
  const SynthStep s = synth_step(a, e);
  synth_frame(a, e, s.count, gridDim.x);
  if (blockIdx.x == 0) {
    synth_masked_action(j, a.reset, e);
    if (threadIdx.x == 0) synth_bookkeeping(a, e, s, is_first, is_last, is_terminal);
  }
}

// ------------------------------------------- step + obs stack + early insert --
//
// The masked step above writes every frame to the env's image buffer; one kernel
// boundary later obs_stack_insert_kernel (step.hip) reads the same bytes back to
// cast them into the policy batch and copy them into the replay's pool.  Nothing
// runs in between but the host, and the lane that generates 16 bytes of a frame
// holds them in registers: here it stores all three copies itself.  No workgroup
// depends on another, one boundary and the re-read of every frame are gone.
//
// The device block: synth_fused.h SynthFusedHead, then the early insert's table.
static_assert(kSynthFusedHeadBytes % alignof(PreTable) == 0, "the early insert's table follows the head");

// Grid as obs_stack_insert_kernel's (one dimension: the n narrow workgroups
// first, then the frame blocks env by env -- see its comment on XCD placement),
// frame slicing as obs_stack_insert_typed's: min(ceil(quads / 256), 32) blocks
// per env, so one lane owns the same 16 bytes for all three stores.  4 channels.
// 56 bytes of arguments = the 14 preloaded dwords; `counters_in` is the
// generation this step reads.
template <typename Out, bool kChannelsFirst>
__global__ __launch_bounds__(kThreads) void synth_env_fused_kernel(
    const int32_t* __restrict__ counters_in, const uint8_t* __restrict__ reset, uint8_t* image, void* dst,
    uint8_t* frame_pool, const SynthFusedHead* __restrict__ blk, int32_t frame_bytes, int32_t n_envs) {
  const PreTable& t = *reinterpret_cast<const PreTable*>(blk + 1);
  if (blockIdx.x < static_cast<uint32_t>(n_envs)) {
    const int64_t e = blockIdx.x;
    const SynthFusedHead h = *blk;                 // uniform: scalar loads
    const SynthArgs a{h.counters, reset, image, h.reward, 0, 0, 0, frame_bytes, h.env0, h.len_turn & 0x7FFFFFFF,
                      static_cast<int32_t>(static_cast<uint32_t>(n_envs) << 1 | (static_cast<uint32_t>(h.len_turn) >> 31))};
    const SynthStep s = synth_step(a, e);
    synth_masked_action(h.job, reset, e);
    uint8_t* flags = reinterpret_cast<uint8_t*>(h.reward);
    const uint8_t* first = flags + h.job.off_first;
    if (threadIdx.x == 0)
      synth_bookkeeping(a, e, s, flags + h.job.off_first, flags + h.job.off_last, flags + h.job.off_terminal);
    // The pool rows of reward and flags from the registers bookkeeping stored.
    const uint32_t reward_bits = __float_as_uint(s.restart ? 0.f : static_cast<float>(s.count % 7));
    const uint8_t* reward_src = reinterpret_cast<const uint8_t*>(h.reward);
    prewrite_narrow(t, n_envs, h.n_narrow, e, [&](const PreKey& key) -> uint8_t {
      if (key.src == reward_src) return static_cast<uint8_t>(reward_bits >> ((threadIdx.x & 3) * 8));
      if (key.src == first) return s.restart ? 1 : 0;
      return s.done ? 1 : 0;                       // is_last, is_terminal
    });
    return;
  }
  const uint32_t quads = static_cast<uint32_t>(frame_bytes) >> 4;
  const uint32_t frame_blocks = min((quads + kThreads - 1) / kThreads, 32u);
  const uint32_t id = blockIdx.x - static_cast<uint32_t>(n_envs);
  const int64_t e = id / frame_blocks;
  const uint32_t block = id - static_cast<uint32_t>(e) * frame_blocks;
  const int64_t row = static_cast<int32_t>(gload<uint32_t>(t.words + e));    // used by the pool store only
  const int32_t env0 = blk->env0;
  const float scale = blk->scale, offset = blk->offset;
  const bool restart = reset[e] != 0 || counters_in[2 * e + 1] != 0;
  const int32_t count = restart ? 0 : counters_in[2 * e] + 1;
  const uint32_t salt = synth_salt(env0, e, count);
  const int64_t pixels = static_cast<uint32_t>(frame_bytes) >> 2;
  u32x4* img = reinterpret_cast<u32x4*>(image + e * frame_bytes);
  u32x4* pool = reinterpret_cast<u32x4*>(frame_pool + row * frame_bytes);
  Out* out = static_cast<Out*>(dst) + e * pixels * 4;
  for (uint32_t q = block * kThreads + threadIdx.x; q < quads; q += frame_blocks * kThreads) {
    const int64_t b = static_cast<int64_t>(q) * 16;
    const uint32_t w[4] = {synth_word(salt, b), synth_word(salt, b + 4), synth_word(salt, b + 8),
                           synth_word(salt, b + 12)};
    __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, img + q);
    store_policy_quad<Out, 4, kChannelsFirst>(out, w, pixels, q, scale, offset);
    if (row >= 0) __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, pool + q);
  }
}

bool synth_args(SynthArgs* a, uint8_t* image, float* reward, int64_t n, int64_t frame_bytes, int64_t env0,
                int64_t episode_len, const uint8_t* reset, int32_t* counters, int turn, dim3* grid) {
  if (!synth_host::shape_ok(image, n, frame_bytes, env0, episode_len)) return false;
  a->counters = counters;
  a->reset = reset;
  a->image = image;
  a->reward = reward;
  a->off_first = a->off_last = a->off_terminal = 0;
  a->frame_bytes = static_cast<int32_t>(frame_bytes);
  a->env0 = static_cast<int32_t>(env0);
  a->episode_len = static_cast<int32_t>(episode_len);
  a->n_turn = static_cast<int32_t>(n << 1 | (turn & 1));
  // A frame over a few workgroups: 64 envs x 4 = one workgroup per CU.
  const int64_t vecs = frame_bytes >> 4;
  constexpr int64_t per_env = 4;
  const uint32_t gx = static_cast<uint32_t>(std::max<int64_t>(1, std::min<int64_t>(per_env, vecs / kThreads)));
  *grid = dim3(gx, static_cast<uint32_t>(n));
  return true;
}

using synth_host::offsets;
bool synth_offsets(const float* reward, const uint8_t* is_first, const uint8_t* is_last,
                   const uint8_t* is_terminal, int32_t* of, int32_t* ol, int32_t* ot) {
  return offsets(reward, is_first, is_last, is_terminal, of, ol, ot);
}

int32_t len_turn_word(const SynthArgs& a, int turn) {
  return static_cast<int32_t>(static_cast<uint32_t>(a.episode_len) | (static_cast<uint32_t>(turn & 1) << 31));
}

}  // namespace

hipError_t launch_synth_env(uint8_t* image, float* reward, uint8_t* is_first, uint8_t* is_last,
                            uint8_t* is_terminal, int64_t n, int64_t frame_bytes, int64_t env0,
                            int64_t episode_len, const uint8_t* reset, int32_t* counters, int turn,
                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  SynthArgs a;
  dim3 grid;
  if (!synth_args(&a, image, reward, n, frame_bytes, env0, episode_len, reset, counters, turn, &grid))
    return hipErrorInvalidValue;
  if (synth_offsets(reward, is_first, is_last, is_terminal, &a.off_first, &a.off_last, &a.off_terminal)) {
    hipLaunchKernelGGL(synth_env_kernel, grid, dim3(kThreads), 0, stream, a.counters, a.reset, a.image,
                       a.reward, a.off_first, a.off_last, a.off_terminal, a.frame_bytes, a.env0,
                       len_turn_word(a, turn));
  } else {
    hipLaunchKernelGGL(synth_env_far_kernel, grid, dim3(kThreads), 0, stream, a, is_first, is_last,
                       is_terminal, SynthMaskJob{nullptr, nullptr, 0, 0, 1, 0, 0, 0});
  }
  return hipGetLastError();
}

bool synth_mask_job(void* job, const void* act, void* masked_out, int64_t rowbytes, int dtype,
                    const float* reward, const uint8_t* is_first, const uint8_t* is_last,
                    const uint8_t* is_terminal) {
  SynthMaskJob j{static_cast<const uint8_t*>(act), static_cast<uint8_t*>(masked_out),
                 static_cast<int32_t>(rowbytes), dtype, std::max(dtype_size(dtype), 1), 0, 0, 0};
  const bool near = synth_offsets(reward, is_first, is_last, is_terminal, &j.off_first, &j.off_last,
                                  &j.off_terminal);
  std::memcpy(job, &j, sizeof(j));
  return near;
}

hipError_t launch_synth_env_masked(uint8_t* image, float* reward, uint8_t* is_first, uint8_t* is_last,
                                   uint8_t* is_terminal, int64_t n, int64_t frame_bytes, int64_t env0,
                                   int64_t episode_len, const uint8_t* reset, int32_t* counters, int turn,
                                   const void* job_host, const void* job_dev, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  SynthMaskJob j;
  std::memcpy(&j, job_host, sizeof(j));
  if (!j.src || !j.out || !carry_supported(j.rowbytes, j.dtype) || j.elem != dtype_size(j.dtype))
    return hipErrorInvalidValue;
  SynthArgs a;
  dim3 grid;
  if (!synth_args(&a, image, reward, n, frame_bytes, env0, episode_len, reset, counters, turn, &grid))
    return hipErrorInvalidValue;
  if (job_dev) {
    hipLaunchKernelGGL(synth_env_masked_kernel, grid, dim3(kThreads), 0, stream, a.counters, a.reset, a.image,
                       a.reward, static_cast<const SynthMaskJob*>(job_dev),
                       a.frame_bytes | static_cast<int32_t>(grid.x - 1), a.env0,
                       len_turn_word(a, turn), static_cast<int32_t>(n));
  } else {
    hipLaunchKernelGGL(synth_env_far_kernel, grid, dim3(kThreads), 0, stream, a, is_first, is_last,
                       is_terminal, j);
  }
  return hipGetLastError();
}

const char* synth_fused_refusal(const SynthStepArgs& env, const PrewritePlan& plan) {
  return synth_host::fused_refusal(env, plan);
}

size_t synth_fused_block_bytes(int64_t n) { return synth_host::fused_block_bytes(n); }

void synth_fused_fill(void* dst, const SynthStepArgs& env, const PrewritePlan& plan, const int32_t* rows,
                      const uint8_t* stepids) {
  synth_host::fused_fill(dst, env, dtype_size(env.dtype), plan, rows, stepids);
}

// (The caller has asked synth_fused_refusal: replay_early_insert does, before it touches its handle.)
hipError_t launch_synth_env_fused(const SynthStepArgs& env, const PrewritePlan& plan, const void* block_dev,
                                  hipStream_t stream, hipEvent_t stop) {
  if (!block_dev || plan.channels != 4 || plan.n != env.n) return hipErrorInvalidValue;
  const uint32_t quads = static_cast<uint32_t>(env.frame_bytes >> 4);
  const uint32_t frame_blocks = std::min<uint32_t>((quads + kThreads - 1) / kThreads, 32u);
  const dim3 grid(static_cast<uint32_t>(env.n) * (frame_blocks + 1));
  const int32_t* counters_in = env.counters + (env.turn & 1) * 2 * env.n;
  const bool cf = plan.layout == kLayoutChannelsFirst;
#define EMB_FUSED_ARGS counters_in, env.reset, env.image, plan.dst, plan.frame_pool,                   \
                       static_cast<const SynthFusedHead*>(block_dev), static_cast<int32_t>(env.frame_bytes), \
                       static_cast<int32_t>(env.n)
#define EMB_FUSED(Out)                                                                                  \
  if (cf && stop) hipExtLaunchKernelGGL((synth_env_fused_kernel<Out, true>), grid, dim3(kThreads), 0,  \
                                        stream, nullptr, stop, 0, EMB_FUSED_ARGS);                      \
  else if (cf) hipLaunchKernelGGL((synth_env_fused_kernel<Out, true>), grid, dim3(kThreads), 0, stream, \
                                  EMB_FUSED_ARGS);                                                      \
  else if (stop) hipExtLaunchKernelGGL((synth_env_fused_kernel<Out, false>), grid, dim3(kThreads), 0,  \
                                       stream, nullptr, stop, 0, EMB_FUSED_ARGS);                       \
  else hipLaunchKernelGGL((synth_env_fused_kernel<Out, false>), grid, dim3(kThreads), 0, stream,       \
                          EMB_FUSED_ARGS);
  switch (plan.out_dtype) {
    case kU8: EMB_FUSED(uint8_t) break;
    case kF16: EMB_FUSED(__half) break;
    case kBF16: EMB_FUSED(__hip_bfloat16) break;
    default: EMB_FUSED(float) break;
  }
#undef EMB_FUSED
#undef EMB_FUSED_ARGS
  return hipGetLastError();
}

}  // namespace emb
