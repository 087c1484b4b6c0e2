// TEST INFRASTRUCTURE: the host side of the device env's fused step
// (embodied_amd/csrc/synth_fused.h) against tests/fake_hip, no GPU: every refusal
// of emb_synth_env_step_fused's launch, and the layout of the device block that
// synth_env_fused_kernel reads (96-byte head, the early insert's table behind it).
// Prints one line per check; exit status = number of failed checks.
#include "synth_fused.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace emb;
using namespace emb::synth_host;

static int failed = 0;
static void check(bool ok, const char* what) {
  std::printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  failed += !ok;
}
static bool refused(const SynthStepArgs& env, const PrewritePlan& plan, const char* word) {
  const char* why = fused_refusal(env, plan);
  return why && std::strstr(why, word);
}
template <typename T>
static T at(const std::vector<uint8_t>& block, size_t offset) {
  T v;
  std::memcpy(&v, block.data() + offset, sizeof(T));
  return v;
}

int main() {
  constexpr int n = 3;
  constexpr int64_t pixels = 64, frame = pixels * 4;
  alignas(16) static uint8_t image[n * frame], pool[8 * frame];
  alignas(16) static uint16_t batch[n * frame];
  alignas(16) static float reward[n];
  static uint8_t first[n], last[n], terminal[n], reset[n], foreign[n];
  static uint8_t pool_reward[8 * 4], pool_first[8], pool_last[8], pool_terminal[8], pool_sid[8 * kStepBytes];
  static int32_t counters[4 * n], act[n], masked[n], rows_out[n];

  SynthStepArgs env;
  env.image = image;
  env.reward = reward;
  env.is_first = first;
  env.is_last = last;
  env.is_terminal = terminal;
  env.n = n;
  env.frame_bytes = frame;
  env.env0 = 5;
  env.episode_len = 7;
  env.reset = reset;
  env.counters = counters;
  env.turn = 1;
  env.act = act;
  env.masked_out = masked;
  env.row_bytes = 4;
  env.dtype = kI32;

  PrewritePlan plan;
  plan.frames = image;
  plan.dst = batch;
  plan.frame_pool = pool;
  plan.pixels = pixels;
  plan.channels = 4;
  plan.layout = kLayoutChannelsFirst;
  plan.out_dtype = kBF16;
  plan.scale = 0.25f;
  plan.offset = -1.5f;
  plan.n = n;
  plan.n_narrow = 4;
  plan.narrow[0] = {reinterpret_cast<const uint8_t*>(reward), pool_reward, 4};
  plan.narrow[1] = {first, pool_first, 1};
  plan.narrow[2] = {last, pool_last, 1};
  plan.narrow[3] = {terminal, pool_terminal, 1};
  plan.stepid_pool = pool_sid;
  plan.rows_out = rows_out;

  // ---- refusals: each names its reason, the good plan has none ----
  check(fused_refusal(env, plan) == nullptr, "a plan of the env's own buffers is taken");
  {
    PrewritePlan p = plan;
    p.pixels = 62;                                   // not a multiple of 4: the early insert's own check
    check(refused(env, p, "prewrite_supported"), "a plan prewrite_supported fails is refused");
    p = plan;
    p.n_narrow = kPreNarrow + 1;
    check(refused(env, p, "prewrite_supported"), "too many narrow keys are refused");
    p = plan;
    p.channels = 3;
    p.pixels = 64;
    check(fused_refusal(env, p) != nullptr, "3-channel frames are refused");
    p = plan;
    p.channels = 2;
    p.pixels = 128;                                  // same frame bytes, still not 4 channels
    check(refused(env, p, "4-channel"), "2-channel frames of the same size are refused");
    p = plan;
    p.frames = pool;
    check(refused(env, p, "image buffer"), "frames that are not the env's image buffer are refused");
    p = plan;
    p.n = n - 1;
    check(refused(env, p, "image buffer"), "a plan for another env count is refused");
    p = plan;
    p.narrow[2].src = foreign;
    check(refused(env, p, "four output buffers"), "a narrow key from a foreign buffer is refused");
    p = plan;
    p.narrow[0].rowbytes = 8;
    check(refused(env, p, "four output buffers"), "reward rows that are not 4 bytes are refused");
    p = plan;
    p.narrow[1].rowbytes = 2;
    check(refused(env, p, "four output buffers"), "flag rows that are not 1 byte are refused");
    p = plan;
    p.out_dtype = kI64;
    check(fused_refusal(env, p) != nullptr, "a policy batch dtype the launch does not write is refused");
  }
  {
    SynthStepArgs e = env;
    // (addresses only: never dereferenced)
    e.is_last = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(reward) + (uintptr_t{1} << 33));
    PrewritePlan p = plan;
    p.narrow[2].src = e.is_last;
    check(refused(e, p, "32-bit offsets"), "flag buffers beyond 32-bit offsets of reward are refused");
    e = env;
    e.row_bytes = 257 * 4;
    check(refused(e, plan, "mask job"), "an action row of more than 256 elements is refused");
    e = env;
    e.dtype = 99;
    check(refused(e, plan, "mask job"), "an unknown action dtype is refused");
    e = env;
    e.reset = nullptr;
    check(refused(e, plan, "mask job"), "a step without reset flags is refused");
    e = env;
    e.act = nullptr;
    check(refused(e, plan, "mask job"), "a step without actions is refused");
    e = env;
    e.counters = nullptr;
    check(refused(e, plan, "bad env"), "a step without counters is refused");
    e = env;
    e.episode_len = 0;
    check(refused(e, plan, "bad env"), "an episode length below 1 is refused");
  }

  // ---- the device block ----
  const int32_t rows[n] = {4, -1, 6};
  uint8_t ids[n * kStepBytes];
  for (int i = 0; i < n * kStepBytes; ++i) ids[i] = static_cast<uint8_t>(i + 1);
  const size_t bytes = fused_block_bytes(n);
  check(bytes == kSynthFusedHeadBytes + prewrite_table_bytes(n) && kSynthFusedHeadBytes == 96,
        "block = 96-byte head + the early insert's table");
  std::vector<uint8_t> block(bytes + 16, 0xA5);
  fused_fill(block.data(), env, 4, plan, rows, ids);
  bool canary = true;
  for (size_t i = bytes; i < bytes + 16; ++i) canary = canary && block[i] == 0xA5;
  check(canary, "the fill stays inside fused_block_bytes(n)");
  // head, field by field at the offsets synth_env_fused_kernel reads
  check(at<const void*>(block, 0) == act && at<void*>(block, 8) == masked, "head +0/+8: mask job source and destination");
  check(at<int32_t>(block, 16) == 4 && at<int32_t>(block, 20) == kI32 && at<int32_t>(block, 24) == 4,
        "head +16..+24: row bytes, dtype, element bytes");
  check(at<int32_t>(block, 28) == static_cast<int32_t>(first - reinterpret_cast<uint8_t*>(reward)) &&
            at<int32_t>(block, 32) == static_cast<int32_t>(last - reinterpret_cast<uint8_t*>(reward)) &&
            at<int32_t>(block, 36) == static_cast<int32_t>(terminal - reinterpret_cast<uint8_t*>(reward)),
        "head +28..+36: flag offsets from reward");
  check(at<uint64_t>(block, 40) == 0, "head +40: padding of the 48-byte job is zero");
  check(at<float*>(block, 48) == reward && at<int32_t*>(block, 56) == counters, "head +48/+56: reward, counters");
  check(at<int32_t>(block, 64) == 5 && at<uint32_t>(block, 68) == (7u | 1u << 31), "head +64/+68: env0, episode length | turn << 31");
  check(at<float>(block, 72) == 0.25f && at<float>(block, 76) == -1.5f, "head +72/+76: scale, offset");
  check(at<int32_t>(block, 80) == 4 && at<int32_t>(block, 84) == 0 && at<int32_t>(block, 88) == 0 &&
            at<int32_t>(block, 92) == 0, "head +80..+92: narrow count, zero padding");
  // the early insert's table starts right behind the head: what prewrite_fill_table
  // wrote (here the fake's: the plan first, then rows and step ids at the end)
  check(at<const void*>(block, 96) == static_cast<const void*>(image), "block +96: the early insert's table begins");
  const size_t tail = 96 + prewrite_table_bytes(n) - static_cast<size_t>(n) * (4 + kStepBytes + 4);
  check(std::memcmp(block.data() + tail, rows, sizeof(rows)) == 0 &&
            std::memcmp(block.data() + tail + sizeof(rows), ids, sizeof(ids)) == 0,
        "the table's rows and step ids are the ones given");
  // turn 0 leaves the sign bit clear
  SynthStepArgs even = env;
  even.turn = 0;
  fused_fill(block.data(), even, 4, plan, rows, ids);
  check(at<uint32_t>(block, 68) == 7u, "turn 0: episode length alone");
  std::printf("%d failed\n", failed);
  return failed;
}
