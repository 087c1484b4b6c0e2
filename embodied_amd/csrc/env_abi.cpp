// The device env's step with the action mask inside its launch
// (emb_synth_env_step_masked): its own translation unit because it owns the
// argument rings the mask job travels through -- one per device, process-wide,
// not tied to any replay handle (an env has none).
#include "handles.h"

namespace {

std::mutex g_env_mu;

// The ring of the calling thread's current device (made on first use, leaked on
// purpose like global_ring(): HIP may be gone at exit).
ArgRing& env_ring() {
  static std::vector<ArgRing*>* rings = new std::vector<ArgRing*>();
  int device = 0;
  HIP_OK(hipGetDevice(&device));
  if (static_cast<size_t>(device) >= rings->size()) rings->resize(device + 1, nullptr);
  if (!(*rings)[device]) (*rings)[device] = new ArgRing();
  return *(*rings)[device];
}

}  // namespace

extern "C" {

int32_t emb_env_mask_supported(int64_t row_bytes, int32_t dtype) {
  return dtype >= 0 && dtype <= emb::kBool && emb::carry_supported(row_bytes, dtype) ? 1 : 0;
}

int32_t emb_synth_env_step_masked(void* image, void* reward, void* is_first, void* is_last, void* is_terminal,
                                  int64_t n, int64_t frame_bytes, int64_t env0, int64_t episode_len,
                                  const void* reset, void* counters, int32_t turn, const void* act,
                                  void* masked_out, int64_t row_bytes, int32_t dtype, void* stream) {
  return guarded([&] {
    need(image && reward && is_first && is_last && is_terminal && counters && n >= 0 && episode_len >= 1,
         "synth_env_step_masked: bad arguments");
    need(act && masked_out && reset, "synth_env_step_masked: the mask job needs the actions, their destination and the flags (reset)");
    need(emb_env_mask_supported(row_bytes, dtype) == 1,
         "synth_env_step_masked: an action row must be 1..256 elements of a known dtype");
    if (n == 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t job[emb::kSynthJobBytes];
    const bool near = emb::synth_mask_job(job, act, masked_out, row_bytes, dtype, static_cast<const float*>(reward),
                                          static_cast<const uint8_t*>(is_first), static_cast<const uint8_t*>(is_last),
                                          static_cast<const uint8_t*>(is_terminal));
    auto launch = [&](const void* job_dev) {
      HIP_OK(emb::launch_synth_env_masked(
          static_cast<uint8_t*>(image), static_cast<float*>(reward), static_cast<uint8_t*>(is_first),
          static_cast<uint8_t*>(is_last), static_cast<uint8_t*>(is_terminal), n, frame_bytes, env0, episode_len,
          static_cast<const uint8_t*>(reset), static_cast<int32_t*>(counters), turn, job, job_dev, s));
    };
    HostLap hp;
    if (!near) {
      launch(nullptr);          // far flag buffers: the job goes by value
    } else {
      std::lock_guard<std::mutex> lock(g_env_mu);
      ArgRing& ring = env_ring();
      if (ring.usable()) {
        const void* dev = ring.put(job, sizeof(job), s);
        launch(dev);
        ring.retire(s);
      } else {
        // No large BAR: the block is uploaded (a copy per step; correct, not fast).
        std::lock_guard<std::mutex> ring_lock(g_ring_mu);
        auto lease = global_ring().acquire(sizeof(job), s);
        std::memcpy(lease.host, job, sizeof(job));
        global_ring().upload(lease, sizeof(job), s);
        launch(lease.device);
        global_ring().retire(lease, s);
      }
    }
    hp.lap(21, "synthetic env: launch");
  });
}

// EMB_STEP_FUSED=0: the env step and the early insert stay two launches.
static bool step_fused() {
  static const bool on = [] {
    const char* v = emb::knob("EMB_STEP_FUSED");
    return !(v && v[0] == '0');
  }();
  return on;
}

int32_t emb_synth_env_step_fused(emb_replay_t* rep, int64_t n, const int64_t* workers, int32_t frame_key,
                                 const emb_synth_step_t* env, const emb_obs_spec_t* spec, void* dst,
                                 const void* const* src, void* stream, uint64_t* token_out) {
  return guarded([&] {
    need(rep && env && token_out, "synth_env_step_fused: bad arguments");
    *token_out = 0;
    if (!step_fused()) return;
    emb::SynthStepArgs a;
    a.image = static_cast<uint8_t*>(env->image);
    a.reward = static_cast<float*>(env->reward);
    a.is_first = static_cast<uint8_t*>(env->is_first);
    a.is_last = static_cast<uint8_t*>(env->is_last);
    a.is_terminal = static_cast<uint8_t*>(env->is_terminal);
    a.n = env->n;
    a.frame_bytes = env->frame_bytes;
    a.env0 = env->env0;
    a.episode_len = env->episode_len;
    a.reset = static_cast<const uint8_t*>(env->reset);
    a.counters = static_cast<int32_t*>(env->counters);
    a.turn = env->turn;
    a.act = env->act;
    a.masked_out = env->masked_out;
    a.row_bytes = env->row_bytes;
    a.dtype = env->dtype;
    need(n == env->n && n > 0, "synth_env_step_fused: the replay's workers are not the env's n envs");
    need(a.dtype >= 0 && a.dtype <= emb::kBool, "synth_env_step_fused: bad action dtype");
    StepLaunch step;
    step.ctx = &a;
    step.refusal = [](void* ctx, const emb::PrewritePlan& plan) {
      return emb::synth_fused_refusal(*static_cast<emb::SynthStepArgs*>(ctx), plan);
    };
    step.bytes = [](void*, int64_t n_envs) { return emb::synth_fused_block_bytes(n_envs); };
    step.fill = [](void* ctx, void* block, const emb::PrewritePlan& plan, const int32_t* rows,
                   const uint8_t* stepids) {
      emb::synth_fused_fill(block, *static_cast<emb::SynthStepArgs*>(ctx), plan, rows, stepids);
    };
    step.launch = [](void* ctx, const emb::PrewritePlan& plan, hipStream_t s, hipEvent_t stop) {
      return emb::launch_synth_env_fused(*static_cast<emb::SynthStepArgs*>(ctx), plan, plan.table_dev, s, stop);
    };
    HostLap hp;
    replay_early_insert(rep, n, workers, frame_key, env->image, spec, dst, src, stream, token_out, &step);
    hp.lap(21, "synthetic env: launch");
  });
}

}  // extern "C"
