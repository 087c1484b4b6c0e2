// The reference's optimizer chain (dreamerv3/agent.py:342-379) over every
// parameter tensor of a learner in two launches:
//   clip_by_agc        embodied/jax/opt.py:109-123   two norms per tensor
//   scale_by_rms       embodied/jax/opt.py:126-143
//   scale_by_momentum  embodied/jax/opt.py:146-164
//   add_decayed_weights, scale_by_learning_rate, apply_updates   agent.py:361-378
// With torch ops the same is two reductions and about ten elementwise passes per
// tensor, a few thousand device operations per step for a few hundred tensors.
//
//   norms    every chunk's sum g^2 and sum p^2 into the partials buffer
//   update   each workgroup sums ITS tensor's partials in a fixed order, forms the
//            scale, updates its chunk: reads g, p, nu, mu, writes p, nu, mu, and
//            leaves the chunk's sum upd^2 and sum p_new^2 behind
//   metrics  (only when asked) one workgroup sums the partials of all chunks
// A tensor's scale needs all of its gradient: the boundary between the launches
// is that synchronisation.  No atomics, no workgroup waits for another one: the
// same bits run to run.
//
// The PPO learner's chain (ppo/agent.py:114-124: clip_by_global_norm,
// scale_by_adam, add_decayed_weights, scale_by_learning_rate) runs on the same
// tables and partials: its norms launch leaves sum g^2 only and never reads p, its
// update launch sums the partials of ALL chunks, once per workgroup, for the one
// global norm.
//
// The slow (EMA) copy of a set of tensors (embodied/jax/utils.py:94-127,
// dreamerv3/agent.py:142) is one more pass over such a chunk map: a launch of its
// own (slow_update_kernel), or no launch at all -- the SLOW instantiations of the
// two update kernels write it from the p_new they still hold in registers.
//
// One workgroup per chunk of kOptimChunk elements of one tensor (grid-stride past
// kMaxBlocks), 16-byte loads and stores from the chunk's first aligned element
// on and scalar ones at its ragged ends (optim.h: optim_plan decides per tensor).
#include "optim.h"
#include "wave_util.h"

// float32 operations one by one, as the composed path
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kMetricThreads = 1024;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups on each of 256 CUs; more chunks: grid stride
static_assert(kOptimChunk % (4 * kThreads) == 0, "a full chunk is whole rounds of one vector per thread");

using namespace segment;                          // widen, wave_sum
static_assert(kWave == kLanes, "the wave helpers shuffle over one wave64");

// jnp.maximum / torch.maximum: a NaN on either side is the result (fmaxf drops it)
__device__ __forceinline__ float maximum(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }

// The workgroup's sums of a and b, the same bits in every thread: each wave's
// butterfly, then the waves in their order.
template <int THREADS>
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*lds)[THREADS / kWave]) {
  constexpr int kWaves = THREADS / kWave;
  a = wave_sum(a);
  b = wave_sum(b);
  if (threadIdx.x % kWave == 0) {
    lds[0][threadIdx.x / kWave] = a;
    lds[1][threadIdx.x / kWave] = b;
  }
  __syncthreads();
  a = 0.f;
  b = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    a = a + lds[0][w];
    b = b + lds[1][w];
  }
  __syncthreads();                                 // the next call writes lds again
}

template <bool BF16>
__device__ __forceinline__ float grad_at(const void* g, int64_t i) {
  if constexpr (BF16) return widen(static_cast<const bf16_t*>(g)[i]);
  else return static_cast<const float*>(g)[i];
}

template <bool BF16>
__device__ __forceinline__ float4 grad4_at(const void* g, int64_t i) {           // i: an aligned element
  if constexpr (BF16) {
    const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(g) + i);
    return make_float4(__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u),
                       __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u));
  } else {
    return *reinterpret_cast<const float4*>(static_cast<const float*>(g) + i);
  }
}

// The parts of the chunk [lo, hi): scalars [lo, first), vectors of 4 from `first`,
// scalars [tail, hi).  Without the vector flag everything is [lo, first).
struct Span {
  int32_t lo, first, nvec, tail, hi;
};

template <class Tensor>                            // OptimTensor or SlowTensor
__device__ __forceinline__ Span span_of(const Tensor& t, int32_t offset) {
  Span s;
  s.lo = offset;
  s.hi = min(t.n - offset, kOptimChunk) + offset;
  if (t.flags & kOptimVector) {
    s.first = min(s.lo + t.head, s.hi);
    s.nvec = (s.hi - s.first) / 4;
    s.tail = s.first + 4 * s.nvec;
  } else {
    s.first = s.hi;
    s.nvec = 0;
    s.tail = s.hi;
  }
  return s;
}

template <class Tensor>
__device__ __forceinline__ Tensor tensor_of(const Tensor* table, const OptimChunk* chunks, int32_t chunk,
                                            int32_t& tensor, int32_t& offset) {
  // the same in every lane: read through scalar registers
  tensor = __builtin_amdgcn_readfirstlane(chunks[chunk].tensor);
  offset = __builtin_amdgcn_readfirstlane(chunks[chunk].offset);
  return table[tensor];
}

// PARAMS: the chunk's sum p^2 as well (AGC needs it); without, p is never read
// and psq stays as it came.
template <bool BF16, bool PARAMS>
__device__ __forceinline__ void norms_chunk(const OptimTensor& t, const Span& s, float& gsq, float& psq) {
  const float* p = reinterpret_cast<const float*>(t.p);
  const void* g = reinterpret_cast<const void*>(t.g);
  const int tid = threadIdx.x;
  for (int64_t i = static_cast<int64_t>(s.lo) + tid; i < s.first; i += kThreads) {
    const float gv = grad_at<BF16>(g, i);
    gsq = gsq + gv * gv;
    if constexpr (PARAMS) {
      const float pv = p[i];
      psq = psq + pv * pv;
    }
  }
#pragma unroll 4
  for (int32_t v = tid; v < s.nvec; v += kThreads) {
    const int32_t i = s.first + 4 * v;
    const float4 gv = grad4_at<BF16>(g, i);
    gsq = gsq + ((gv.x * gv.x + gv.y * gv.y) + (gv.z * gv.z + gv.w * gv.w));
    if constexpr (PARAMS) {
      const float4 pv = *reinterpret_cast<const float4*>(p + i);
      psq = psq + ((pv.x * pv.x + pv.y * pv.y) + (pv.z * pv.z + pv.w * pv.w));
    }
  }
  for (int64_t i = static_cast<int64_t>(s.tail) + tid; i < s.hi; i += kThreads) {
    const float gv = grad_at<BF16>(g, i);
    gsq = gsq + gv * gv;
    if constexpr (PARAMS) {
      const float pv = p[i];
      psq = psq + pv * pv;
    }
  }
}

// PARAMS = false (the Adam chain): row 0 of the partials only.
template <bool PARAMS>
__global__ __launch_bounds__(kThreads) void optim_norms_kernel(const OptimTensor* __restrict__ table,
                                                               const OptimChunk* __restrict__ chunks, int32_t n_chunks,
                                                               float* __restrict__ partials) {
  __shared__ float lds[2][kThreads / kWave];
  for (int32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    int32_t tensor, offset;
    const OptimTensor t = tensor_of(table, chunks, chunk, tensor, offset);
    const Span s = span_of(t, offset);
    float gsq = 0.f, psq = 0.f;
    if (t.flags & kOptimBf16) norms_chunk<true, PARAMS>(t, s, gsq, psq);
    else norms_chunk<false, PARAMS>(t, s, gsq, psq);
    block_sum2<kThreads>(gsq, psq, lds);
    if (threadIdx.x == 0) {
      partials[chunk] = gsq;
      if constexpr (PARAMS) partials[static_cast<int64_t>(n_chunks) + chunk] = psq;
    }
  }
}

// One element of the chain; `usq` and `pnsq` collect upd^2 and p_new^2.
__device__ __forceinline__ void update_one(float g, float& p, float& nu, float& mu, float scale, bool decay,
                                           const OptimStep& s, float& usq, float& pnsq) {
  const float g1 = g * scale;                                      // opt.py:119
  nu = s.beta2 * nu + s.omb2 * (g1 * g1);                          // opt.py:136-137
  const float u = g1 / (sqrtf(nu / s.c2) + s.eps);                 // opt.py:138-140
  mu = s.omb1 * u + s.beta1 * mu;                                  // opt.py:156, optax.update_moment
  float m = s.nesterov ? s.omb1 * u + s.beta1 * mu : mu;           // opt.py:157-161
  m = m / s.c1;
  if (decay) m = m + s.wd * p;                                     // agent.py:365, optax.add_decayed_weights
  const float upd = m * -s.lr;                                     // agent.py:378, optax.scale_by_learning_rate
  p = p + upd;                                                     // optax.apply_updates
  usq = usq + upd * upd;
  pnsq = pnsq + p * p;
}

// The slow copy of one element (utils.py:118): two products and one sum.
__device__ __forceinline__ float slow_one(float src, float dst, float mix, float omm) { return mix * src + omm * dst; }

// The four elements of a slow copy at d + i: one 16-byte access where `d + i` is
// aligned (VECTOR), else four scalar ones.  Read with the step's other loads,
// written from p_new right after p was.
template <bool VECTOR>
__device__ __forceinline__ float4 slow_load4(const float* d, int32_t i) {
  if constexpr (VECTOR) return *reinterpret_cast<const float4*>(d + i);
  else return make_float4(d[i], d[i + 1], d[i + 2], d[i + 3]);
}

template <bool VECTOR>
__device__ __forceinline__ void slow_store4(float* d, int32_t i, const float4& pv, float4 dv, float mix, float omm) {
  dv.x = slow_one(pv.x, dv.x, mix, omm);
  dv.y = slow_one(pv.y, dv.y, mix, omm);
  dv.z = slow_one(pv.z, dv.z, mix, omm);
  dv.w = slow_one(pv.w, dv.w, mix, omm);
  if constexpr (VECTOR) {
    *reinterpret_cast<float4*>(d + i) = dv;
  } else {
    d[i] = dv.x, d[i + 1] = dv.y, d[i + 2] = dv.z, d[i + 3] = dv.w;
  }
}

// Whether the slow copy at address `d` of a tensor on the vector path takes
// 16-byte accesses too: aligned at element `head`, hence at the first vector of
// every chunk.  The same in every lane.
__device__ __forceinline__ bool slow_aligned(const OptimTensor& t, uint64_t d) {
  return __builtin_amdgcn_readfirstlane(static_cast<int32_t>((d + 4u * static_cast<uint32_t>(t.head)) & 15u)) == 0;
}

// SLOW: `d` is the tensor's slow copy, written from p_new at the same index;
// SLOW_VECTOR: in 16-byte accesses on the vector path.  Without SLOW, `d`, `mix`
// and `omm` are not looked at.
template <bool BF16, bool SLOW = false, bool SLOW_VECTOR = false>
__device__ __forceinline__ void update_chunk(const OptimTensor& t, const Span& s, float scale, const OptimStep& step,
                                             float& usq, float& pnsq, float* d = nullptr, float mix = 0.f,
                                             float omm = 0.f) {
  float* p = reinterpret_cast<float*>(t.p);
  float* nu = reinterpret_cast<float*>(t.nu);
  float* mu = reinterpret_cast<float*>(t.mu);
  const void* g = reinterpret_cast<const void*>(t.g);
  const bool decay = t.flags & kOptimDecay;
  const int tid = threadIdx.x;
  for (int64_t i = static_cast<int64_t>(s.lo) + tid; i < s.first; i += kThreads) {
    float pv = p[i], nv = nu[i], mv = mu[i];
    update_one(grad_at<BF16>(g, i), pv, nv, mv, scale, decay, step, usq, pnsq);
    p[i] = pv, nu[i] = nv, mu[i] = mv;
    if constexpr (SLOW) d[i] = slow_one(pv, d[i], mix, omm);
  }
  // two steps in flight; with the slow copy's registers on top that costs a wave
  // per SIMD (85 VGPRs against 76), so the SLOW instantiations take one
  constexpr int kSteps = SLOW ? 1 : 2;
#pragma unroll kSteps
  for (int32_t v = tid; v < s.nvec; v += kThreads) {
    const int32_t i = s.first + 4 * v;
    const float4 gv = grad4_at<BF16>(g, i);
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    float4 nv = *reinterpret_cast<const float4*>(nu + i);
    float4 mv = *reinterpret_cast<const float4*>(mu + i);
    [[maybe_unused]] float4 dv;
    if constexpr (SLOW) dv = slow_load4<SLOW_VECTOR>(d, i);
    update_one(gv.x, pv.x, nv.x, mv.x, scale, decay, step, usq, pnsq);
    update_one(gv.y, pv.y, nv.y, mv.y, scale, decay, step, usq, pnsq);
    update_one(gv.z, pv.z, nv.z, mv.z, scale, decay, step, usq, pnsq);
    update_one(gv.w, pv.w, nv.w, mv.w, scale, decay, step, usq, pnsq);
    *reinterpret_cast<float4*>(p + i) = pv;
    if constexpr (SLOW) slow_store4<SLOW_VECTOR>(d, i, pv, dv, mix, omm);
    *reinterpret_cast<float4*>(nu + i) = nv;
    *reinterpret_cast<float4*>(mu + i) = mv;
  }
  for (int64_t i = static_cast<int64_t>(s.tail) + tid; i < s.hi; i += kThreads) {
    float pv = p[i], nv = nu[i], mv = mu[i];
    update_one(grad_at<BF16>(g, i), pv, nv, mv, scale, decay, step, usq, pnsq);
    p[i] = pv, nu[i] = nv, mu[i] = mv;
    if constexpr (SLOW) d[i] = slow_one(pv, d[i], mix, omm);
  }
}

// SLOW: slow[tensor] is the address of that tensor's slow copy, 0 for none; it,
// `mix` and `omm` are read by the SLOW instantiation only.
template <bool SLOW>
__global__ __launch_bounds__(kThreads) void optim_update_kernel(const OptimTensor* __restrict__ table,
                                                                const OptimChunk* __restrict__ chunks, int32_t n_chunks,
                                                                float* __restrict__ partials, const OptimStep step,
                                                                const uint64_t* __restrict__ slow, float mix,
                                                                float omm) {
  __shared__ float lds[2][kThreads / kWave];
  const float* gsq_of = partials;
  const float* psq_of = partials + n_chunks;
  float* usq_of = partials + 2 * static_cast<int64_t>(n_chunks);
  float* pnsq_of = partials + 3 * static_cast<int64_t>(n_chunks);
  int32_t scaled = -1;                              // the tensor `scale` belongs to
  float scale = 1.f;
  for (int32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    int32_t tensor, offset;
    const OptimTensor t = tensor_of(table, chunks, chunk, tensor, offset);
    if (step.agc != 0.f && tensor != scaled) {      // opt.py:116-120; uniform over the workgroup
      const int32_t count = (t.n + kOptimChunk - 1) / kOptimChunk;
      float gsq = 0.f, psq = 0.f;
      for (int32_t k = threadIdx.x; k < count; k += kThreads) {
        gsq = gsq + gsq_of[t.first_chunk + k];
        psq = psq + psq_of[t.first_chunk + k];
      }
      block_sum2<kThreads>(gsq, psq, lds);
      const float unorm = sqrtf(gsq), pnorm = sqrtf(psq);
      const float upper = step.agc * maximum(step.pmin, pnorm);
      scale = 1.f / maximum(1.f, unorm / upper);
      scaled = tensor;
    }
    const Span s = span_of(t, offset);
    float usq = 0.f, pnsq = 0.f;
    uint64_t d = 0;
    if constexpr (SLOW) d = slow[tensor];           // `tensor` is the same in every lane
    if (SLOW && d) {
      float* to = reinterpret_cast<float*>(d);
      if (slow_aligned(t, d)) {
        if (t.flags & kOptimBf16) update_chunk<true, true, true>(t, s, scale, step, usq, pnsq, to, mix, omm);
        else update_chunk<false, true, true>(t, s, scale, step, usq, pnsq, to, mix, omm);
      } else {
        if (t.flags & kOptimBf16) update_chunk<true, true, false>(t, s, scale, step, usq, pnsq, to, mix, omm);
        else update_chunk<false, true, false>(t, s, scale, step, usq, pnsq, to, mix, omm);
      }
    } else if (t.flags & kOptimBf16) update_chunk<true>(t, s, scale, step, usq, pnsq);
    else update_chunk<false>(t, s, scale, step, usq, pnsq);
    block_sum2<kThreads>(usq, pnsq, lds);
    if (threadIdx.x == 0) {
      usq_of[chunk] = usq;
      pnsq_of[chunk] = pnsq;
    }
  }
}

// ---- the PPO learner's chain (ppo/agent.py:114-124): clip_by_global_norm,
// scale_by_adam, add_decayed_weights, scale_by_learning_rate, apply_updates.

// One element; `clipped` and `gnorm` are the same in every thread of every
// workgroup.  optax.clip_by_global_norm selects on gnorm < clip, so a NaN norm
// takes the division and reaches every element of every tensor.
__device__ __forceinline__ void adam_one(float g, float& p, float& nu, float& mu, bool clipped, float gnorm, bool decay,
                                         const AdamStep& s, float& usq, float& pnsq) {
  const float g1 = clipped ? (g / gnorm) * s.clip : g;             // optax.clip_by_global_norm
  mu = s.beta1 * mu + s.omb1 * g1;                                 // optax.scale_by_adam: update_moment
  nu = s.beta2 * nu + s.omb2 * (g1 * g1);                          //   update_moment_per_elem_norm
  float u = (mu / s.c1) / (sqrtf(nu / s.c2) + s.eps);              //   bias_correction, eps_root = 0
  if (decay) u = u + s.wd * p;                                     // optax.add_decayed_weights
  const float upd = u * -s.lr;                                     // optax.scale_by_learning_rate
  p = p + upd;                                                     // optax.apply_updates
  usq = usq + upd * upd;
  pnsq = pnsq + p * p;
}

template <bool BF16, bool SLOW = false, bool SLOW_VECTOR = false>
__device__ __forceinline__ void adam_chunk(const OptimTensor& t, const Span& s, bool clipped, float gnorm,
                                           const AdamStep& step, float& usq, float& pnsq, float* d = nullptr,
                                           float mix = 0.f, float omm = 0.f) {
  float* p = reinterpret_cast<float*>(t.p);
  float* nu = reinterpret_cast<float*>(t.nu);
  float* mu = reinterpret_cast<float*>(t.mu);
  const void* g = reinterpret_cast<const void*>(t.g);
  const bool decay = t.flags & kOptimDecay;
  const int tid = threadIdx.x;
  for (int64_t i = static_cast<int64_t>(s.lo) + tid; i < s.first; i += kThreads) {
    float pv = p[i], nv = nu[i], mv = mu[i];
    adam_one(grad_at<BF16>(g, i), pv, nv, mv, clipped, gnorm, decay, step, usq, pnsq);
    p[i] = pv, nu[i] = nv, mu[i] = mv;
    if constexpr (SLOW) d[i] = slow_one(pv, d[i], mix, omm);
  }
#pragma unroll 2
  for (int32_t v = tid; v < s.nvec; v += kThreads) {
    const int32_t i = s.first + 4 * v;
    const float4 gv = grad4_at<BF16>(g, i);
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    float4 nv = *reinterpret_cast<const float4*>(nu + i);
    float4 mv = *reinterpret_cast<const float4*>(mu + i);
    [[maybe_unused]] float4 dv;
    if constexpr (SLOW) dv = slow_load4<SLOW_VECTOR>(d, i);
    adam_one(gv.x, pv.x, nv.x, mv.x, clipped, gnorm, decay, step, usq, pnsq);
    adam_one(gv.y, pv.y, nv.y, mv.y, clipped, gnorm, decay, step, usq, pnsq);
    adam_one(gv.z, pv.z, nv.z, mv.z, clipped, gnorm, decay, step, usq, pnsq);
    adam_one(gv.w, pv.w, nv.w, mv.w, clipped, gnorm, decay, step, usq, pnsq);
    *reinterpret_cast<float4*>(p + i) = pv;
    if constexpr (SLOW) slow_store4<SLOW_VECTOR>(d, i, pv, dv, mix, omm);
    *reinterpret_cast<float4*>(nu + i) = nv;
    *reinterpret_cast<float4*>(mu + i) = mv;
  }
  for (int64_t i = static_cast<int64_t>(s.tail) + tid; i < s.hi; i += kThreads) {
    float pv = p[i], nv = nu[i], mv = mu[i];
    adam_one(grad_at<BF16>(g, i), pv, nv, mv, clipped, gnorm, decay, step, usq, pnsq);
    p[i] = pv, nu[i] = nv, mu[i] = mv;
    if constexpr (SLOW) d[i] = slow_one(pv, d[i], mix, omm);
  }
}

template <bool SLOW>                               // as optim_update_kernel's
__global__ __launch_bounds__(kThreads) void optim_adam_update_kernel(const OptimTensor* __restrict__ table,
                                                                     const OptimChunk* __restrict__ chunks,
                                                                     int32_t n_chunks, float* __restrict__ partials,
                                                                     const AdamStep step,
                                                                     const uint64_t* __restrict__ slow, float mix,
                                                                     float omm) {
  __shared__ float lds[2][kThreads / kWave];
  const float* gsq_of = partials;
  float* usq_of = partials + 2 * static_cast<int64_t>(n_chunks);
  float* pnsq_of = partials + 3 * static_cast<int64_t>(n_chunks);
  // optax.global_norm: every chunk of every tensor, once per workgroup and in the
  // same order in all of them, so all hold the same bits and take the same branch
  float gsq = 0.f, unused = 0.f;
  for (int32_t k = threadIdx.x; k < n_chunks; k += kThreads) gsq = gsq + gsq_of[k];
  block_sum2<kThreads>(gsq, unused, lds);
  const float gnorm = sqrtf(gsq);
  const bool clipped = step.clip != 0.f && !(gnorm < step.clip);
  for (int32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    int32_t tensor, offset;
    const OptimTensor t = tensor_of(table, chunks, chunk, tensor, offset);
    const Span s = span_of(t, offset);
    float usq = 0.f, pnsq = 0.f;
    uint64_t d = 0;
    if constexpr (SLOW) d = slow[tensor];
    if (SLOW && d) {
      float* to = reinterpret_cast<float*>(d);
      if (slow_aligned(t, d)) {
        if (t.flags & kOptimBf16) adam_chunk<true, true, true>(t, s, clipped, gnorm, step, usq, pnsq, to, mix, omm);
        else adam_chunk<false, true, true>(t, s, clipped, gnorm, step, usq, pnsq, to, mix, omm);
      } else {
        if (t.flags & kOptimBf16) adam_chunk<true, true, false>(t, s, clipped, gnorm, step, usq, pnsq, to, mix, omm);
        else adam_chunk<false, true, false>(t, s, clipped, gnorm, step, usq, pnsq, to, mix, omm);
      }
    } else if (t.flags & kOptimBf16) adam_chunk<true>(t, s, clipped, gnorm, step, usq, pnsq);
    else adam_chunk<false>(t, s, clipped, gnorm, step, usq, pnsq);
    block_sum2<kThreads>(usq, pnsq, lds);
    if (threadIdx.x == 0) {
      usq_of[chunk] = usq;
      pnsq_of[chunk] = pnsq;
    }
  }
}

__global__ __launch_bounds__(kMetricThreads) void optim_metrics_kernel(const float* __restrict__ partials,
                                                                       int32_t n_chunks, float count,
                                                                       float* __restrict__ out) {
  __shared__ float lds[2][kMetricThreads / kWave];
  const float* gsq_of = partials;
  const float* usq_of = partials + 2 * static_cast<int64_t>(n_chunks);
  const float* pnsq_of = partials + 3 * static_cast<int64_t>(n_chunks);
  float gsq = 0.f, usq = 0.f, pnsq = 0.f, unused = 0.f;
  for (int32_t k = threadIdx.x; k < n_chunks; k += kMetricThreads) {
    gsq = gsq + gsq_of[k];
    usq = usq + usq_of[k];
    pnsq = pnsq + pnsq_of[k];
  }
  block_sum2<kMetricThreads>(gsq, usq, lds);
  block_sum2<kMetricThreads>(pnsq, unused, lds);
  if (threadIdx.x == 0) {
    out[0] = sqrtf(gsq);                            // opt.py:64, optax.global_norm
    out[1] = sqrtf(gsq / count);                    // opt.py:76, nets.py:120-124
    out[2] = sqrtf(usq / count);                    // opt.py:77
    out[3] = sqrtf(pnsq / count);                   // opt.py:78
  }
}

// ---- the slow copy on its own (utils.py:117-119): dst = mix * src + omm * dst.
// A pure stream, 8 bytes read and 4 written per element; a full chunk is 8 vectors
// per thread, taken two at a time with both pairs of loads ahead of both stores.
__global__ __launch_bounds__(kThreads) void slow_update_kernel(const SlowTensor* __restrict__ table,
                                                               const OptimChunk* __restrict__ chunks, int32_t n_chunks,
                                                               float mix, float omm) {
  const int tid = threadIdx.x;
  for (int32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    int32_t tensor, offset;
    const SlowTensor t = tensor_of(table, chunks, chunk, tensor, offset);
    const Span s = span_of(t, offset);
    float* dst = reinterpret_cast<float*>(t.dst);
    const float* src = reinterpret_cast<const float*>(t.src);
    for (int64_t i = static_cast<int64_t>(s.lo) + tid; i < s.first; i += kThreads)
      dst[i] = slow_one(src[i], dst[i], mix, omm);
    int32_t v = tid;
    for (; v + kThreads < s.nvec; v += 2 * kThreads) {              // both of the pair inside the chunk
      const int32_t i = s.first + 4 * v, j = i + 4 * kThreads;
      const float4 a = *reinterpret_cast<const float4*>(src + i);
      const float4 b = *reinterpret_cast<const float4*>(src + j);
      float4 x = *reinterpret_cast<const float4*>(dst + i);
      float4 y = *reinterpret_cast<const float4*>(dst + j);
      x.x = slow_one(a.x, x.x, mix, omm);
      x.y = slow_one(a.y, x.y, mix, omm);
      x.z = slow_one(a.z, x.z, mix, omm);
      x.w = slow_one(a.w, x.w, mix, omm);
      y.x = slow_one(b.x, y.x, mix, omm);
      y.y = slow_one(b.y, y.y, mix, omm);
      y.z = slow_one(b.z, y.z, mix, omm);
      y.w = slow_one(b.w, y.w, mix, omm);
      *reinterpret_cast<float4*>(dst + i) = x;
      *reinterpret_cast<float4*>(dst + j) = y;
    }
    if (v < s.nvec) {                                                // the one left over
      const int32_t i = s.first + 4 * v;
      const float4 a = *reinterpret_cast<const float4*>(src + i);
      float4 x = *reinterpret_cast<const float4*>(dst + i);
      x.x = slow_one(a.x, x.x, mix, omm);
      x.y = slow_one(a.y, x.y, mix, omm);
      x.z = slow_one(a.z, x.z, mix, omm);
      x.w = slow_one(a.w, x.w, mix, omm);
      *reinterpret_cast<float4*>(dst + i) = x;
    }
    for (int64_t i = static_cast<int64_t>(s.tail) + tid; i < s.hi; i += kThreads)
      dst[i] = slow_one(src[i], dst[i], mix, omm);
  }
}

LaunchCount g_count;

int chunk_blocks(int64_t n_chunks) { return static_cast<int>(n_chunks < kMaxBlocks ? n_chunks : kMaxBlocks); }

}  // namespace

int64_t optim_launches() { return g_count.value(); }

hipError_t launch_optim_norms(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks, float* partials,
                              hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_norms_kernel<true>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table, chunks,
                     static_cast<int32_t>(n_chunks), partials);
  return g_count.launched();
}

hipError_t launch_optim_grad_norms(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                   float* partials, hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_norms_kernel<false>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table, chunks,
                     static_cast<int32_t>(n_chunks), partials);
  return g_count.launched();
}

hipError_t launch_optim_adam_update(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                    float* partials, const AdamStep& step, hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_adam_update_kernel<false>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table,
                     chunks, static_cast<int32_t>(n_chunks), partials, step, static_cast<const uint64_t*>(nullptr), 0.f,
                     0.f);
  return g_count.launched();
}

hipError_t launch_optim_adam_update_slow(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                         float* partials, const AdamStep& step, const uint64_t* slow, float mix,
                                         float omm, hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials || !slow) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_adam_update_kernel<true>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table,
                     chunks, static_cast<int32_t>(n_chunks), partials, step, slow, mix, omm);
  return g_count.launched();
}

hipError_t launch_optim_update(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks, float* partials,
                               const OptimStep& step, hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_update_kernel<false>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table, chunks,
                     static_cast<int32_t>(n_chunks), partials, step, static_cast<const uint64_t*>(nullptr), 0.f, 0.f);
  return g_count.launched();
}

hipError_t launch_optim_update_slow(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                    float* partials, const OptimStep& step, const uint64_t* slow, float mix, float omm,
                                    hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks || !partials || !slow) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_update_kernel<true>, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table, chunks,
                     static_cast<int32_t>(n_chunks), partials, step, slow, mix, omm);
  return g_count.launched();
}

hipError_t launch_slow_update(const SlowTensor* table, const OptimChunk* chunks, int64_t n_chunks, float mix, float omm,
                              hipStream_t stream) {
  if (n_chunks < 1 || n_chunks > INT32_MAX || !table || !chunks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(slow_update_kernel, dim3(chunk_blocks(n_chunks)), dim3(kThreads), 0, stream, table, chunks,
                     static_cast<int32_t>(n_chunks), mix, omm);
  return g_count.launched();
}

hipError_t launch_optim_metrics(const float* partials, int64_t n_chunks, int64_t count, float* out,
                                hipStream_t stream) {
  if (n_chunks < 0 || n_chunks > INT32_MAX || (n_chunks > 0 && !partials) || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_metrics_kernel, dim3(1), dim3(kMetricThreads), 0, stream, partials,
                     static_cast<int32_t>(n_chunks), static_cast<float>(count), out);
  return g_count.launched();
}

}  // namespace emb
