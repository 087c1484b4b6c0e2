// The optimizer step of the reference's learners (embodied/jax/opt.py:109-164,
// chained by dreamerv3/agent.py:342-379) over any number of parameter tensors in
// two kernel launches: the host-side table builder (plain C++, no HIP: it also
// compiles into a stand-alone host program) and the launchers of optim.hip.
#pragma once

#include <cstdint>

namespace emb {

// Work is cut into chunks of at most kOptimChunk elements of ONE tensor: a chunk
// is what one workgroup reads, and what one partial sum covers.  A multiple of 4,
// so every chunk of a tensor starts at the same address modulo 16 bytes.
constexpr int kOptimChunk = 8192;

enum : int32_t {
  kOptimBf16 = 1,       // the gradient is bfloat16 (else float32); widened in registers
  kOptimDecay = 2,      // weight decay applies to this tensor (agent.py:361-365's mask)
  kOptimVector = 4,     // set by optim_plan: 16-byte accesses from element `head` of every chunk on
};

// One per tensor, read by every workgroup that holds one of its chunks.
struct OptimTensor {
  uint64_t p, g, nu, mu;   // device addresses: parameter, gradient, second and first moment
  int32_t n;               // elements, 0 .. 2^31 - 1
  int32_t first_chunk;     // index of the tensor's first chunk = of its first partial sum
  int32_t flags;           // kOptim*
  int32_t head;            // 0 .. 3 scalar elements in front of a chunk's first aligned vector
};
static_assert(sizeof(OptimTensor) == 48, "the table is read as 48-byte records");

struct OptimChunk {
  int32_t tensor;          // index into the table
  int32_t offset;          // first element, a multiple of kOptimChunk
};
static_assert(sizeof(OptimChunk) == 8, "the chunk map is read as 8-byte records");

inline int64_t optim_chunks_of(int64_t n) { return (n + kOptimChunk - 1) / kOptimChunk; }

// addrs (tensors, 4) = p, g, nu, mu of every tensor; counts (tensors); flags
// (tensors) of kOptimBf16 | kOptimDecay.  Writes the number of chunks, and, where
// given, the table (tensors records) and the chunk map (as many records as there
// are chunks; `chunk_capacity` is what `chunks` holds).  A tensor of 0 elements has
// a record and no chunk.  Returns null, or what is wrong: nothing is written past
// what was asked for, and nothing at all once something is wrong with the sizes.
//
// A tensor takes the vector path when, from the first 16-byte boundary of p on,
// nu, mu and g are aligned too (g: 16 bytes as float32, 8 as bfloat16), which is
// the case whenever the four are views at the same element offset modulo 4 --
// flat buffers cut the same way.  Otherwise every access of that tensor is scalar.
inline const char* optim_plan(const int64_t* addrs, const int64_t* counts, const int32_t* flags, int64_t tensors,
                              OptimTensor* table, OptimChunk* chunks, int64_t chunk_capacity, int64_t* n_chunks) {
  if (tensors < 0 || tensors > INT32_MAX) return "optim_table: the number of tensors is outside 0 .. 2^31 - 1";
  if (tensors > 0 && (!addrs || !counts || !flags)) return "optim_table: a pointer is null";
  int64_t total = 0;
  for (int64_t i = 0; i < tensors; ++i) {
    if (counts[i] < 0 || counts[i] > INT32_MAX) return "optim_table: a tensor of more than 2^31 - 1 elements";
    if (flags[i] & ~(kOptimBf16 | kOptimDecay)) return "optim_table: unknown flags";
    const uint64_t gsize = flags[i] & kOptimBf16 ? 2 : 4;
    const int64_t* a = addrs + 4 * i;
    if (counts[i] > 0) {
      if (!a[0] || !a[1] || !a[2] || !a[3]) return "optim_table: a null address";
      if ((a[0] | a[2] | a[3]) & 3 || static_cast<uint64_t>(a[1]) & (gsize - 1))
        return "optim_table: an address that is not aligned to its element";
    }
    total += optim_chunks_of(counts[i]);
  }
  if (total > INT32_MAX) return "optim_table: more than 2^31 - 1 chunks";
  if (chunks && chunk_capacity < total) return "optim_table: the chunk map is too small";
  if (n_chunks) *n_chunks = total;
  int64_t next = 0;
  for (int64_t i = 0; i < tensors; ++i) {
    const int64_t* a = addrs + 4 * i;
    const int64_t n = counts[i];
    if (table) {
      OptimTensor t{};
      t.p = static_cast<uint64_t>(a[0]);
      t.g = static_cast<uint64_t>(a[1]);
      t.nu = static_cast<uint64_t>(a[2]);
      t.mu = static_cast<uint64_t>(a[3]);
      t.n = static_cast<int32_t>(n);
      t.first_chunk = static_cast<int32_t>(next);
      t.flags = flags[i];
      if (n > 0) {
        const uint64_t head = ((16 - (t.p & 15)) & 15) / 4;
        const uint64_t gsize = flags[i] & kOptimBf16 ? 2 : 4;
        const bool aligned = ((t.nu + 4 * head) & 15) == 0 && ((t.mu + 4 * head) & 15) == 0 &&
                             ((t.g + gsize * head) & (4 * gsize - 1)) == 0;
        if (aligned) {
          t.flags |= kOptimVector;
          t.head = static_cast<int32_t>(head);
        }
      }
      table[i] = t;
    }
    for (int64_t off = 0; off < n; off += kOptimChunk, ++next) {
      if (chunks) {
        chunks[next].tensor = static_cast<int32_t>(i);
        chunks[next].offset = static_cast<int32_t>(off);
      }
    }
  }
  return nullptr;
}

// ---- the slow (EMA) copy of a set of tensors, embodied/jax/utils.py:94-127:
// dst = mix * src + (1 - mix) * dst over every tensor in one launch, on the same
// kind of chunk map.

// One per tensor, read by every workgroup that holds one of its chunks.
struct SlowTensor {
  uint64_t dst, src;       // device addresses, float32: the slow copy and what it follows
  int32_t n;               // elements, 0 .. 2^31 - 1
  int32_t first_chunk;     // index of the tensor's first chunk
  int32_t flags;           // kOptimVector or 0
  int32_t head;            // 0 .. 3 scalar elements in front of a chunk's first aligned vector
};
static_assert(sizeof(SlowTensor) == 32, "the table is read as 32-byte records");

// addrs (tensors, 2) = dst, src of every tensor; counts (tensors).  The
// conventions of optim_plan: writes the number of chunks and, where given, the
// table and the chunk map; a tensor of 0 elements has a record and no chunk;
// returns null, or what is wrong, and then has written nothing.
//
// A tensor takes the vector path when, from the first 16-byte boundary of dst
// on, src is aligned too; otherwise every access of that tensor is scalar.
inline const char* slow_plan(const int64_t* addrs, const int64_t* counts, int64_t tensors, SlowTensor* table,
                             OptimChunk* chunks, int64_t chunk_capacity, int64_t* n_chunks) {
  if (tensors < 0 || tensors > INT32_MAX) return "slow_table: the number of tensors is outside 0 .. 2^31 - 1";
  if (tensors > 0 && (!addrs || !counts)) return "slow_table: a pointer is null";
  int64_t total = 0;
  for (int64_t i = 0; i < tensors; ++i) {
    if (counts[i] < 0 || counts[i] > INT32_MAX) return "slow_table: a tensor of more than 2^31 - 1 elements";
    const int64_t* a = addrs + 2 * i;
    if (counts[i] > 0) {
      if (!a[0] || !a[1]) return "slow_table: a null address";
      if ((a[0] | a[1]) & 3) return "slow_table: an address that is not aligned to its element";
      if (a[0] == a[1]) return "slow_table: dst and src are the same tensor";
    }
    total += optim_chunks_of(counts[i]);
  }
  if (total > INT32_MAX) return "slow_table: more than 2^31 - 1 chunks";
  if (chunks && chunk_capacity < total) return "slow_table: the chunk map is too small";
  if (n_chunks) *n_chunks = total;
  int64_t next = 0;
  for (int64_t i = 0; i < tensors; ++i) {
    const int64_t* a = addrs + 2 * i;
    const int64_t n = counts[i];
    if (table) {
      SlowTensor t{};
      t.dst = static_cast<uint64_t>(a[0]);
      t.src = static_cast<uint64_t>(a[1]);
      t.n = static_cast<int32_t>(n);
      t.first_chunk = static_cast<int32_t>(next);
      if (n > 0) {
        const uint64_t head = ((16 - (t.dst & 15)) & 15) / 4;
        if (((t.src + 4 * head) & 15) == 0) {
          t.flags = kOptimVector;
          t.head = static_cast<int32_t>(head);
        }
      }
      table[i] = t;
    }
    for (int64_t off = 0; off < n; off += kOptimChunk, ++next) {
      if (chunks) {
        chunks[next].tensor = static_cast<int32_t>(i);
        chunks[next].offset = static_cast<int32_t>(off);
      }
    }
  }
  return nullptr;
}

}  // namespace emb

#ifndef EMB_OPTIM_HOST_ONLY
#include <hip/hip_runtime.h>

namespace emb {

// What one update needs besides the tables, all of it kernel arguments.  The
// host forms, in double and rounded once (as a Python scalar meets a float32
// array): omb = 1 - beta, c = 1 - beta ** t with t the update counted from 1, and
// lr = the schedule at t - 1.
struct OptimStep {
  float lr, beta1, omb1, c1, beta2, omb2, c2, eps, agc, pmin, wd;
  int32_t nesterov;
};

// The scalars of one update of the PPO learner's chain (ppo/agent.py:114-124:
// clip_by_global_norm, scale_by_adam, add_decayed_weights, scale_by_learning_rate),
// formed on the host as OptimStep's.  clip == 0: no clipping.
struct AdamStep {
  float lr, beta1, omb1, c1, beta2, omb2, c2, eps, clip, wd;
};

// partials is (4, n_chunks) float32: per chunk sum g^2 and sum p^2 (written by the
// norms launch), sum upd^2 and sum p_new^2 (written by the update launch).
// Launch 1: every chunk's sum g^2 and sum p^2 (opt.py:116-117's norms, and
// optax.global_norm of opt.py:64).
hipError_t launch_optim_norms(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks, float* partials,
                              hipStream_t stream);
// Launch 2: each workgroup sums its tensor's partials in a fixed order, forms the
// AGC scale (opt.py:118-119) and updates its chunk (opt.py:136-140, 156-161,
// agent.py:361-378, optax.apply_updates).
hipError_t launch_optim_update(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks, float* partials,
                               const OptimStep& step, hipStream_t stream);
// Launch 1 of the Adam chain: every chunk's sum g^2 into row 0 of `partials`; the
// parameters are not read and row 1 is not written.
hipError_t launch_optim_grad_norms(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                   float* partials, hipStream_t stream);
// Launch 2 of the Adam chain: every workgroup sums row 0 of ALL chunks in one
// fixed order (optax.global_norm), takes the clip decision and updates its chunks
// (optax.clip_by_global_norm, scale_by_adam, add_decayed_weights,
// scale_by_learning_rate, apply_updates); leaves rows 2 and 3 as launch_optim_update.
hipError_t launch_optim_adam_update(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                    float* partials, const AdamStep& step, hipStream_t stream);
// out (4,) float32: grad_norm, grad_rms, update_rms, param_rms (opt.py:64, 75-78,
// nets.py:120-124) from the partials, one workgroup, a fixed order.
hipError_t launch_optim_metrics(const float* partials, int64_t n_chunks, int64_t count, float* out, hipStream_t stream);

// dst = mix * src + omm * dst over every tensor of a slow_plan table, one launch
// (utils.py:117-119); two rounded products and one rounded sum per element.
hipError_t launch_slow_update(const SlowTensor* table, const OptimChunk* chunks, int64_t n_chunks, float mix, float omm,
                              hipStream_t stream);
// launch_optim_update / launch_optim_adam_update that also write the slow copy
// while p_new is in registers: `slow` holds one device address per table entry,
// 0 where a tensor has none; d = mix * p_new + omm * d at the same element index.
hipError_t launch_optim_update_slow(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                    float* partials, const OptimStep& step, const uint64_t* slow, float mix, float omm,
                                    hipStream_t stream);
hipError_t launch_optim_adam_update_slow(const OptimTensor* table, const OptimChunk* chunks, int64_t n_chunks,
                                         float* partials, const AdamStep& step, const uint64_t* slow, float mix,
                                         float omm, hipStream_t stream);

// Kernel launches the launchers above have issued in this process.
int64_t optim_launches();

}  // namespace emb
#endif  // EMB_OPTIM_HOST_ONLY
