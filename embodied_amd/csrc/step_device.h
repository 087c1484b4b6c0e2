// Device code that the Driver-step kernels (step.hip) and the device env's fused
// step (synth_env.hip) share: the per-channel cast of the policy batch, its
// streaming stores, and the narrow workgroup of the early insert with the
// table it reads.  One definition: both families must store the same bytes.
#pragma once

#include "device_util.h"
#include "kernels.h"

#include <cstddef>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace emb {

// ---------------------------------------------------------------- obs stack --

template <typename Out>
__device__ __forceinline__ Out cvt(uint8_t v, float scale, float offset);
template <> __device__ __forceinline__ uint8_t cvt<uint8_t>(uint8_t v, float, float) { return v; }
template <> __device__ __forceinline__ float cvt<float>(uint8_t v, float s, float o) { return fmaf(static_cast<float>(v), s, o); }
template <> __device__ __forceinline__ __half cvt<__half>(uint8_t v, float s, float o) { return __float2half(fmaf(static_cast<float>(v), s, o)); }
template <> __device__ __forceinline__ __hip_bfloat16 cvt<__hip_bfloat16>(uint8_t v, float s, float o) { return __float2bfloat16(fmaf(static_cast<float>(v), s, o)); }

template <typename Out>
struct alignas(4 * sizeof(Out)) Quad { Out v[4]; };

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Streaming store of one Quad (4, 8 or 16 bytes): the policy batch is consumed
// by another kernel, keeping it dirty in this XCD's L2 only delays the next
// kernel boundary.
template <typename Out>
__device__ __forceinline__ void store_quad(Out* dst, const Quad<Out>& q) {
  if constexpr (sizeof(Quad<Out>) == 4) {
    uint32_t w;
    __builtin_memcpy(&w, &q, 4);
    __builtin_nontemporal_store(w, reinterpret_cast<uint32_t*>(dst));
  } else if constexpr (sizeof(Quad<Out>) == 8) {
    u32x2 w;
    __builtin_memcpy(&w, &q, 8);
    __builtin_nontemporal_store(w, reinterpret_cast<u32x2*>(dst));
  } else {
    u32x4 w;
    __builtin_memcpy(&w, &q, 16);
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(dst));
  }
}

// The policy-batch stores of quad `q` (4 pixels x C channels, the bytes in `w`)
// of one frame: per channel one 4-element vector, (C, P) channels-first or
// (P, C) as stored.
template <typename Out, int C, bool kChannelsFirst>
__device__ __forceinline__ void store_policy_quad(Out* out, const uint32_t (&w)[C], int64_t pixels, int64_t q,
                                                  float scale, float offset) {
  auto byte_at = [&w](int idx) {
    return static_cast<uint8_t>((w[idx >> 2] >> ((idx & 3) * 8)) & 0xFFu);
  };
  if (kChannelsFirst) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      Quad<Out> o;
#pragma unroll
      for (int p = 0; p < 4; ++p) o.v[p] = cvt<Out>(byte_at(p * C + c), scale, offset);
      store_quad(out + c * pixels + q * 4, o);
    }
  } else {
#pragma unroll
    for (int j = 0; j < C; ++j) {
      Quad<Out> o;
#pragma unroll
      for (int p = 0; p < 4; ++p) o.v[p] = cvt<Out>(byte_at(j * 4 + p), scale, offset);
      store_quad(out + (q * C + j) * 4, o);
    }
  }
}

// ------------------------------------------------- the early insert's table --

struct PreKey {
  const uint8_t* src;
  uint8_t* pool;
  int64_t rowbytes;
};
// The action of the PREVIOUS step, carried into this launch (see "carried
// publish" in step.hip): value * !flags[e] in `dtype` to row prev_rows[e] of `pool`.
struct PreCarry {
  const uint8_t* src;           // (n, rowbytes); null = nothing carried
  uint8_t* pool;
  const uint8_t* flags;         // the replay's is_last POOL (1-byte rows): the carried step's flag is at its own row
  int32_t rowbytes, dtype, elem, pad;
};
struct alignas(16) PreTable {
  uint8_t* stepid_pool;
  int32_t* rows_out;            // device int32[n]: the rows again, for the publish launch (may be null)
  PreKey narrow[kPreNarrow];
  PreCarry carry;
  uint32_t words[1];            // rows[n] | step ids, 5 words per row | the carried step's rows[n] (7 * n words)
};

// (prewrite_fill_table, step.hip, writes this layout; synth_env_fused_kernel finds
// it 96 bytes into its block.)
static_assert(offsetof(PreTable, narrow) == 16, "stepid_pool, rows_out, then the narrow keys");
static_assert(offsetof(PreTable, carry) == 208, "8 narrow keys of 24 bytes");
static_assert(offsetof(PreTable, words) == 248, "the carry's 40 bytes, then rows | step ids | carried rows");

// The narrow keys, the step id and the row for the publish launch of env n: one
// extra workgroup per env (the first n of the grid), so that this chain of
// dependent reads (table -> source bytes -> stores) runs beside the frame
// workgroups instead of behind one of them.  All loads are issued before the
// first store: three memory round trips, however many keys.
//
// Carried publish: when all that an insert has left after the policy is one
// small masked key (the action) and nobody needs the masked values back, the
// publish launch is not made at all -- the previous step's action rides in THIS
// launch (one element per lane of the env's narrow workgroup, the same typed
// multiply as publish_one_kernel), one dependent launch less per env step.
__device__ __forceinline__ void prewrite_carry(const PreTable& t, const uint32_t* tab, int32_t n_envs,
                                               int64_t n) {
  const PreCarry c = t.carry;                    // uniform: scalar loads
  if (!c.src) return;
  const int64_t prev = static_cast<int32_t>(gload<uint32_t>(tab + 6 * static_cast<int64_t>(n_envs) + n));
  const int64_t off = static_cast<int64_t>(threadIdx.x) * c.elem;
  if (prev < 0 || off >= c.rowbytes) return;
  // The carried step's is_last as the replay stored it (written by that step's
  // own early-insert launch, earlier on this stream) -- not the env's output
  // buffer, which an env with one output set has overwritten by now.
  const bool keep = gload<uint8_t>(c.flags + prev) == 0;
  const uint8_t* src = c.src + n * c.rowbytes + off;
  uint8_t* pool = c.pool + prev * c.rowbytes + off;
  put_masked_as(c.dtype, src, pool, nullptr, keep);
}

// `value(key)`: byte `threadIdx.x` of env n's row of a narrow key -- a load from
// the key's source (step.hip), or a register of the launch that has just
// computed the row (synth_env.hip).
template <typename Value>
__device__ __forceinline__ void prewrite_narrow(const PreTable& t, int32_t n_envs, int32_t n_narrow, int64_t n,
                                                Value value) {
  const uint32_t* tab = t.words;
  prewrite_carry(t, tab, n_envs, n);
  const int64_t row = static_cast<int32_t>(gload<uint32_t>(tab + n));
  if (row < 0) return;
  uint32_t sid = 0;
  if (threadIdx.x < kStepBytes / 4)
    sid = gload<uint32_t>(tab + n_envs + n * (kStepBytes / 4) + threadIdx.x);
  PreKey key[kPreNarrow];
#pragma unroll
  for (int k = 0; k < kPreNarrow; ++k) key[k] = t.narrow[k];      // uniform: scalar loads
  uint8_t v[kPreNarrow];
#pragma unroll
  for (int k = 0; k < kPreNarrow; ++k) {
    v[k] = 0;
    if (k < n_narrow && static_cast<int64_t>(threadIdx.x) < key[k].rowbytes) v[k] = value(key[k]);
  }
#pragma unroll
  for (int k = 0; k < kPreNarrow; ++k)
    if (k < n_narrow && static_cast<int64_t>(threadIdx.x) < key[k].rowbytes)
      gstore<uint8_t>(key[k].pool + row * key[k].rowbytes + threadIdx.x, v[k]);
  if (t.stepid_pool && threadIdx.x < kStepBytes / 4)
    gstore<uint32_t>(t.stepid_pool + row * kStepBytes + threadIdx.x * 4, sid);
  if (t.rows_out && threadIdx.x == 0) t.rows_out[n] = static_cast<int32_t>(row);
}
static_assert(kThreads >= 256, "a narrow key (<= 256 bytes per step) is one byte per lane");

}  // namespace emb
