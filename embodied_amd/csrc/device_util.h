// Device helpers shared by the gfx950 (CDNA4, wave64) kernel families of the
// Driver / Replay / return-scan hot path -- movers.hip, step.hip, scans.hip,
// synth_env.hip: what more than one of them uses, nothing else.  Internal
// linkage: every translation unit gets its own copy.
//
// Everything in those files is HBM-bound byte movement or a short recurrence: no MFMA.
// What matters (cdna_hip_programming.md G2, G11, G13): 16-byte accesses per
// lane with consecutive lanes on consecutive addresses, several independent
// loads in flight per lane, and far more than 256 workgroups per launch.
#pragma once

#include "kernels.h"

#include <cstdint>

namespace emb {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // one dwordx4

// Payload pointers that reach a kernel through memory (the indirect-argument
// movers read their KeyDescs with loads) have no known address space, and the
// compiler then emits flat_load / flat_store — slower than global_load /
// global_store and tied to the LDS counter.  Everything the movers touch is
// device global memory: say so.
typedef __attribute__((address_space(1))) u32x4 gu32x4;
template <bool kNonTemporal>
__device__ __forceinline__ u32x4 load16(const u32x4* p) {
  const gu32x4* g = (const gu32x4*)p;
  if constexpr (kNonTemporal) return __builtin_nontemporal_load(g);
  else return *g;
}
template <bool kNonTemporal>
__device__ __forceinline__ void store16(u32x4* p, u32x4 v) {
  gu32x4* g = (gu32x4*)p;
  if constexpr (kNonTemporal) __builtin_nontemporal_store(v, g);
  else *g = v;
}

constexpr int kThreads = 256;

template <typename T>
__device__ __forceinline__ T gload(const void* p) {
  return *(const __attribute__((address_space(1))) T*)p;
}
template <typename T>
__device__ __forceinline__ void gstore(void* p, T v) {
  *(__attribute__((address_space(1))) T*)p = v;
}

template <typename T>
__device__ __forceinline__ void copy_unit(const uint8_t* s, uint8_t* d) {
  gstore<T>(d, gload<T>(s));
}

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void copy_bytes(const uint8_t* s, uint8_t* d, int unit) {
  switch (unit) {
    case 16: copy_unit<u32x4>(s, d); break;
    case 8: copy_unit<u32x2_t>(s, d); break;
    case 4: copy_unit<uint32_t>(s, d); break;
    case 2: copy_unit<uint16_t>(s, d); break;
    default: copy_unit<uint8_t>(s, d); break;
  }
}

// One element of a masked key: value * keep in the key's own dtype — a real
// multiply, so -x -> -0.0 and NaN stays NaN exactly as numpy's
// `value * mask.astype(value.dtype)` (driver.py:84-87) — to the pool row and to
// the masked-action buffer.
template <typename T>
__device__ __forceinline__ T put_masked(const uint8_t* src, uint8_t* pool, uint8_t* out, bool keep) {
  const T v = gload<T>(src) * static_cast<T>(keep ? 1 : 0);
  if (pool) gstore<T>(pool, v);
  if (out) gstore<T>(out, v);
  return v;
}

__device__ __forceinline__ uint16_t put_masked_bf16(const uint8_t* src, uint8_t* pool, uint8_t* out, bool keep) {
  // Widen to f32 (exact), multiply, narrow: the product is x, +-0 or NaN.
  const float x = __uint_as_float(static_cast<uint32_t>(gload<uint16_t>(src)) << 16);
  const uint16_t v = static_cast<uint16_t>(__float_as_uint(x * (keep ? 1.f : 0.f)) >> 16);
  if (pool) gstore<uint16_t>(pool, v);
  if (out) gstore<uint16_t>(out, v);
  return v;
}

// The same by dtype code: THE definition of `value * ~flag` for every launch that
// masks an action (the movers in movers.hip, the publish launch and the carried
// publish in step.hip, a device env's step in synth_env.hip).  Returns the
// product's bits, zero-extended, for a caller that goes on computing with the
// masked value.
template <typename T>
__device__ __forceinline__ uint64_t masked_bits(T v) {
  static_assert(sizeof(T) <= 8, "a masked element fits 64 bits");
  uint64_t bits = 0;
  __builtin_memcpy(&bits, &v, sizeof(T));
  return bits;
}

__device__ __forceinline__ uint64_t put_masked_as(int dtype, const uint8_t* src, uint8_t* pool, uint8_t* out,
                                                  bool keep) {
  switch (dtype) {
    case kU8: case kBool: return masked_bits(put_masked<uint8_t>(src, pool, out, keep));
    case kI8: return masked_bits(put_masked<int8_t>(src, pool, out, keep));
    case kI16: return masked_bits(put_masked<int16_t>(src, pool, out, keep));
    case kI32: return masked_bits(put_masked<int32_t>(src, pool, out, keep));
    case kI64: return masked_bits(put_masked<int64_t>(src, pool, out, keep));
    case kF16: return masked_bits(put_masked<_Float16>(src, pool, out, keep));
    case kBF16: return masked_bits(put_masked_bf16(src, pool, out, keep));
    case kF32: return masked_bits(put_masked<float>(src, pool, out, keep));
    default: return masked_bits(put_masked<double>(src, pool, out, keep));
  }
}

// Bytes of one element of a DType code (host side); 0 for an unknown one.
int dtype_size(int dtype) {
  switch (dtype) {
    case kU8: case kI8: case kBool: return 1;
    case kI16: case kF16: case kBF16: return 2;
    case kI32: case kF32: return 4;
    case kI64: case kF64: return 8;
    default: return 0;
  }
}

}  // namespace
}  // namespace emb
