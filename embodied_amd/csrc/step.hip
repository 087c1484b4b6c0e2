// Driver step: obs stack (+ early insert into the replay), publish of the action,
// action mask, windowing and the byte copy.
#include "device_util.h"
#include "step_device.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace emb {
namespace {

// ---------------------------------------------------------------- obs stack --

// Each lane owns 4 consecutive pixels of one frame: it reads their 4*C bytes as
// C dwords (coalesced across lanes) and writes, per channel, one 4-element
// vector.  Output is (N, C, P) channels-first or (N, P, C) as stored.
template <typename Out, int C, bool kChannelsFirst>
__global__ __launch_bounds__(kThreads) void obs_stack_kernel(
    const uint8_t* src, const int32_t* env_ids, Out* dst, int64_t pixels,
    float scale, float offset) {
  const int64_t n = blockIdx.y;
  const int64_t e = env_ids ? env_ids[n] : n;
  const int64_t quads = pixels >> 2;
  const uint32_t* frame = reinterpret_cast<const uint32_t*>(src + e * pixels * C);
  Out* out = dst + n * pixels * C;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; q < quads;
       q += static_cast<int64_t>(gridDim.x) * kThreads) {
    uint32_t w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = frame[q * C + c];
    store_policy_quad<Out, C, kChannelsFirst>(out, w, pixels, q, scale, offset);
  }
}

// Any channel count / pixel tail: one element per lane.
template <typename Out>
__global__ __launch_bounds__(kThreads) void obs_stack_generic_kernel(
    const uint8_t* src, const int32_t* env_ids, Out* dst, int64_t pixels,
    int64_t channels, int layout, float scale, float offset) {
  const int64_t n = blockIdx.y;
  const int64_t e = env_ids ? env_ids[n] : n;
  const int64_t elems = pixels * channels;
  const uint8_t* frame = src + e * elems;
  Out* out = dst + n * elems;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < elems;
       i += static_cast<int64_t>(gridDim.x) * kThreads) {
    int64_t s = i;
    if (layout == kLayoutChannelsFirst) {
      const int64_t c = i / pixels, p = i - c * pixels;
      s = p * channels + c;
    }
    out[i] = cvt<Out>(frame[s], scale, offset);
  }
}

template <typename Out>
hipError_t obs_stack_typed(const uint8_t* src, const int32_t* env_ids, void* dst,
                           int64_t n, int64_t pixels, int64_t channels, int layout,
                           float scale, float offset, hipStream_t stream) {
  Out* out = static_cast<Out*>(dst);
  const bool fast = pixels % 4 == 0 && channels >= 1 && channels <= 4 &&
                    reinterpret_cast<uint64_t>(src) % 4 == 0 &&
                    (pixels * channels) % 4 == 0 &&
                    reinterpret_cast<uint64_t>(dst) % (4 * sizeof(Out)) == 0;
  if (!fast) {
    const int64_t elems = pixels * channels;
    dim3 grid(static_cast<uint32_t>(std::min<int64_t>((elems + kThreads - 1) / kThreads, 64)),
              static_cast<uint32_t>(n));
    hipLaunchKernelGGL(obs_stack_generic_kernel<Out>, grid, dim3(kThreads), 0, stream,
                       src, env_ids, out, pixels, channels, layout, scale, offset);
    return hipGetLastError();
  }
  const int64_t quads = pixels / 4;
  dim3 grid(static_cast<uint32_t>(std::min<int64_t>((quads + kThreads - 1) / kThreads, 32)),
            static_cast<uint32_t>(n));
  const bool cf = layout == kLayoutChannelsFirst && channels > 1;
#define EMB_OBS(C)                                                                         \
  if (cf) hipLaunchKernelGGL((obs_stack_kernel<Out, C, true>), grid, dim3(kThreads), 0,   \
                             stream, src, env_ids, out, pixels, scale, offset);           \
  else hipLaunchKernelGGL((obs_stack_kernel<Out, C, false>), grid, dim3(kThreads), 0,     \
                          stream, src, env_ids, out, pixels, scale, offset);
  switch (channels) {
    case 1: EMB_OBS(1) break;
    case 2: EMB_OBS(2) break;
    case 3: EMB_OBS(3) break;
    default: EMB_OBS(4) break;
  }
#undef EMB_OBS
  return hipGetLastError();
}

// ------------------------------------------------- obs stack + early insert --
//
// The frames of a vectorised step are needed twice: by the policy (cast /
// transposed into its batch) and by the replay (copied into the pool rows the
// step will occupy).  Those rows are known before the policy runs — a worker's
// next row is its open chunk's cursor (replay_index.h peek) — so ONE launch
// reads every frame once and writes both: the policy batch exactly as
// obs_stack_kernel does, and the same 16 bytes per lane into the reserved pool
// row.  The other observation keys (reward, flags: a few bytes per env) and the
// step ids ride along in the workgroup that owns the frame's tail.  What is
// left for after the policy is the action (publish_one_kernel).
//
// Arguments: 64 bytes, all of them inside the kernel-argument preload (they
// arrive in SGPRs with the wave).  Everything per-env — the row table, the step
// ids, the narrow keys' descriptors — sits in a block in DEVICE memory that the
// host wrote through the BAR (abi.cpp ArgRing) or uploaded: with host-resident
// kernel arguments every wave's read of a by-value table would be a PCIe round
// trip of its own (1 800 waves: measured 11.5 us for this launch instead of 5).
// The row of a frame is read while the frame's loads are in flight (the
// policy-batch stores do not depend on it).
struct PrewriteArgs {
  const uint8_t* frames;
  void* dst;
  uint8_t* frame_pool;
  int32_t pixels, frame_blocks;
  float scale, offset;
  int32_t n, n_narrow;
  const PreTable* table;        // device memory
};
static_assert(sizeof(PrewriteArgs) == 56, "obs_stack_insert_kernel's arguments (passed one by one) fit the 14 preloaded dwords");

// (Scalar parameters, not the struct: the kernel-argument preload only takes
// arguments passed as scalars / pointers -- a by-value struct is fetched with
// s_load by every wave, `.amdhsa_user_sgpr_kernarg_preload_length 0`.)
template <typename Out, int C, bool kChannelsFirst>
// (The preload covers 14 dwords = 56 bytes: exactly these.)
// ONE-dimensional grid: workgroups [0, n) are the narrow ones (their chain is the
// longest: first out), [n, n + n * frame_blocks) the frame blocks, env by env.
// The hardware hands consecutive workgroup ids to the 8 XCDs in turn: as a
// (frame_blocks + 1, n) grid with 7 + 1 blocks per env (84 x 84 x 4) every
// narrow workgroup landed on one XCD, which then took no frame block at all
// (tools/insert_lab.hip: 0.24 us of the launch).
__global__ __launch_bounds__(kThreads) void obs_stack_insert_kernel(
    const uint8_t* frames, const PreTable* table, uint8_t* frame_pool, void* dst,
    int32_t pixels_, int32_t frame_blocks, int32_t n_envs, int32_t n_narrow, float scale, float offset) {
  const PrewriteArgs a{frames, dst, frame_pool, pixels_, frame_blocks, scale, offset, n_envs, n_narrow, table};
  if (blockIdx.x < static_cast<uint32_t>(n_envs)) {
    // (cvt, store_quad, the table and prewrite_narrow: step_device.h)
    const int64_t n = blockIdx.x;
    prewrite_narrow(*a.table, a.n, a.n_narrow, n, [n](const PreKey& key) {
      return gload<uint8_t>(key.src + n * key.rowbytes + threadIdx.x);
    });
    return;
  }
  const uint32_t id = blockIdx.x - static_cast<uint32_t>(n_envs);
  const int64_t n = id / static_cast<uint32_t>(frame_blocks);
  const uint32_t block = id - static_cast<uint32_t>(n) * static_cast<uint32_t>(frame_blocks);
  const int64_t pixels = a.pixels;
  const int64_t quads = pixels >> 2;
  const uint32_t* frame = reinterpret_cast<const uint32_t*>(a.frames + n * pixels * C);
  Out* out = static_cast<Out*>(a.dst) + n * pixels * C;
  const int64_t row = static_cast<int32_t>(gload<uint32_t>(a.table->words + n));
  uint32_t* pool = reinterpret_cast<uint32_t*>(a.frame_pool + row * pixels * C);
  const int64_t stride = static_cast<int64_t>(frame_blocks) * kThreads;
  for (int64_t q = static_cast<int64_t>(block) * kThreads + threadIdx.x; q < quads; q += stride) {
    uint32_t w[C];
    if constexpr (C == 4) {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(frame) + q);
      w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) w[c] = frame[q * C + c];
    }
    store_policy_quad<Out, C, kChannelsFirst>(out, w, pixels, q, a.scale, a.offset);
    if (row >= 0) {
      if constexpr (C == 4) {
        __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4*>(pool) + q);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) __builtin_nontemporal_store(w[c], pool + q * C + c);
      }
    }
  }
}

template <typename Out>
hipError_t obs_stack_insert_typed(const PrewriteArgs& a, int64_t channels, int layout,
                                  hipStream_t stream, hipEvent_t stop) {
  // one workgroup per env for the narrow keys + frame_blocks per env for its frames
  dim3 grid(static_cast<uint32_t>(a.n) * static_cast<uint32_t>(a.frame_blocks + 1));
  const bool cf = layout == kLayoutChannelsFirst && channels > 1;
  // (hipExtLaunchKernelGGL only when a completion stamp is wanted: the plain
  // launch is the cheaper call.)
#define EMB_PRE_ARGS a.frames, a.table, a.frame_pool, a.dst, a.pixels, a.frame_blocks, a.n, a.n_narrow, a.scale, a.offset
#define EMB_PRE(C)                                                                                \
  if (cf && stop) hipExtLaunchKernelGGL((obs_stack_insert_kernel<Out, C, true>), grid,            \
                                        dim3(kThreads), 0, stream, nullptr, stop, 0, EMB_PRE_ARGS); \
  else if (cf) hipLaunchKernelGGL((obs_stack_insert_kernel<Out, C, true>), grid, dim3(kThreads),  \
                                  0, stream, EMB_PRE_ARGS);                                       \
  else if (stop) hipExtLaunchKernelGGL((obs_stack_insert_kernel<Out, C, false>), grid,            \
                                       dim3(kThreads), 0, stream, nullptr, stop, 0, EMB_PRE_ARGS); \
  else hipLaunchKernelGGL((obs_stack_insert_kernel<Out, C, false>), grid, dim3(kThreads), 0,      \
                          stream, EMB_PRE_ARGS);
  switch (channels) {
    case 1: EMB_PRE(1) break;
    case 2: EMB_PRE(2) break;
    case 3: EMB_PRE(3) break;
    default: EMB_PRE(4) break;
  }
#undef EMB_PRE
#undef EMB_PRE_ARGS
  return hipGetLastError();
}

// What is left of an insert after obs_stack_insert_kernel when the only other
// key is the action: rows[r] comes from the table that launch left in device
// memory, the value is written as src * !flags[r] (driver.py:72-74; a real
// multiply in the key's dtype) to its pool row and to `out`, the actions the
// next env step receives.  56 bytes of arguments, passed one by one: exactly
// the 14 dwords the kernel-argument preload covers.
struct PublishArgs {
  const uint8_t* src;
  uint8_t* pool;
  uint8_t* out;
  const int32_t* rows;
  const uint8_t* flags;      // null: plain copy
  int32_t n, rowbytes, dtype, elem;
};
static_assert(sizeof(PublishArgs) <= 64, "publish_one_kernel's arguments are preloaded");

__global__ __launch_bounds__(kThreads) void publish_one_kernel(
    const uint8_t* src_, uint8_t* pool_, uint8_t* out_, const int32_t* rows, const uint8_t* flags,
    int32_t n, int32_t rowbytes, int32_t dtype, int32_t elem) {
  const PublishArgs a{src_, pool_, out_, rows, flags, n, rowbytes, dtype, elem};
  const int64_t epr = a.rowbytes / a.elem;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= epr * a.n) return;
  const int64_t r = e / epr;
  const int64_t off = (e - r * epr) * a.elem;
  const int64_t row = a.rows[r];
  // dtype bit 8: `flags` is a pool of 1-byte rows, the flag of batch row r sits
  // at its pool row (a carried publish settled late, abi.cpp settle_carry).
  const bool by_row = (a.dtype & 0x100) != 0;
  const bool keep = !a.flags || (by_row ? row < 0 || gload<uint8_t>(a.flags + row) == 0
                                        : gload<uint8_t>(a.flags + r) == 0);
  const uint8_t* src = a.src + r * a.rowbytes + off;
  uint8_t* pool = row >= 0 ? a.pool + row * a.rowbytes + off : nullptr;
  uint8_t* out = a.out ? a.out + r * a.rowbytes + off : nullptr;
  put_masked_as(a.dtype & 0xFF, src, pool, out, keep);
}

// ------------------------------------------------------------- action mask --

// `flag` (optional): a word in pinned host memory that receives `seq` when every
// workgroup of the launch has stored its part -- with `out` in pinned memory too
// (the Driver bringing the next step's actions down to its env processes) the host
// sees the rows complete by reading one word, without an event.  `counter`: a
// zeroed device word of the caller's, left zeroed again.
__device__ __forceinline__ void notify_host(uint32_t* counter, uint32_t* flag, uint32_t seq) {
  if (!flag) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t seen = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (seen + 1 == gridDim.x) {
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mask_rows_kernel(
    const T* act, T* out, int64_t n, int64_t row_elems, const uint8_t* is_last, uint32_t* counter,
    uint32_t* flag, uint32_t seq) {
  const int64_t total = n * row_elems;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t r = i / row_elems;
    // value * mask.astype(value.dtype): a real multiply, so -x -> -0.0 and
    // NaN stays NaN exactly as numpy does (driver.py:84-87).
    out[i] = act[i] * static_cast<T>(is_last[r] ? 0 : 1);
  }
  notify_host(counter, flag, seq);
}

// bf16 has no native multiply: widen to f32 (exact), multiply, narrow (the
// product is x, +-0 or NaN, all exactly representable).
template <>
__global__ __launch_bounds__(kThreads) void mask_rows_kernel<__hip_bfloat16>(
    const __hip_bfloat16* act, __hip_bfloat16* out, int64_t n, int64_t row_elems,
    const uint8_t* is_last, uint32_t* counter, uint32_t* flag, uint32_t seq) {
  const int64_t total = n * row_elems;
  const uint16_t* bits = reinterpret_cast<const uint16_t*>(act);
  uint16_t* obits = reinterpret_cast<uint16_t*>(out);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * kThreads) {
    const float x = __uint_as_float(static_cast<uint32_t>(bits[i]) << 16);
    const float y = x * (is_last[i / row_elems] ? 0.f : 1.f);
    obits[i] = static_cast<uint16_t>(__float_as_uint(y) >> 16);
  }
  notify_host(counter, flag, seq);
}

// ---------------------------------------------------------------- windowing --

__global__ __launch_bounds__(kThreads) void window_kernel(
    const uint8_t* src, uint8_t* dst, int64_t total, int64_t start, int64_t count,
    int64_t rowbytes, int unit, int64_t units_per_seq) {
  const int64_t b = blockIdx.y;
  const uint8_t* s = src + (b * total + start) * rowbytes;
  uint8_t* d = dst + b * count * rowbytes;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
       u < units_per_seq; u += static_cast<int64_t>(gridDim.x) * kThreads)
    copy_bytes(s + u * unit, d + u * unit, unit);
}

// Bytes of any alignment from `src` to `dst`: 16-byte units when both allow it, a
// byte tail.  `src` may be pinned host memory the GPU reads across PCIe (a piece
// of the Driver's shared observation slab): four units per lane in flight.
__global__ __launch_bounds__(kThreads) void copy_bytes_kernel(const uint8_t* __restrict__ src,
                                                             uint8_t* __restrict__ dst, int64_t bytes) {
  const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int64_t vecs = aligned ? bytes >> 4 : 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  for (; i + 3 * stride < vecs; i += 4 * stride) {
    const u32x4 a = reinterpret_cast<const u32x4*>(src)[i], b = reinterpret_cast<const u32x4*>(src)[i + stride];
    const u32x4 c = reinterpret_cast<const u32x4*>(src)[i + 2 * stride], d = reinterpret_cast<const u32x4*>(src)[i + 3 * stride];
    reinterpret_cast<u32x4*>(dst)[i] = a;
    reinterpret_cast<u32x4*>(dst)[i + stride] = b;
    reinterpret_cast<u32x4*>(dst)[i + 2 * stride] = c;
    reinterpret_cast<u32x4*>(dst)[i + 3 * stride] = d;
  }
  for (; i < vecs; i += stride) reinterpret_cast<u32x4*>(dst)[i] = reinterpret_cast<const u32x4*>(src)[i];
  for (int64_t j = (vecs << 4) + static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < bytes; j += stride)
    dst[j] = src[j];
}

}  // namespace

hipError_t launch_window(const uint8_t* src, uint8_t* dst, int64_t batch, int64_t total,
                         int64_t start, int64_t count, int64_t rowbytes,
                         hipStream_t stream) {
  if (batch <= 0 || count <= 0) return hipSuccess;
  const uint64_t mix = reinterpret_cast<uint64_t>(src) | reinterpret_cast<uint64_t>(dst) |
                       static_cast<uint64_t>(rowbytes);
  const int unit = mix % 16 == 0 ? 16 : mix % 8 == 0 ? 8 : mix % 4 == 0 ? 4 : mix % 2 == 0 ? 2 : 1;
  const int64_t units = count * rowbytes / unit;
  const int64_t bx = std::min<int64_t>((units + kThreads - 1) / kThreads, 1024);
  hipLaunchKernelGGL(window_kernel, dim3(static_cast<uint32_t>(bx), static_cast<uint32_t>(batch)),
                     dim3(kThreads), 0, stream, src, dst, total, start, count, rowbytes, unit, units);
  return hipGetLastError();
}

hipError_t launch_copy_bytes(const void* src, void* dst, int64_t bytes, hipStream_t stream) {
  if (bytes <= 0) return hipSuccess;
  // one unit per lane up to 256 workgroups, then several per lane
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(256, ((bytes >> 4) + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(copy_bytes_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), bytes);
  return hipGetLastError();
}

hipError_t launch_mask_rows(const void* act, void* out, int64_t n, int64_t row_elems, int dtype,
                            const uint8_t* is_last, hipStream_t stream, uint32_t* counter, uint32_t* flag,
                            uint32_t seq) {
  const int64_t total = n * row_elems;
  if (total <= 0) return flag ? hipErrorInvalidValue : hipSuccess;
  const dim3 grid(static_cast<uint32_t>(std::min<int64_t>((total + kThreads - 1) / kThreads, 2048)));
#define EMB_MASK(T) hipLaunchKernelGGL(mask_rows_kernel<T>, grid, dim3(kThreads), 0, stream, static_cast<const T*>(act), static_cast<T*>(out), n, row_elems, is_last, counter, flag, seq)
  switch (dtype) {
    case kU8: case kBool: EMB_MASK(uint8_t); break;
    case kI8: EMB_MASK(int8_t); break;
    case kI16: EMB_MASK(int16_t); break;
    case kI32: EMB_MASK(int32_t); break;
    case kI64: EMB_MASK(int64_t); break;
    case kF16: EMB_MASK(_Float16); break;
    case kBF16: EMB_MASK(__hip_bfloat16); break;
    case kF32: EMB_MASK(float); break;
    case kF64: EMB_MASK(double); break;
    default: return hipErrorInvalidValue;
  }
#undef EMB_MASK
  return hipGetLastError();
}

hipError_t launch_publish_one(const void* src, void* pool, void* out, const int32_t* rows_dev,
                              const uint8_t* flags, int64_t n, int64_t rowbytes, int dtype,
                              hipStream_t stream, hipEvent_t stop, bool flags_by_row) {
  if (n <= 0 || rowbytes <= 0) return hipSuccess;
  PublishArgs a;
  a.src = static_cast<const uint8_t*>(src);
  a.pool = static_cast<uint8_t*>(pool);
  a.out = static_cast<uint8_t*>(out);
  a.rows = rows_dev;
  a.flags = flags;
  a.n = static_cast<int32_t>(n);
  a.rowbytes = static_cast<int32_t>(rowbytes);
  if (flags) {
    a.dtype = dtype | (flags_by_row ? 0x100 : 0);
    a.elem = dtype_size(dtype);
    if (a.elem == 0 || rowbytes % a.elem) return hipErrorInvalidValue;
  } else {
    a.dtype = kU8;       // plain copy: bytes
    a.elem = 1;
  }
  const int64_t elems = n * (rowbytes / a.elem);
  if (n > INT32_MAX || rowbytes > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((elems + kThreads - 1) / kThreads));
  if (stop) hipExtLaunchKernelGGL(publish_one_kernel, grid, dim3(kThreads), 0, stream, nullptr, stop, 0,
                                  a.src, a.pool, a.out, a.rows, a.flags, a.n, a.rowbytes, a.dtype, a.elem);
  else hipLaunchKernelGGL(publish_one_kernel, grid, dim3(kThreads), 0, stream,
                          a.src, a.pool, a.out, a.rows, a.flags, a.n, a.rowbytes, a.dtype, a.elem);
  return hipGetLastError();
}

bool prewrite_supported(const PrewritePlan& p) {
  // (one-dimensional grid of n * (frame blocks + 1) workgroups, 32-bit pixel count)
  return p.n > 0 && p.n <= (1 << 24) && p.pixels > 0 && p.pixels <= INT32_MAX && p.pixels % 4 == 0 &&
         p.channels >= 1 && p.channels <= 4 &&
         reinterpret_cast<uint64_t>(p.frames) % 16 == 0 &&
         reinterpret_cast<uint64_t>(p.frame_pool) % 16 == 0 &&
         (p.pixels * p.channels) % 16 == 0 &&
         reinterpret_cast<uint64_t>(p.dst) % 16 == 0 && p.n_narrow >= 0 && p.n_narrow <= kPreNarrow &&
         (p.out_dtype == kU8 || p.out_dtype == kF16 || p.out_dtype == kBF16 || p.out_dtype == kF32);
}

size_t prewrite_table_bytes(int64_t n) {
  return offsetof(PreTable, words) + static_cast<size_t>(n) * 7 * sizeof(uint32_t);
}

void prewrite_fill_table(void* dst, const PrewritePlan& p, const int32_t* rows, const uint8_t* stepids) {
  // (dst may be write-combined device memory behind the BAR: written once, front to back.)
  PreTable head;
  head.stepid_pool = p.stepid_pool;
  head.rows_out = p.rows_out;
  for (int k = 0; k < kPreNarrow; ++k)
    head.narrow[k] = k < p.n_narrow ? PreKey{p.narrow[k].src, p.narrow[k].pool, p.narrow[k].rowbytes}
                                    : PreKey{nullptr, nullptr, 0};
  head.carry = PreCarry{nullptr, nullptr, nullptr, 0, 0, 1, 0};
  if (p.carry_src && p.carry_rows) {
    const int elem = dtype_size(p.carry_dtype);
    head.carry = PreCarry{p.carry_src, p.carry_pool, p.carry_flags, static_cast<int32_t>(p.carry_rowbytes),
                          p.carry_dtype, elem > 0 ? elem : 1, 0};
  }
  uint8_t* out = static_cast<uint8_t*>(dst);
  std::memcpy(out, &head, offsetof(PreTable, words));
  out += offsetof(PreTable, words);
  std::memcpy(out, rows, static_cast<size_t>(p.n) * sizeof(int32_t));
  out += static_cast<size_t>(p.n) * sizeof(int32_t);
  std::memcpy(out, stepids, static_cast<size_t>(p.n) * kStepBytes);
  out += static_cast<size_t>(p.n) * kStepBytes;
  if (head.carry.src) std::memcpy(out, p.carry_rows, static_cast<size_t>(p.n) * sizeof(int32_t));
}

bool carry_supported(int64_t rowbytes, int dtype) {
  const int elem = dtype_size(dtype);
  return elem > 0 && rowbytes > 0 && rowbytes % elem == 0 && rowbytes / elem <= kThreads &&
         rowbytes <= INT32_MAX;
}

hipError_t launch_obs_stack_insert(const PrewritePlan& p, hipStream_t stream, hipEvent_t stop) {
  if (!prewrite_supported(p) || !p.table_dev) return hipErrorInvalidValue;
  PrewriteArgs a;
  a.frames = p.frames;
  a.dst = p.dst;
  a.frame_pool = p.frame_pool;
  a.pixels = static_cast<int32_t>(p.pixels);
  a.frame_blocks = static_cast<int32_t>(std::min<int64_t>((p.pixels / 4 + kThreads - 1) / kThreads, 32));
  a.scale = p.scale;
  a.offset = p.offset;
  a.n = p.n;
  a.n_narrow = p.n_narrow;
  a.table = static_cast<const PreTable*>(p.table_dev);
  switch (p.out_dtype) {
    case kU8: return obs_stack_insert_typed<uint8_t>(a, p.channels, p.layout, stream, stop);
    case kF16: return obs_stack_insert_typed<__half>(a, p.channels, p.layout, stream, stop);
    case kBF16: return obs_stack_insert_typed<__hip_bfloat16>(a, p.channels, p.layout, stream, stop);
    default: return obs_stack_insert_typed<float>(a, p.channels, p.layout, stream, stop);
  }
}

hipError_t launch_obs_stack(const uint8_t* src, const int32_t* env_ids, void* dst, int64_t n,
                            int64_t pixels, int64_t channels, int layout, int out_dtype,
                            float scale, float offset, hipStream_t stream) {
  if (n <= 0 || pixels <= 0 || channels <= 0) return hipSuccess;
  switch (out_dtype) {
    case kU8: return obs_stack_typed<uint8_t>(src, env_ids, dst, n, pixels, channels, layout, scale, offset, stream);
    case kF16: return obs_stack_typed<__half>(src, env_ids, dst, n, pixels, channels, layout, scale, offset, stream);
    case kBF16: return obs_stack_typed<__hip_bfloat16>(src, env_ids, dst, n, pixels, channels, layout, scale, offset, stream);
    case kF32: return obs_stack_typed<float>(src, env_ids, dst, n, pixels, channels, layout, scale, offset, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace emb
