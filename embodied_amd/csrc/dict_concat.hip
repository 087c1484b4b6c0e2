// nn.DictConcat in one launch (dict_concat.h): what the world model's scan does
// before its first GEMM --
//   embodied/jax/nets.py:476-500   per key: available, mask, one_hot or squish,
//                                  the cast, mask again, reshape; then concatenate
//   embodied/jax/nets.py:80-99     available with bdims: a row of a key is there
//                                  unless one of its elements is -inf (floats) or -1
//                                  (signed integers)
//   dreamerv3/rssm.py:76-79        mask(action, ~reset) before and after
//   dreamerv3/rssm.py:137          action /= max(1, |action|)
// With torch ops these are twenty to thirty launches for a dict of two keys.
//
// Geometry.  L = 8, 16, 32 or 64 lanes of a wave64 share one output row (the
// ladder of dict_concat.h), 256 / L rows per workgroup, at most kDictMaxBlocks
// workgroups, a grid stride over the rows beyond them.
//   1. Availability: the L lanes walk the E elements of every key whose dtype
//      can be unavailable, each lane sets bit k of a word for a bad element of key
//      k, and one OR butterfly over the L lanes gives every lane the row's word.
//      No LDS, no atomics; the inputs of adjacent rows are adjacent in memory.
//   2. Columns: a row is cut at the 16-byte boundaries of ITS OWN address into a
//      head of fewer than 16 bytes, whole 16-byte groups and a tail; group j goes
//      to lane j mod L.  A lane holds its group's 4 float32 or 8 bfloat16 values
//      in registers, fills them key by key and stores a whole group with one
//      16-byte store, head and tail element by element with the same bits.
// The key loop is uniform over the wave (the table is read with scalar loads, the
// dtype and kind branches are scalar branches), and a key whose span cannot meet
// the columns the wave holds in this round is skipped.
//
// An index is compared with the column's class and is never used as an address.
// Arithmetic is float32, rounded once at the store.
#include "dict_concat.h"
#include "wave_util.h"

namespace emb {
namespace {

using segment::bf16_t;

template <int L>
__device__ __forceinline__ uint32_t seg_or(uint32_t v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, kDictWave);
  return v;
}

// Element i of a key's input as the float32 the reference's astype gives.
template <int DT>
__device__ __forceinline__ float as_float(uint64_t x, uint32_t i) {
  if constexpr (DT == EMB_F32) return reinterpret_cast<const float*>(x)[i];
  else if constexpr (DT == EMB_BF16) return segment::widen(reinterpret_cast<const bf16_t*>(x)[i]);
  else if constexpr (DT == EMB_I32) return static_cast<float>(reinterpret_cast<const int32_t*>(x)[i]);
  else if constexpr (DT == EMB_I64) return static_cast<float>(reinterpret_cast<const int64_t*>(x)[i]);
  else if constexpr (DT == EMB_U8) return static_cast<float>(reinterpret_cast<const uint8_t*>(x)[i]);
  else return reinterpret_cast<const uint8_t*>(x)[i] ? 1.f : 0.f;
}

// ... and as an index, 64 bits wide: an int64 beyond the int32 range matches no class.
template <int DT>
__device__ __forceinline__ int64_t as_index(uint64_t x, uint32_t i) {
  if constexpr (DT == EMB_I32) return reinterpret_cast<const int32_t*>(x)[i];
  else if constexpr (DT == EMB_I64) return reinterpret_cast<const int64_t*>(x)[i];
  else if constexpr (DT == EMB_U8) return reinterpret_cast<const uint8_t*>(x)[i];
  else return reinterpret_cast<const uint8_t*>(x)[i] ? 1 : 0;
}

// nets.py:84-87: is one of the row's elements that this lane walks unavailable?
template <int DT, int L>
__device__ __forceinline__ bool lane_unavailable(const DictKey& e, uint32_t row, uint32_t lane) {
  const uint32_t base = row * static_cast<uint32_t>(e.elements);
  bool bad = false;
  for (uint32_t i = lane; i < static_cast<uint32_t>(e.elements); i += L) {
    if constexpr (DT == EMB_F32 || DT == EMB_BF16) bad |= as_float<DT>(e.x, base + i) == -__builtin_inff();
    else bad |= as_index<DT>(e.x, base + i) == -1;
  }
  return bad;
}

template <int L>
__device__ __forceinline__ bool key_unavailable(const DictKey& e, uint32_t row, uint32_t lane) {
  switch (e.dtype) {
    case EMB_F32: return lane_unavailable<EMB_F32, L>(e, row, lane);
    case EMB_BF16: return lane_unavailable<EMB_BF16, L>(e, row, lane);
    case EMB_I32: return lane_unavailable<EMB_I32, L>(e, row, lane);
    case EMB_I64: return lane_unavailable<EMB_I64, L>(e, row, lane);
    default: return false;                         // unsigned and bool: always there (nets.py:88-92)
  }
}

__device__ __forceinline__ float symlog(float x) { return copysignf(log1pf(fabsf(x)), x); }      // nets.py:59-60

// The columns [c0, c1) of a lane's group that lie in key e, into v[c - c0].
template <int G, int DT, int KIND>
__device__ __forceinline__ void fill(float (&v)[G], const DictKey& e, uint32_t row, int32_t c0, int32_t c1, bool unit) {
  const int32_t from = max(c0, e.first), to = min(c1, e.first + e.span);
  if (from >= to) return;
  const uint32_t base = row * static_cast<uint32_t>(e.elements);
  if constexpr (KIND == EMB_DICT_ONEHOT) {
    const uint32_t rel = static_cast<uint32_t>(from - e.first), classes = static_cast<uint32_t>(e.classes);
    uint32_t element = rel / classes;
    int32_t cls = static_cast<int32_t>(rel - element * classes);
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int32_t c = c0 + i;
      if (c >= from && c < to) {
        v[i] = as_index<DT>(e.x, base + element) == static_cast<int64_t>(cls) ? 1.f : 0.f;
        if (++cls == e.classes) {
          cls = 0;
          ++element;
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int32_t c = c0 + i;
      if (c >= from && c < to) {
        float x = as_float<DT>(e.x, base + static_cast<uint32_t>(c - e.first));
        if constexpr (KIND == EMB_DICT_SYMLOG) x = symlog(x);
        v[i] = unit ? x / fmaxf(1.f, fabsf(x)) : x;                  // rssm.py:137: x itself, or +-1
      }
    }
  }
}

template <int G>
__device__ __forceinline__ void fill_key(float (&v)[G], const DictKey& e, uint32_t row, int32_t c0, int32_t c1, bool unit) {
  if (e.kind == EMB_DICT_ONEHOT) {
    switch (e.dtype) {
      case EMB_I32: return fill<G, EMB_I32, EMB_DICT_ONEHOT>(v, e, row, c0, c1, unit);
      case EMB_I64: return fill<G, EMB_I64, EMB_DICT_ONEHOT>(v, e, row, c0, c1, unit);
      case EMB_U8: return fill<G, EMB_U8, EMB_DICT_ONEHOT>(v, e, row, c0, c1, unit);
      default: return fill<G, EMB_BOOL, EMB_DICT_ONEHOT>(v, e, row, c0, c1, unit);
    }
  }
  if (e.kind == EMB_DICT_SYMLOG) {
    if (e.dtype == EMB_F32) return fill<G, EMB_F32, EMB_DICT_SYMLOG>(v, e, row, c0, c1, unit);
    return fill<G, EMB_BF16, EMB_DICT_SYMLOG>(v, e, row, c0, c1, unit);
  }
  switch (e.dtype) {
    case EMB_F32: return fill<G, EMB_F32, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
    case EMB_BF16: return fill<G, EMB_BF16, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
    case EMB_I32: return fill<G, EMB_I32, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
    case EMB_I64: return fill<G, EMB_I64, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
    case EMB_U8: return fill<G, EMB_U8, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
    default: return fill<G, EMB_BOOL, EMB_DICT_NONE>(v, e, row, c0, c1, unit);
  }
}

__device__ __forceinline__ void store_group(float* at, const float (&v)[4]) {
  *reinterpret_cast<float4*>(at) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_group(bf16_t* at, const float (&v)[8]) {
  uint4 q;
  q.x = segment::bf16_bits(v[0]) | static_cast<uint32_t>(segment::bf16_bits(v[1])) << 16;
  q.y = segment::bf16_bits(v[2]) | static_cast<uint32_t>(segment::bf16_bits(v[3])) << 16;
  q.z = segment::bf16_bits(v[4]) | static_cast<uint32_t>(segment::bf16_bits(v[5])) << 16;
  q.w = segment::bf16_bits(v[6]) | static_cast<uint32_t>(segment::bf16_bits(v[7])) << 16;
  *reinterpret_cast<uint4*>(at) = q;
}

// The scalar arguments come first: they arrive with the wave (kernel-argument
// preload), the table behind them is read with scalar loads.
template <typename Out, int L>
__global__ __launch_bounds__(kDictBlock) void dict_concat_kernel(Out* __restrict__ out, const uint8_t* __restrict__ reset,
                                                                 int64_t stride, int32_t rows, int32_t width,
                                                                 int32_t count, int32_t unit, const DictTable table) {
  constexpr int G = 16 / sizeof(Out);              // values of one 16-byte store
  constexpr int kRows = kDictBlock / L;            // rows of a workgroup
  const uint32_t lane = threadIdx.x % L;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kRows + threadIdx.x / L; r < rows;
       r += static_cast<int64_t>(gridDim.x) * kRows) {
    const uint32_t row = static_cast<uint32_t>(r);
    const bool zero = reset && reset[row];         // rssm.py:76-79: the whole row
    uint32_t bad = 0;
    if (!zero)
      for (int32_t k = 0; k < count; ++k) {
        const DictKey e = table.e[k];
        if (e.dtype == EMB_U8 || e.dtype == EMB_BOOL) continue;
        bad |= key_unavailable<L>(e, row, lane) ? 1u << k : 0u;
      }
    bad = seg_or<L>(bad);                          // the L lanes of a row are all here or all gone
    Out* orow = out + r * stride;
    const int32_t head =
        min(width, static_cast<int32_t>(((16 - (reinterpret_cast<uintptr_t>(orow) & 15)) & 15) / sizeof(Out)));
    const int32_t groups = 1 + (width - head + G - 1) / G;          // group 0 is the head, possibly empty
    for (int32_t first = 0; first < groups; first += L) {
      const int32_t j = first + static_cast<int32_t>(lane);
      const int32_t c0 = j == 0 ? 0 : min(width, head + (j - 1) * G);
      const int32_t c1 = j == 0 ? head : min(width, c0 + G);
      // the columns the wave's rows hold in this round, whatever their heads
      const int32_t lo = first == 0 ? 0 : (first - 1) * G, hi = (first + L) * G;
      float v[G];
#pragma unroll
      for (int i = 0; i < G; ++i) v[i] = 0.f;
      for (int32_t k = 0; k < count; ++k) {
        const DictKey e = table.e[k];
        if (e.first >= hi || e.first + e.span <= lo) continue;      // uniform: a scalar branch
        if (!zero && !((bad >> k) & 1u)) fill_key<G>(v, e, row, c0, c1, unit != 0);
      }
      if (j > 0 && c1 - c0 == G) {
        store_group(orow + c0, v);
      } else {
#pragma unroll
        for (int i = 0; i < G; ++i)
          if (c0 + i < c1) segment::store(orow, c0 + i, v[i]);
      }
    }
  }
}

segment::LaunchCount g_count;

template <typename Out, int L>
void launch(const DictTable& table, int count, int64_t rows, int64_t width, void* out, int64_t stride,
            const uint8_t* reset, bool unit, hipStream_t stream) {
  constexpr int kRows = kDictBlock / L;
  const int64_t want = (rows + kRows - 1) / kRows;
  const int blocks = static_cast<int>(want < kDictMaxBlocks ? want : kDictMaxBlocks);
  hipLaunchKernelGGL((dict_concat_kernel<Out, L>), dim3(blocks), dim3(kDictBlock), 0, stream, static_cast<Out*>(out),
                     reset, stride, static_cast<int32_t>(rows), static_cast<int32_t>(width), static_cast<int32_t>(count),
                     static_cast<int32_t>(unit), table);
}

template <typename Out>
void launch_lanes(int lanes, const DictTable& table, int count, int64_t rows, int64_t width, void* out, int64_t stride,
                  const uint8_t* reset, bool unit, hipStream_t stream) {
  switch (lanes) {
    case 8: return launch<Out, 8>(table, count, rows, width, out, stride, reset, unit, stream);
    case 16: return launch<Out, 16>(table, count, rows, width, out, stride, reset, unit, stream);
    case 32: return launch<Out, 32>(table, count, rows, width, out, stride, reset, unit, stream);
    default: return launch<Out, 64>(table, count, rows, width, out, stride, reset, unit, stream);
  }
}

}  // namespace

int64_t dict_concat_launches() { return g_count.value(); }

hipError_t launch_dict_concat(const DictTable& table, int count, int64_t rows, int64_t width, void* out,
                              int64_t out_stride, bool bf16, const uint8_t* reset, bool unit, hipStream_t stream) {
  if (count < 1 || count > kDictMaxKeys || rows < 1 || width < 1 || width > kDictMaxWidth || out_stride < width ||
      rows > kDictMaxElements / out_stride || !out)
    return hipErrorInvalidValue;
  const int lanes = dict_concat_lanes(width);
  if (bf16) launch_lanes<bf16_t>(lanes, table, count, rows, width, out, out_stride, reset, unit, stream);
  else launch_lanes<float>(lanes, table, count, rows, width, out, out_stride, reset, unit, stream);
  return g_count.launched();
}

}  // namespace emb
