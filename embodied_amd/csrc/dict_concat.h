// nn.DictConcat (embodied/jax/nets.py:467-500) with the masks and the clamp around
// it (dreamerv3/rssm.py:76-79, 137) in one launch: the key table, its check and the
// launch geometry.  Everything above EMB_DICT_CONCAT_HOST_ONLY's #ifndef is plain
// C++ without HIP types: a host compiler can include this file with that macro,
// and every refusal is reached without a GPU.
//
// A key is a contiguous (rows, E) input of one of six dtypes.  It fills the
// columns [first, first + span) of every output row: span = E * classes for a
// one-hot key, E for a continuous one.  The spans of a table tile [0, width).
#pragma once

#include <cstdint>

#include "../../include/embodied_hip.h"

namespace emb {

constexpr int kDictMaxKeys = EMB_DICT_MAX_KEYS;      // keys of one launch; the availability flags of a row are one 16-bit word
constexpr int kDictMaxWidth = 16384;                 // columns of a row
constexpr int kDictMaxClasses = 16384;               // of a one-hot key
constexpr int64_t kDictMaxElements = INT32_MAX;      // rows * row stride: 32-bit index arithmetic
constexpr int kDictBlock = 256;                      // threads of a workgroup: four waves
constexpr int kDictMaxBlocks = 2048;                 // the grid's cap; more rows: grid stride
constexpr int kDictWave = 64;
// The packing ladder: a row of at most kDictLadderWidths[i] columns takes
// kDictLadderLanes[i] lanes of a wave64, a wider one the whole wave.
constexpr int kDictLadderSteps = 3;
constexpr int kDictLadderWidths[kDictLadderSteps] = {32, 64, 128};
constexpr int kDictLadderLanes[kDictLadderSteps + 1] = {8, 16, 32, 64};

// Lanes of a wave that share one row.
inline int dict_concat_lanes(int64_t width) {
  for (int i = 0; i < kDictLadderSteps; ++i)
    if (width <= kDictLadderWidths[i]) return kDictLadderLanes[i];
  return kDictLadderLanes[kDictLadderSteps];
}
// Rows one pass of the capped grid covers.
inline int64_t dict_concat_pass_rows(int64_t width) {
  return static_cast<int64_t>(kDictMaxBlocks) * (kDictBlock / dict_concat_lanes(width));
}

// What the kernel reads, passed by value in the kernel arguments.
struct DictKey {
  uint64_t x;              // device address of the (rows, E) input
  int32_t dtype, kind;     // EMB_F32 .., EMB_DICT_*
  int32_t elements;        // E
  int32_t classes;         // one-hot: classes, else 1
  int32_t first, span;     // output columns [first, first + span)
};
static_assert(sizeof(DictKey) == 32, "the table is passed as 32-byte records");

struct DictTable {
  DictKey e[kDictMaxKeys];
};

inline int dict_dtype_bytes(int32_t dtype) {
  switch (dtype) {
    case EMB_F32: case EMB_I32: return 4;
    case EMB_BF16: return 2;
    case EMB_I64: return 8;
    case EMB_U8: case EMB_BOOL: return 1;
    default: return 0;
  }
}
inline bool dict_dtype_float(int32_t dtype) { return dtype == EMB_F32 || dtype == EMB_BF16; }

// Columns of one key, or -1 where the entry itself is refused (dict_entry_error says why).
inline int64_t dict_entry_span(const emb_dict_entry_t& e) {
  return e.kind == EMB_DICT_ONEHOT ? static_cast<int64_t>(e.elements) * e.classes : e.elements;
}

// nullptr, or what is wrong with the entry on its own.
inline const char* dict_entry_error(const emb_dict_entry_t& e) {
  if (!e.x) return "dict_concat: a null address";
  if (!dict_dtype_bytes(e.dtype)) return "dict_concat: an unknown input dtype";
  if (e.kind != EMB_DICT_ONEHOT && e.kind != EMB_DICT_NONE && e.kind != EMB_DICT_SYMLOG)
    return "dict_concat: an unknown kind";
  if (e.elements < 1) return "dict_concat: a key of less than 1 element";
  if (e.kind == EMB_DICT_ONEHOT && dict_dtype_float(e.dtype)) return "dict_concat: one-hot of a float input";
  if (e.kind == EMB_DICT_SYMLOG && !dict_dtype_float(e.dtype)) return "dict_concat: squish of an integer input";
  if (e.kind == EMB_DICT_ONEHOT && (e.classes < 1 || e.classes > kDictMaxClasses))
    return "dict_concat: classes outside 1 .. 16384";
  if (reinterpret_cast<uintptr_t>(e.x) % dict_dtype_bytes(e.dtype)) return "dict_concat: an address off its element size";
  return nullptr;
}

// The whole call: nullptr, or why it is refused.  Nothing is launched once
// anything is wrong, whichever entry it is in; rows = 0 is checked like any call.
inline const char* dict_concat_error(const emb_dict_entry_t* table, int64_t count, int64_t rows, int64_t width,
                                     const void* out, int64_t out_stride, int32_t out_dtype) {
  if (count < 1 || count > kDictMaxKeys) return "dict_concat: the number of keys is outside 1 .. 16";
  if (!table || !out) return "dict_concat: a null address";
  if (out_dtype != EMB_F32 && out_dtype != EMB_BF16) return "dict_concat: out is neither float32 nor bfloat16";
  if (rows < 0) return "dict_concat: rows < 0";
  if (width < 1 || width > kDictMaxWidth) return "dict_concat: width outside 1 .. 16384";
  if (out_stride < width) return "dict_concat: out_stride < width";
  if (rows > kDictMaxElements / out_stride) return "dict_concat: more than 2^31 - 1 elements of out";
  if (reinterpret_cast<uintptr_t>(out) % dict_dtype_bytes(out_dtype)) return "dict_concat: an address off its element size";
  for (int64_t k = 0; k < count; ++k)
    if (const char* wrong = dict_entry_error(table[k])) return wrong;
  // the spans in the order of their first columns: each starts where the one before ends
  int order[kDictMaxKeys];
  for (int k = 0; k < count; ++k) {
    int at = k;
    for (; at > 0 && table[order[at - 1]].first > table[k].first; --at) order[at] = order[at - 1];
    order[at] = k;
  }
  int64_t next = 0;
  for (int k = 0; k < count; ++k) {
    const emb_dict_entry_t& e = table[order[k]];
    if (e.first < next) return "dict_concat: the spans overlap";
    if (e.first > next || dict_entry_span(e) > width - next) return "dict_concat: the spans do not tile [0, width)";
    next += dict_entry_span(e);
  }
  if (next != width) return "dict_concat: the spans do not tile [0, width)";
  return nullptr;
}

// An entry the check accepted, as the kernel reads it.
inline DictKey dict_key_of(const emb_dict_entry_t& e) {
  DictKey k{};
  k.x = reinterpret_cast<uintptr_t>(e.x);
  k.dtype = e.dtype;
  k.kind = e.kind;
  k.elements = e.elements;
  k.classes = e.kind == EMB_DICT_ONEHOT ? e.classes : 1;
  k.first = e.first;
  k.span = static_cast<int32_t>(dict_entry_span(e));
  return k;
}

}  // namespace emb

#ifndef EMB_DICT_CONCAT_HOST_ONLY
#include <hip/hip_runtime.h>

namespace emb {

// out[r, first_k + ...] for every row r < rows and key k < count of a table
// dict_concat_error accepted; rows >= 1.  `reset`: one byte per row or null.
hipError_t launch_dict_concat(const DictTable& table, int count, int64_t rows, int64_t width, void* out,
                              int64_t out_stride, bool bf16, const uint8_t* reset, bool unit, hipStream_t stream);

// Kernel launches the launcher has issued in this process.
int64_t dict_concat_launches();

}  // namespace emb
#endif  // EMB_DICT_CONCAT_HOST_ONLY
