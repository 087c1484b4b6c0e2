// Many small independent reductions in one launch: the metrics of imag_loss
// (dreamerv3/agent.py:424-442) and the loss means at the end of Agent.loss
// (dreamerv3/agent.py:239-240).  The table check and the device form of an entry
// are plain C++ without HIP types: a host compiler can include this file with
// EMB_STAT_ROWS_HOST_ONLY, and every refusal is reached without a GPU.
//
// An entry is a float32 matrix view (address, rows, cols, row stride in
// elements), optionally under an affine map whose (offset, scale) pair is read
// from device memory.  One workgroup per entry writes six float32 statistics.
#pragma once

#include <cstdint>

#include "../../include/embodied_hip.h"

namespace emb {

constexpr int kStatMaxEntries = EMB_STAT_MAX_ENTRIES;   // entries of one launch: imag_loss's 8 + 2 per key of 20 action keys
constexpr int kStatThreads = 1024;                      // one workgroup per entry
constexpr int kStatVector = 4;                          // floats of one 16-byte load
constexpr int64_t kStatPass = static_cast<int64_t>(kStatThreads) * kStatVector;   // elements one pass of the widest load covers
constexpr int kStatValues = EMB_STAT_VALUES;            // mean, std, absmean, min, max, rate
constexpr int64_t kStatMaxElements = INT32_MAX;

// What the kernels read, passed by value in the kernel arguments.  A view whose
// rows follow each other without a gap (stride == cols, or one row) arrives as one
// row of rows * cols elements.
struct StatEntry {
  uint64_t x, affine;      // device addresses; affine: (offset, scale) float32, unused with EMB_STAT_NONE
  int64_t stride;          // elements from one row to the next
  int32_t rows, cols;
  int32_t mode;            // EMB_STAT_*
  float weight;            // the entry's factor in the total (emb_stat_rows with `total`)
};
static_assert(sizeof(StatEntry) == 40, "the table is passed as 40-byte records");

struct StatTable {
  StatEntry e[kStatMaxEntries];
};

// nullptr, or what is wrong with the entry.
inline const char* stat_entry_error(const emb_stat_entry_t& e) {
  if (e.rows < 1 || e.cols < 1) return "stat_rows: rows or cols < 1";
  if (e.stride < e.cols) return "stat_rows: stride < cols";
  if (e.cols > kStatMaxElements || e.rows > kStatMaxElements / e.cols)
    return "stat_rows: an entry of more than 2^31 - 1 elements";
  if (e.mode != EMB_STAT_NONE && e.mode != EMB_STAT_MUL_ADD && e.mode != EMB_STAT_SUB_DIV)
    return "stat_rows: an unknown affine mode";
  if (!e.x || (e.mode != EMB_STAT_NONE && !e.affine)) return "stat_rows: a null address";
  if (reinterpret_cast<uintptr_t>(e.x) & 3 || (e.mode != EMB_STAT_NONE && reinterpret_cast<uintptr_t>(e.affine) & 3))
    return "stat_rows: an address off 4 bytes";
  return nullptr;
}

// The whole call: nullptr, or why it is refused.  Nothing is launched once
// anything is wrong, whichever entry it is in.
inline const char* stat_rows_error(const emb_stat_entry_t* entries, int64_t count, const void* out, const void* total) {
  if (count < 0 || count > INT32_MAX) return "stat_rows: the number of entries is outside 0 .. 2^31 - 1";
  if (count == 0) return nullptr;
  if (!entries || !out) return "stat_rows: a null address";
  if (reinterpret_cast<uintptr_t>(out) & 3 || reinterpret_cast<uintptr_t>(total) & 3)
    return "stat_rows: an address off 4 bytes";
  if (total && count > kStatMaxEntries) return "stat_rows: a total needs all of its entries in one launch";
  for (int64_t i = 0; i < count; ++i)
    if (const char* wrong = stat_entry_error(entries[i])) return wrong;
  return nullptr;
}

// An entry the check accepted, as the kernels read it.
inline StatEntry stat_entry_of(const emb_stat_entry_t& e) {
  StatEntry s{};
  s.x = reinterpret_cast<uintptr_t>(e.x);
  s.affine = e.mode == EMB_STAT_NONE ? 0 : reinterpret_cast<uintptr_t>(e.affine);
  s.mode = e.mode;
  s.weight = e.weight;
  if (e.stride == e.cols || e.rows == 1) {
    s.rows = 1;
    s.cols = static_cast<int32_t>(e.rows * e.cols);
    s.stride = s.cols;
  } else {
    s.rows = static_cast<int32_t>(e.rows);
    s.cols = static_cast<int32_t>(e.cols);
    s.stride = e.stride;
  }
  return s;
}

struct FillTable {
  emb_fill_entry_t e[kStatMaxEntries];
};

inline const char* mean_fill_error(const emb_fill_entry_t* entries, int64_t count, const void* g) {
  if (count < 0 || count > INT32_MAX) return "mean_fill: the number of entries is outside 0 .. 2^31 - 1";
  if (count == 0) return nullptr;
  if (!entries || !g) return "mean_fill: a null address";
  if (reinterpret_cast<uintptr_t>(g) & 3) return "mean_fill: an address off 4 bytes";
  for (int64_t i = 0; i < count; ++i) {
    if (entries[i].n < 1) return "mean_fill: an entry of less than 1 element";
    if (entries[i].n > kStatMaxElements) return "mean_fill: an entry of more than 2^31 - 1 elements";
    if (!entries[i].out) return "mean_fill: a null address";
    if (reinterpret_cast<uintptr_t>(entries[i].out) & 3) return "mean_fill: an address off 4 bytes";
  }
  return nullptr;
}

}  // namespace emb

#ifndef EMB_STAT_ROWS_HOST_ONLY
#include <hip/hip_runtime.h>

namespace emb {

// count = 1 .. kStatMaxEntries entries of `table`, one workgroup each, write
// out[e, 0:6].  With `total` one more workgroup re-reduces every entry and writes
// total[0] = 0 + mean_0 * weight_0 + mean_1 * weight_1 + ... in float32, left to right.
hipError_t launch_stat_rows(const StatTable& table, int count, float* out, float* total, hipStream_t stream);
// out_k[i] = (g[0] * scale_k) / n_k for every element of count = 1 .. kStatMaxEntries entries.
hipError_t launch_mean_fill(const FillTable& table, int count, const float* g, hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t stat_rows_launches();

}  // namespace emb
#endif  // EMB_STAT_ROWS_HOST_ONLY
