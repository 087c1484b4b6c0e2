// BlockLinear (embodied/jax/nets.py:254-281) on the bf16 matrix cores: the launch
// plan.  No HIP types: a host compiler can include this file, and
// `block_linear_plan` runs without a GPU.
//
// The plan only.  The kernels it was drawn for are not in the tree (DESIGN.md says
// why), so nothing launches through it yet.  ONE function sizes everything: the
// launchers are to take their grids, their pass counts, the number of row splits
// of dW and the workspace size from `block_linear_plan` and from nothing else;
// emb_block_linear_plan exports it, so Python can ask it for the workspace instead
// of restating a formula, and a CPU test can walk it over every shape.
//
// Index rule: the ABI REFUSES any shape for which x, out / gout, W or the
// workspace holds more than 2^31 - 1 elements (`block_linear_shape_error` below,
// which `shape_ok` in block_linear_abi.cpp calls).
#pragma once

#include <cstdint>

#include "../../include/embodied_hip.h"

namespace emb {

// Geometry (tests/block_linear_cases.py was drawn for these switch points).
constexpr int kBlThreads = 256;                   // four waves
constexpr int kBlMfmaK = 32, kBlMfmaN = 16;       // v_mfma_f32_16x16x32_bf16
constexpr int64_t kBlSkinnyRows = 32;             // up to here: 32 rows x 16 columns per workgroup, K split over its waves
constexpr int64_t kBlTiledRows = 128;             // above: 128 rows (32 per wave) x 64 columns per workgroup
constexpr int64_t kBlTiledCols = 64;
constexpr int64_t kBlMaxRowBlocks = 1024;         // row blocks per grid pass; more rows: the workgroup loops
constexpr int64_t kBlGradTile = 64;               // dW: 64 x 64 of (I, O) per workgroup ...
constexpr int64_t kBlGradRows = 32;               // ... walking 32 rows at a time
constexpr int64_t kBlGradSplitRows = 256;         // one row split of dW per this many rows ...
constexpr int64_t kBlGradMaxSplits = 8;           // ... and never more than this many
// The workspace holds `splits` partial copies of dW and dbias (none for one
// split).  dbias is at most 1/8 of dW (I >= 8), so the workspace is at most this
// multiple of dW's own bytes whatever the row count.
constexpr int64_t kBlWorkspaceMaxMultiple = kBlGradMaxSplits + 1;
constexpr int64_t kBlSumThreads = 256, kBlSumMaxBlocks = 2048;
constexpr int64_t kBlMaxElements = INT32_MAX;

constexpr int32_t kBlOut = EMB_BLOCK_LINEAR_OUT, kBlDx = EMB_BLOCK_LINEAR_DX, kBlDw = EMB_BLOCK_LINEAR_DW,
                  kBlDbias = EMB_BLOCK_LINEAR_DBIAS;

inline int64_t bl_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// nullptr, or why the kernels do not take (rows, g, I, O) for the outputs asked for (a mask of
// EMB_BLOCK_LINEAR_*; the workspace bound holds only where dW or dbias is).  rows = 0 is fine (nothing is launched).
inline const char* block_linear_shape_error(int64_t rows, int64_t g, int64_t I, int64_t O, int32_t outputs) {
  if (rows < 0) return "negative rows";
  if (g < 1 || I < 1 || O < 1) return "g, I and O must be at least 1";
  if (g > 65535) return "more than 65535 blocks (grid y)";
  if (I % 8 || O % 8) return "I and O must be multiples of 8 (16-byte rows of x, gout and W)";
  if (I > kBlMaxElements / g || O > kBlMaxElements / g || I * O > kBlMaxElements / g)
    return "more than 2^31 - 1 elements of W";
  if (rows > kBlMaxElements / (g * I) || rows > kBlMaxElements / (g * O)) return "more than 2^31 - 1 elements of x or out";
  if ((outputs & (kBlDw | kBlDbias)) && (g * I * O + g * O) > kBlMaxElements / kBlGradMaxSplits)
    return "more than 2^31 - 1 elements of workspace";
  return nullptr;
}

// One (K, N) product launch: forward is K = I, N = O; dx is K = O, N = I.
inline emb_block_linear_launch_t bl_product_launch(int64_t rows, int64_t g, int64_t K, int64_t N) {
  emb_block_linear_launch_t l{};
  const bool skinny = rows <= kBlSkinnyRows;
  l.block = kBlThreads;
  l.row_tile = skinny ? kBlSkinnyRows : kBlTiledRows;
  l.col_tile = skinny ? kBlMfmaN : kBlTiledCols;
  l.col_tiles = bl_ceil(N, l.col_tile);
  l.k_tile = skinny ? kBlMfmaK * (kBlThreads / 64) : kBlMfmaK;      // skinny: each wave every fourth K step
  l.k_steps = bl_ceil(K, l.k_tile);
  const int64_t row_blocks = bl_ceil(rows, l.row_tile);
  l.grid_x = l.col_tiles;
  l.grid_y = g;
  l.grid_z = row_blocks < kBlMaxRowBlocks ? row_blocks : kBlMaxRowBlocks;
  l.passes = bl_ceil(row_blocks, l.grid_z);
  return l;
}

// rows >= 1 and a shape `block_linear_shape_error` accepts; `outputs` a mask of EMB_BLOCK_LINEAR_*.
inline emb_block_linear_plan_t block_linear_plan(int64_t rows, int64_t g, int64_t I, int64_t O, int32_t outputs) {
  emb_block_linear_plan_t p{};
  p.workspace_max_multiple = kBlWorkspaceMaxMultiple;
  if (outputs & kBlOut) p.forward = bl_product_launch(rows, g, I, O);
  if (outputs & kBlDx) p.grad_x = bl_product_launch(rows, g, O, I);
  if (outputs & (kBlDw | kBlDbias)) {
    const bool dw = outputs & kBlDw, db = outputs & kBlDbias;
    emb_block_linear_launch_t& l = p.grad_w;
    const int64_t want = bl_ceil(rows, kBlGradSplitRows);
    p.splits = want < kBlGradMaxSplits ? want : kBlGradMaxSplits;
    p.split_rows = bl_ceil(bl_ceil(rows, p.splits), kBlGradRows) * kBlGradRows;
    l.block = kBlThreads;
    l.row_tile = kBlGradRows;
    l.passes = p.split_rows / kBlGradRows;
    l.col_tile = kBlGradTile;
    l.col_tiles = bl_ceil(O, kBlGradTile);
    l.k_tile = kBlGradTile;
    l.k_steps = dw ? bl_ceil(I, kBlGradTile) : 1;                    // dbias alone: one tile of I, not read
    l.grid_x = l.col_tiles * l.k_steps;
    l.grid_y = g;
    l.grid_z = p.splits;
    p.launches_grad_w = p.splits > 1 ? 2 : 1;
    if (p.splits > 1) {
      p.workspace_bytes = p.splits * ((dw ? g * I * O : 0) + (db ? g * O : 0)) * 4;
      const int64_t blocks = bl_ceil((dw ? g * I * O : 0) + (db ? g * O : 0), kBlSumThreads);
      p.sum_grid_x = blocks < kBlSumMaxBlocks ? blocks : kBlSumMaxBlocks;
    }
  }
  return p;
}

}  // namespace emb
