// Launchers of the blocked GRU gate kernels in gru_gate.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

// x: (rows, 3 * deter) as the `dyngru` BlockLinear leaves it, deter: (rows, deter),
// both float32 or both bfloat16; `blocks` divides deter, h = deter / blocks.
// dreamerv3/rssm.py:153-158 for block k and j < h, in float32, rounded once at the store:
//   reset = sigmoid(x[r, 3hk + j]), cand = tanh(reset * x[r, 3hk + h + j]),
//   update = sigmoid(x[r, 3hk + 2h + j] - 1)
//   out[r, hk + j] = update * cand + (1 - update) * deter[r, hk + j]
// rows, deter >= 1, rows * 3 * deter <= 2^31 - 1 (refused otherwise).
hipError_t launch_gru_gate(const void* x, const void* deter, bool bf16, int64_t rows, int64_t width, int64_t blocks,
                           void* out, hipStream_t stream);

// dx (rows, 3 * deter) and ddeter (rows, deter) in the inputs' dtype, from x, deter
// and gout (rows, deter) in one launch; either may be null (not written).
hipError_t launch_gru_gate_grad(const void* x, const void* deter, const void* gout, bool bf16, int64_t rows,
                                int64_t width, int64_t blocks, void* dx, void* ddeter, hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t gru_gate_launches();

}  // namespace emb
