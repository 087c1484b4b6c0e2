// Launchers of the norm + activation kernels in norm_act.hip (host-callable, no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

constexpr int kNormActMaxUnits = 16384;    // the forward: a row in the registers of one workgroup of 1024, 16 values per thread
constexpr int kNormActWaveUnits = 1024;    // up to here one wave64 takes a row (16 values per lane), 4 rows per workgroup
constexpr int kNormActMaxPartials = 512;   // workgroups of the gradient launch = rows of per-workgroup partial sums

enum NormImpl : int32_t { kNormRms = 0, kNormLayer = 1 };
enum NormAct : int32_t { kActNone = 0, kActSilu = 1, kActGelu = 2, kActRelu = 3 };

// Workgroups of the gradient launch, each of which leaves one row of partial sums.
inline int64_t norm_act_partials(int64_t rows, int64_t units) {
  const int64_t per_block = units <= kNormActWaveUnits ? 4 : 1;
  const int64_t blocks = (rows + per_block - 1) / per_block;
  return blocks < kNormActMaxPartials ? blocks : kNormActMaxPartials;
}

// x, out: (rows, units) float32 or bfloat16; scale, shift: (units,) float32 or
// null (ones / zeros).  embodied/jax/nets.py:374-399 followed by nets.py:26-39, in
// float32, the activation on the float32 value, rounded once at the store:
//   rms    y = x * (rsqrt(mean(x^2) + eps) * scale)
//   layer  y = (x - mean) * (rsqrt(max(0, mean(x^2) - mean^2) + eps) * scale) + shift
//   out = act(y)
// A row whose mean(x^2) is not finite is NaN throughout.  1 <= units <=
// kNormActMaxUnits, rows >= 1, rows * units <= 2^31 - 1 (refused otherwise).
hipError_t launch_norm_act(const void* x, const float* scale, const float* shift, bool bf16, int64_t rows,
                           int64_t units, int32_t impl, int32_t act, float eps, void* out, hipStream_t stream);

// dx (rows, units) in the dtype of x and gout, dscale / dshift (units,) float32,
// each may be null (not written); everything is recomputed from x.  With dscale
// or dshift: every workgroup leaves its rows' column sums in `partials`, float32
// (2, norm_act_partials(rows, units), units) -- scale first, shift second -- and a
// second launch adds them in a fixed order.  Without: one launch, partials unused.
hipError_t launch_norm_act_grad(const void* x, const float* scale, const float* shift, const void* gout, bool bf16,
                                int64_t rows, int64_t units, int32_t impl, int32_t act, float eps, void* dx,
                                float* dscale, float* dshift, float* partials, hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t norm_act_launches();

}  // namespace emb
