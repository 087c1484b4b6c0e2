// Launchers of the reconstruction-loss kernels in recon_loss.hip (host-callable,
// no torch).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

// The four ops.  t = float32(raw target) / div in float32 (div == 1: the raw
// value), g the upstream gradient of the row, s(x) = 1 / (1 + exp(-x)):
//   kReconMse         loss = sum_j (x - t)^2                 grad = 2 (x - t) g
//   kReconMseSymlog   loss = sum_j (x - symlog t)^2          grad = 2 (x - symlog t) g
//                     symlog t = sign(t) log1p|t|            (embodied/jax/nets.py symlog)
//   kReconSigmoidMse  loss = sum_j (s(x) - t)^2              grad = 2 (s(x) - t) s(x) (1 - s(x)) g
//   kReconBinary      loss = sum_j -(t ls(x) + (1 - t) ls(-x)),  ls(x) = min(x, 0) - log1p(exp(-|x|))
//                                                            grad = (s(x) - t) g
// (embodied/jax/outs.py:129-141 MSE, 189-201 Binary, 40-58 Agg; dreamerv3/rssm.py:349,
// 353-356; dreamerv3/agent.py:170-182).
constexpr int kReconMse = 0;
constexpr int kReconMseSymlog = 1;
constexpr int kReconSigmoidMse = 2;
constexpr int kReconBinary = 3;

// Element types: x is kReconF32 or kReconBf16, the target any of the three.
constexpr int kReconF32 = 0;
constexpr int kReconBf16 = 1;
constexpr int kReconU8 = 2;

// The boundaries between the launch geometries, by the row's width `units`:
//   units <= kReconSegmentMaxUnits   a segment of W lanes per row, W the next power
//                                    of two >= units: 64 / W rows per wave, one
//                                    element per lane (the continue head: W = 1),
//                                    loaded and stored singly; the gradient is a
//                                    flat elementwise pass
//   units <= kReconWaveMaxUnits      one wave per row, 16-byte chunks of x per lane,
//                                    each read in the widest pieces its address allows
//   wider                            one workgroup of 4 waves per row (images)
constexpr int kReconSegmentMaxUnits = 64;
constexpr int kReconWaveMaxUnits = 2048;

// x, target: (rows, units) contiguous; loss[r] float32 = the row's sum, the terms
// added in an order that depends on (units, dtypes) alone: the same bits from run
// to run and whatever the alignment of the pointers.  A row holding a NaN or
// infinite x: NaN, no other row touched.  rows, units >= 1, rows * units <= 2^31 - 1.
hipError_t launch_recon_loss(const void* x, int x_dtype, const void* target, int target_dtype, float div,
                             int64_t rows, int64_t units, int op, float* loss, hipStream_t stream);

// grad (rows, units) in the dtype of x, rounded once at the store; gout[r] float32.
// A NaN or infinite x: that element NaN.
hipError_t launch_recon_loss_grad(const void* x, int x_dtype, const void* target, int target_dtype, float div,
                                  int64_t rows, int64_t units, int op, const float* gout, void* grad,
                                  hipStream_t stream);

// Kernel launches the two launchers have issued in this process.
int64_t recon_loss_launches();

}  // namespace emb
