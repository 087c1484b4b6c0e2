// Launchers of the conv-stage kernels in conv_stage.hip (host-callable, no torch):
// the tail of an Encoder stage, 2x2 max pool + Norm + activation
// (dreamerv3/rssm.py:238-241), and of a Decoder stage, Norm + activation + 2x
// nearest upsample (dreamerv3/rssm.py:327, 336-338, 346).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "norm_act.h"

namespace emb {

constexpr int kConvStageMaxUnits = 1024;      // channels: a pixel's row in the registers of one wave64, 16 values per lane
constexpr int kConvStageMaxBlocks = 2048;     // workgroups of a forward launch; more pixels: grid stride
constexpr int kConvStageMaxPartials = 1024;   // workgroups of a gradient launch = rows of per-workgroup partial sums

// Lanes of a wave64 that share one pixel's row of `units` channels, 8 values per
// lane (16 past 512 channels); 64 / lanes adjacent pixels are packed into a wave.
inline int conv_stage_lanes(int64_t units) { return units <= 64 ? 8 : units <= 128 ? 16 : units <= 256 ? 32 : 64; }

// Workgroups of a gradient launch over `pixels` Norm rows (pool: images * H/2 * W/2,
// upsample: images * H * W), each of which leaves one row of partial sums.
inline int64_t conv_stage_partials(int64_t pixels, int64_t units) {
  const int64_t per_block = 4 * (64 / conv_stage_lanes(units));
  const int64_t blocks = (pixels + per_block - 1) / per_block;
  return blocks < kConvStageMaxPartials ? blocks : kConvStageMaxPartials;
}

// x (images, H, W, C) float32 or bfloat16, channels last; scale, shift (C,)
// float32 or null (ones / zeros); impl, act, eps and the row arithmetic as
// launch_norm_act.  1 <= C <= kConvStageMaxUnits, images, H, W >= 1, and the
// larger of the two tensors holds at most 2^31 - 1 elements (refused otherwise).
//
// pool:  out (images, H/2, W/2, C) = act(Norm(max over the 2x2 window)), H and W
// even.  The max propagates a NaN; a pixel whose pooled row has a non-finite
// mean(x^2) is NaN throughout and no other pixel is touched.
hipError_t launch_pool_norm_act(const void* x, const float* scale, const float* shift, bool bf16, int64_t images,
                                int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                                hipStream_t stream);

// gout (images, H/2, W/2, C); dx (images, H, W, C): the pooled row's Norm/act
// gradient g as launch_norm_act_grad forms it, recomputed from x, then per window
// and channel g / count where x equals the max (count: the tied positions) and 0
// elsewhere (NaN in the whole window of a pixel whose g is NaN).  dscale, dshift,
// partials: as launch_norm_act_grad with conv_stage_partials(pixels, C) rows.
hipError_t launch_pool_norm_act_grad(const void* x, const float* scale, const float* shift, const void* gout, bool bf16,
                                     int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act,
                                     float eps, void* dx, float* dscale, float* dshift, float* partials,
                                     hipStream_t stream);

// upsample:  out (images, 2H, 2W, C), out[n, 2h+i, 2w+j] = act(Norm(x[n, h, w])), i, j in {0, 1}.
hipError_t launch_norm_act_upsample(const void* x, const float* scale, const float* shift, bool bf16, int64_t images,
                                    int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                                    hipStream_t stream);

// gout (images, 2H, 2W, C); per pixel of x the four rows of gout are added in
// float32 as ((0,0) + (0,1)) + ((1,0) + (1,1)), then launch_norm_act_grad's row.
hipError_t launch_norm_act_upsample_grad(const void* x, const float* scale, const float* shift, const void* gout,
                                         bool bf16, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl,
                                         int32_t act, float eps, void* dx, float* dscale, float* dshift,
                                         float* partials, hipStream_t stream);

// Kernel launches the four launchers have issued in this process.
int64_t conv_stage_launches();

}  // namespace emb
