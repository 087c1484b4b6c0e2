// The tails of DreamerV3's convolution stages, channels last:
//   pool      Encoder (dreamerv3/rssm.py:238-241): 2x2 max pool, Norm, activation
//   upsample  Decoder (dreamerv3/rssm.py:327, 336-338, 346): Norm, activation, every
//             pixel repeated 2x2
// each ONE launch forward and ONE backward that recomputes everything from x (with
// parameter gradients every workgroup also leaves the column sums of its pixels,
// and norm_act's reduce launch adds those in a fixed order).  With torch ops the
// pool or the repeat is a memory pass of its own over the largest activations of
// the model, on top of norm_act's chain.
//
// A Norm row is one pixel: an output pixel of the pool, an input pixel of the
// upsample, C <= 1024 channels.  It belongs to L = 8, 16, 32 or 64 lanes of a
// wave64 by its width, each holding PER = 8 of its values (16 past 512 channels) as
// norm_act_device.h's Map lays them out; 64 / L pixels that follow each other in
// (image, row, column) order share a wave, 256 / L a workgroup, so the wave's
// accesses to the larger tensor are runs of 2 * (64 / L) * C contiguous elements
// from image rows 2h and 2h + 1 (a wave that crosses the end of an image row
// starts new runs there).  Row sums are wave_util.h's butterflies over the L lanes.
// Loads and stores are 16 bytes where C is a multiple of that and every pointer
// is aligned, and element by element otherwise.  No atomics: the same bits run to run.
#include "conv_stage.h"
#include "norm_act_device.h"   // the row's thread map, statistics, activation, reduce launch; fp contract off

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                       // threads of every workgroup here
static_assert(kWave == kLanes && kBlock == kReduceBlock, "one wave64; the reduce launch is a workgroup of kBlock");

// The larger of two values that propagates a NaN (fmaxf drops one).  Exact.
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a >= b) ? a : b; }

// Where pixel p of the `wide` Norm pixels per image row has its 2x2 window in the
// larger tensor (rows of 2 * wide pixels): the element offset of position (0, 0);
// (i, j) is i * 2 * wide * units + j * units further.  p < 2^31.
__device__ __forceinline__ int64_t window_of(int64_t p, int32_t wide, int32_t units) {
  const uint32_t r = static_cast<uint32_t>(p) / static_cast<uint32_t>(wide);
  const uint32_t w = static_cast<uint32_t>(p) - r * static_cast<uint32_t>(wide);
  return (static_cast<int64_t>(r) * 4 * wide + 2 * static_cast<int64_t>(w)) * units;
}

// The four positions of a window, and per value the max over them.
template <typename M, int PER, typename T>
__device__ __forceinline__ void load_window(const T* at, int64_t stride, int units, int t, float (&w)[4][PER],
                                            float (&m)[PER]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) M::load(at + (k / 2) * stride + (k % 2) * units, units, t, 0.f, w[k]);
#pragma unroll
  for (int j = 0; j < PER; ++j) m[j] = nan_max(nan_max(w[0][j], w[1][j]), nan_max(w[2][j], w[3][j]));
}

// The kernels' loops over pixels end per pixel, not per wave: on a wave's last
// trip some of its 64 / L pixels may have left.  seg_sum<L> inside such a loop is
// safe because its xor offsets stay below L, so a lane only ever reads lanes of
// its own pixel, which are in the loop with it (as normal_policy.hip's rows).
// Anything that crosses pixels -- across_sum -- belongs behind the loop, where
// the whole wave has met again.
//
// v: a row's values (0 past `units`) -> act(Norm(v)), norm_act_kernel's arithmetic
// with the two sums over the row's L lanes.
template <typename M, int L, int PER>
__device__ __forceinline__ void row_forward(float (&v)[PER], const float* scale, const float* shift, int32_t units,
                                            int t, int32_t impl, int32_t act, float eps) {
  float sum = 0.f, sum2 = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    sum = sum + v[j];
    sum2 = sum2 + v[j] * v[j];
  }
  sum = seg_sum<L>(sum);
  sum2 = seg_sum<L>(sum2);
  const Stats s = stats_of(sum, sum2, units, impl, eps);
#pragma unroll
  for (int c = 0; c < PER / M::E; ++c) {                           // the parameters a part at a time: they stay in cache
    float g[M::E], b[M::E];
    M::load_part(scale, units, t, c, 1.f, g);
    M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
    for (int k = 0; k < M::E; ++k) {
      const int j = c * M::E + k;
      const float y = impl == kNormLayer ? (v[j] - s.mean) * (s.rstd * g[k]) + b[k]        // nets.py:395
                                         : v[j] * (s.rstd * g[k]);                          // nets.py:386
      v[j] = activate(y, act);
    }
  }
}

// v: a row's values, h: the gradient of its output -> v: the gradient of the row,
// norm_act_grad_kernel's arithmetic (the formulas stand there); the row's terms of
// the two column sums are added to dscale / dshift.
template <typename M, int L, int PER>
__device__ __forceinline__ void row_backward(float (&v)[PER], float (&h)[PER], const float* scale, const float* shift,
                                             int32_t units, int t, int32_t impl, int32_t act, float eps,
                                             float (&dscale)[PER], float (&dshift)[PER]) {
  const float n = static_cast<float>(units);
  float sum = 0.f, sum2 = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    sum = sum + v[j];
    sum2 = sum2 + v[j] * v[j];
  }
  sum = seg_sum<L>(sum);
  sum2 = seg_sum<L>(sum2);
  const Stats s = stats_of(sum, sum2, units, impl, eps);
  float sum_h = 0.f, sum_hx = 0.f;
#pragma unroll
  for (int c = 0; c < PER / M::E; ++c) {
    float g[M::E], b[M::E];
    M::load_part(scale, units, t, c, 1.f, g);
    M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
    for (int k = 0; k < M::E; ++k) {
      const int j = c * M::E + k;
      const bool live = M::index(j, t) < units;
      const float xc = impl == kNormLayer ? v[j] - s.mean : v[j];
      const float y = impl == kNormLayer ? xc * (s.rstd * g[k]) + b[k] : xc * (s.rstd * g[k]);
      const float dy = live ? h[j] * activate_slope(y, act) : 0.f;
      dscale[j] = dscale[j] + dy * (xc * s.rstd);
      dshift[j] = dshift[j] + dy;
      h[j] = dy * g[k];
      v[j] = live ? xc : 0.f;
      sum_h = sum_h + h[j];
      sum_hx = sum_hx + h[j] * v[j];
    }
  }
  sum_h = seg_sum<L>(sum_h);
  sum_hx = seg_sum<L>(sum_hx);
  const float r3 = s.rstd * s.rstd * s.rstd;
  const float pull = impl == kNormLayer ? (s.slope * r3) * sum_hx / n : r3 * sum_hx / n;
  const float centre = impl == kNormLayer ? sum_h / n : 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) v[j] = s.rstd * (h[j] - centre) - v[j] * pull;
}

// `pixels` Norm rows, `wide` of them per image row (pool: W / 2, upsample: W).
template <typename T, int L, int PER, bool VEC, bool POOL>
__global__ __launch_bounds__(kBlock) void conv_stage_kernel(
    const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, T* __restrict__ out,
    int32_t pixels, int32_t wide, int32_t units, int32_t impl, int32_t act, float eps) {
  using M = Map<T, L, PER, VEC>;
  constexpr int kPixels = kBlock / L;
  const int t = threadIdx.x % L, sub = threadIdx.x / L;
  const int64_t stride = 2 * static_cast<int64_t>(wide) * units;   // an image row of the larger tensor
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kPixels + sub; p < pixels;
       p += static_cast<int64_t>(gridDim.x) * kPixels) {            // uniform over the pixel's lanes
    const int64_t big = window_of(p, wide, units);
    float v[PER];
    if constexpr (POOL) {
      float w[4][PER];
      load_window<M>(x + big, stride, units, t, w, v);
    } else {
      M::load(x + p * units, units, t, 0.f, v);
    }
    row_forward<M, L>(v, scale, shift, units, t, impl, act, eps);
    if constexpr (POOL) {
      M::store(out + p * units, units, t, v);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) M::store(out + big + (k / 2) * stride + (k % 2) * units, units, t, v);
    }
  }
}

// The column sums: every lane adds its own columns over its pixels in registers;
// then the 64 / L pixels of a wave (butterflies), then the four waves through LDS
// in the order of the waves, and the workgroup's row of `partials` is written once.
template <typename T, int L, int PER, bool VEC, bool POOL>
__global__ __launch_bounds__(kBlock) void conv_stage_grad_kernel(
    const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const T* __restrict__ gout, T* __restrict__ dx, float* partials, int32_t pixels, int32_t wide, int32_t units,
    int32_t impl, int32_t act, float eps) {
  using M = Map<T, L, PER, VEC>;
  constexpr int kPixels = kBlock / L, kWaves = kBlock / kWave;
  __shared__ float meet[(kWaves - 1) * PER * L];
  const int t = threadIdx.x % L, sub = threadIdx.x / L;
  const int64_t stride = 2 * static_cast<int64_t>(wide) * units;
  float dscale[PER], dshift[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) dscale[j] = 0.f, dshift[j] = 0.f;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kPixels + sub; p < pixels;
       p += static_cast<int64_t>(gridDim.x) * kPixels) {            // uniform over the pixel's lanes
    const int64_t big = window_of(p, wide, units);
    float v[PER], h[PER];
    if constexpr (POOL) {
      float w[4][PER], m[PER];
      load_window<M>(x + big, stride, units, t, w, m);
      M::load(gout + p * units, units, t, 0.f, h);
#pragma unroll
      for (int j = 0; j < PER; ++j) v[j] = m[j];
      row_backward<M, L>(v, h, scale, shift, units, t, impl, act, eps, dscale, dshift);
      if (dx) {                                                    // uniform over the launch
        float share[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const float count = ((w[0][j] == m[j] ? 1.f : 0.f) + (w[1][j] == m[j] ? 1.f : 0.f)) +
                              ((w[2][j] == m[j] ? 1.f : 0.f) + (w[3][j] == m[j] ? 1.f : 0.f));
          share[j] = v[j] / count;                                 // torch.amax, jax's reduce_max: equal parts among ties
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float d[PER];
#pragma unroll
          for (int j = 0; j < PER; ++j) d[j] = w[k][j] == m[j] ? share[j] : (v[j] != v[j] ? v[j] : 0.f);
          M::store(dx + big + (k / 2) * stride + (k % 2) * units, units, t, d);
        }
      }
    } else {
      float g[4][PER];
#pragma unroll
      for (int k = 0; k < 4; ++k) M::load(gout + big + (k / 2) * stride + (k % 2) * units, units, t, 0.f, g[k]);
#pragma unroll
      for (int j = 0; j < PER; ++j) h[j] = (g[0][j] + g[1][j]) + (g[2][j] + g[3][j]);
      M::load(x + p * units, units, t, 0.f, v);
      row_backward<M, L>(v, h, scale, shift, units, t, impl, act, eps, dscale, dshift);
      if (dx) M::store(dx + p * units, units, t, v);
    }
  }
  if (!partials) return;                                           // uniform over the launch
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float* const my_scale = partials + static_cast<int64_t>(blockIdx.x) * units;
  float* const my_shift = my_scale + static_cast<int64_t>(gridDim.x) * units;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    float (&mine)[PER] = which ? dshift : dscale;
#pragma unroll
    for (int j = 0; j < PER; ++j) mine[j] = across_sum<L>(mine[j]);
    if (wave > 0 && lane < L) {
#pragma unroll
      for (int j = 0; j < PER; ++j) meet[((wave - 1) * PER + j) * L + t] = mine[j];
    }
    __syncthreads();
    if (wave == 0 && lane < L) {
#pragma unroll
      for (int j = 0; j < PER; ++j) {
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) mine[j] = mine[j] + meet[(w * PER + j) * L + t];
      }
      M::store(which ? my_shift : my_scale, units, t, mine);
    }
    __syncthreads();
  }
}

LaunchCount g_count;

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The Norm rows of a call, or 0 where the kernels do not take it (conv_stage.h).
int64_t pixels_of(bool pool, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act) {
  if (images < 1 || H < 1 || W < 1 || C < 1 || C > kConvStageMaxUnits) return 0;
  if ((impl != kNormRms && impl != kNormLayer) || act < kActNone || act > kActRelu) return 0;
  if (pool && (H % 2 || W % 2)) return 0;
  const int64_t grow = pool ? 1 : 4;                               // the larger tensor: x of the pool, out of the upsample
  int64_t room = INT32_MAX / (C * grow);
  if (images > room) return 0;
  room /= images;
  if (H > room || W > room / H) return 0;
  return pool ? images * (H / 2) * (W / 2) : images * H * W;
}

// lanes per pixel and values per lane by the row's width (conv_stage_lanes)
#define EMB_STAGE_BY_WIDTH(CALL, u)           \
  do {                                        \
    if ((u) <= 64) { CALL(8, 8); }            \
    else if ((u) <= 128) { CALL(16, 8); }     \
    else if ((u) <= 256) { CALL(32, 8); }     \
    else if ((u) <= 512) { CALL(64, 8); }     \
    else { CALL(64, 16); }                    \
  } while (0)
static_assert(kConvStageMaxUnits == 64 * 16, "the ladder above");

template <bool POOL>
hipError_t forward(const void* x, const float* scale, const float* shift, bool bf16, int64_t images, int64_t H,
                   int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out, hipStream_t stream) {
  const int64_t pixels = pixels_of(POOL, images, H, W, C, impl, act);
  if (!pixels || !x || !out) return hipErrorInvalidValue;
  const int64_t per = kBlock / conv_stage_lanes(C), blocks = (pixels + per - 1) / per;
  const dim3 grid(static_cast<unsigned>(blocks < kConvStageMaxBlocks ? blocks : kConvStageMaxBlocks)), block(kBlock);
  const int32_t n = static_cast<int32_t>(pixels), wide = static_cast<int32_t>(POOL ? W / 2 : W);
  const int32_t u = static_cast<int32_t>(C);
  const bool vec = C % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(out) && aligned16(scale) && aligned16(shift);
#define EMB_FORWARD_AS(T_, L_, PER_, VEC_)                                                              \
  hipLaunchKernelGGL((conv_stage_kernel<T_, L_, PER_, VEC_, POOL>), grid, block, 0, stream,             \
                     static_cast<const T_*>(x), scale, shift, static_cast<T_*>(out), n, wide, u, impl, act, eps)
#define EMB_FORWARD(L_, PER_)                                \
  if (bf16 && vec) EMB_FORWARD_AS(bf16_t, L_, PER_, true);   \
  else if (bf16) EMB_FORWARD_AS(bf16_t, L_, PER_, false);    \
  else if (vec) EMB_FORWARD_AS(float, L_, PER_, true);       \
  else EMB_FORWARD_AS(float, L_, PER_, false)
  EMB_STAGE_BY_WIDTH(EMB_FORWARD, C);
#undef EMB_FORWARD
#undef EMB_FORWARD_AS
  return g_count.launched();
}

template <bool POOL>
hipError_t backward(const void* x, const float* scale, const float* shift, const void* gout, bool bf16, int64_t images,
                    int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* dx, float* dscale,
                    float* dshift, float* partials, hipStream_t stream) {
  const int64_t pixels = pixels_of(POOL, images, H, W, C, impl, act);
  if (!pixels || !x || !gout) return hipErrorInvalidValue;
  if (!dx && !dscale && !dshift) return hipErrorInvalidValue;
  const bool params = dscale || dshift;
  if (params && !partials) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(conv_stage_partials(pixels, C))), block(kBlock);
  const int32_t n = static_cast<int32_t>(pixels), wide = static_cast<int32_t>(POOL ? W / 2 : W);
  const int32_t u = static_cast<int32_t>(C);
  float* part = params ? partials : nullptr;
  const bool vec = C % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(gout) && aligned16(dx) && aligned16(scale) &&
                   aligned16(shift) && aligned16(part);
#define EMB_GRAD_AS(T_, L_, PER_, VEC_)                                                                  \
  hipLaunchKernelGGL((conv_stage_grad_kernel<T_, L_, PER_, VEC_, POOL>), grid, block, 0, stream,         \
                     static_cast<const T_*>(x), scale, shift, static_cast<const T_*>(gout), static_cast<T_*>(dx), \
                     part, n, wide, u, impl, act, eps)
#define EMB_GRAD(L_, PER_)                               \
  if (bf16 && vec) EMB_GRAD_AS(bf16_t, L_, PER_, true);  \
  else if (bf16) EMB_GRAD_AS(bf16_t, L_, PER_, false);   \
  else if (vec) EMB_GRAD_AS(float, L_, PER_, true);      \
  else EMB_GRAD_AS(float, L_, PER_, false)
  EMB_STAGE_BY_WIDTH(EMB_GRAD, C);
#undef EMB_GRAD
#undef EMB_GRAD_AS
  hipError_t status = g_count.launched();
  if (status != hipSuccess || !params) return status;
  const dim3 rgrid(static_cast<unsigned>((C + kReduceCols - 1) / kReduceCols), 2);
  hipLaunchKernelGGL(norm_act_reduce_kernel, rgrid, dim3(kBlock), 0, stream, part, dscale, dshift,
                     static_cast<int32_t>(grid.x), u);
  return g_count.launched();
}

}  // namespace

int64_t conv_stage_launches() { return g_count.value(); }

hipError_t launch_pool_norm_act(const void* x, const float* scale, const float* shift, bool bf16, int64_t images,
                                int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                                hipStream_t stream) {
  return forward<true>(x, scale, shift, bf16, images, H, W, C, impl, act, eps, out, stream);
}

hipError_t launch_pool_norm_act_grad(const void* x, const float* scale, const float* shift, const void* gout, bool bf16,
                                     int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act,
                                     float eps, void* dx, float* dscale, float* dshift, float* partials,
                                     hipStream_t stream) {
  return backward<true>(x, scale, shift, gout, bf16, images, H, W, C, impl, act, eps, dx, dscale, dshift, partials,
                        stream);
}

hipError_t launch_norm_act_upsample(const void* x, const float* scale, const float* shift, bool bf16, int64_t images,
                                    int64_t H, int64_t W, int64_t C, int32_t impl, int32_t act, float eps, void* out,
                                    hipStream_t stream) {
  return forward<false>(x, scale, shift, bf16, images, H, W, C, impl, act, eps, out, stream);
}

hipError_t launch_norm_act_upsample_grad(const void* x, const float* scale, const float* shift, const void* gout,
                                         bool bf16, int64_t images, int64_t H, int64_t W, int64_t C, int32_t impl,
                                         int32_t act, float eps, void* dx, float* dscale, float* dshift,
                                         float* partials, hipStream_t stream) {
  return backward<false>(x, scale, shift, gout, bf16, images, H, W, C, impl, act, eps, dx, dscale, dshift, partials,
                         stream);
}

}  // namespace emb
