// Norm followed by the activation (embodied/jax/nets.py:361-399, nets.py:26-39):
// what follows every Linear, BlockLinear and Conv2D of DreamerV3's networks and,
// inside the recurrence, runs four times per RSSM._core (dreamerv3/rssm.py:141-151).
//   forward  one launch, x read once: a row stays in registers between its
//            reduction and its output
//   grad     one launch that recomputes everything from x and writes dx; with
//            parameter gradients every workgroup also leaves the column sums of
//            its rows, and a second launch adds those in a fixed order
// With torch ops the forward alone is a chain of about eight launches.
//
// A row belongs to TPR threads, each holding PER of its values: one wave64 up to
// 1024 units (4 rows per workgroup, butterflies of wave_util.h and nothing
// else), a workgroup of 256 up to 8192 (the waves' sums meet in LDS, added in the
// order of the waves).  Up to 16 384 the forward takes a workgroup of 1024, 16
// values per thread; the gradient there keeps nothing: a workgroup of 256 passes
// three times over its row (statistics, sums, dx), the second and third time out
// of the cache.  Loads and stores are 16 bytes
// (4 float32, 8 bfloat16) where `units` is a multiple of that and every pointer is
// aligned, and element by element otherwise.  No atomics: the same bits run to run.
#include "norm_act.h"
#include "wave_util.h"
// the thread map of a row, its statistics, the activation and the reduce launch
// (shared with conv_stage.hip); float32 operations one by one from there on
#include "norm_act_device.h"

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                       // threads of a workgroup unless one row takes more
constexpr int kMaxBlocks = 2048;                  // of the forward launch; more rows: grid stride

static_assert(kWave == kLanes, "the segment helpers shuffle over one wave64");
static_assert(kBlock == kReduceBlock, "the reduce launch below is a workgroup of kBlock");

// Two sums over the TPR threads of a row at once; every thread ends with the same
// bits.  One wave: butterflies.  More: each wave's butterfly, then the waves'
// results from LDS in the order of the waves (the row is the whole workgroup's,
// so every thread reaches the barriers).
template <int TPR>
__device__ __forceinline__ void row_sum2(float& a, float& b, float* lds) {
  a = seg_sum<kWave>(a);
  b = seg_sum<kWave>(b);
  if constexpr (TPR > kWave) {
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
      lds[2 * wave] = a;
      lds[2 * wave + 1] = b;
    }
    __syncthreads();
    a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < TPR / kWave; ++w) {
      a = a + lds[2 * w];
      b = b + lds[2 * w + 1];
    }
    __syncthreads();
  }
}

template <typename T, int TPR, int PER, bool VEC>
__global__ __launch_bounds__(TPR > kBlock ? TPR : kBlock) void norm_act_kernel(
    const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, T* __restrict__ out,
    int32_t rows, int32_t units, int32_t impl, int32_t act, float eps) {
  using M = Map<T, TPR, PER, VEC>;
  constexpr int kThreads = TPR > kBlock ? TPR : kBlock, kRows = kThreads / TPR;
  __shared__ float lds[2 * (TPR / kWave)];
  const int t = threadIdx.x % TPR, sub = threadIdx.x / TPR;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kRows + sub; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kRows) {           // uniform over the row's threads
    float v[PER];
    M::load(x + row * units, units, t, 0.f, v);
    float sum = 0.f, sum2 = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      sum = sum + v[j];
      sum2 = sum2 + v[j] * v[j];
    }
    row_sum2<TPR>(sum, sum2, lds);
    const Stats s = stats_of(sum, sum2, units, impl, eps);
#pragma unroll
    for (int c = 0; c < PER / M::E; ++c) {                         // the parameters a part at a time: they stay in cache
      float g[M::E], b[M::E];
      M::load_part(scale, units, t, c, 1.f, g);
      M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
      for (int k = 0; k < M::E; ++k) {
        const int j = c * M::E + k;
        const float y = impl == kNormLayer ? (v[j] - s.mean) * (s.rstd * g[k]) + b[k]      // nets.py:395
                                           : v[j] * (s.rstd * g[k]);                        // nets.py:386
        v[j] = activate(y, act);
      }
      __builtin_amdgcn_sched_barrier(0);                           // a part at a time: its temporaries do not pile up
    }
    M::store(out + row * units, units, t, v);
  }
}

// With xc = x - mean (x for rms), r = rstd, y = xc (r scale) + shift, dy = gout act'(y),
// h = dy scale, N = units and k the slope of max(0, .):
//   dscale_i = sum_rows dy_i xc_i r        dshift_i = sum_rows dy_i
//   rms      dx_i = r h_i - xc_i (r^3 / N) sum_j h_j xc_j
//   layer    dx_i = r (h_i - sum_j h_j / N) - xc_i (k r^3 / N) sum_j h_j xc_j
// (the one-pass variance mean(x^2) - mean^2 has the gradient 2 xc_i / N, as the two-pass one).
//
// The column sums of a workgroup's rows: where a wave takes a row (4 rows per
// workgroup) each wave adds in registers and the four meet in LDS, in the order
// of the waves, once; where the workgroup takes a row it adds every row's terms to
// its own row of `partials` in memory (the first row writes), each thread its own
// columns, so the registers hold the row and nothing else.
template <typename T, int TPR, int PER, bool VEC>
__global__ __launch_bounds__(kBlock) void norm_act_grad_kernel(
    const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const T* __restrict__ gout, T* __restrict__ dx, float* partials, int32_t rows, int32_t units, int32_t impl,
    int32_t act, float eps) {
  using M = Map<T, TPR, PER, VEC>;
  static_assert(TPR <= kBlock, "wider rows: norm_act_grad_wide_kernel");
  constexpr int kRows = kBlock / TPR;
  constexpr int kHeld = kRows > 1 ? PER : 1;                       // column sums in registers: the wave kernels only
  __shared__ float lds[2 * (TPR / kWave)];
  __shared__ float meet[kRows > 1 ? (kRows - 1) * PER * TPR : 1];
  const int t = threadIdx.x % TPR, sub = threadIdx.x / TPR;
  const float n = static_cast<float>(units);
  const int64_t part = static_cast<int64_t>(gridDim.x) * units;
  float* const my_scale = partials ? partials + static_cast<int64_t>(blockIdx.x) * units : nullptr;
  float* const my_shift = partials ? my_scale + part : nullptr;
  float dscale[kHeld], dshift[kHeld];
#pragma unroll
  for (int j = 0; j < kHeld; ++j) dscale[j] = 0.f, dshift[j] = 0.f;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kRows + sub; row < rows;
       row += static_cast<int64_t>(gridDim.x) * kRows) {           // uniform over the row's threads
    float v[PER], h[PER];
    M::load(x + row * units, units, t, 0.f, v);
    float sum = 0.f, sum2 = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      sum = sum + v[j];
      sum2 = sum2 + v[j] * v[j];
    }
    row_sum2<TPR>(sum, sum2, lds);
    const Stats s = stats_of(sum, sum2, units, impl, eps);
    M::load(gout + row * units, units, t, 0.f, h);
    const bool first = row == blockIdx.x;                          // kRows == 1: the workgroup's first row
    float sum_h = 0.f, sum_hx = 0.f;
#pragma unroll
    for (int c = 0; c < PER / M::E; ++c) {                         // the parameters a part at a time: they stay in cache
      float g[M::E], b[M::E], of_scale[M::E], of_shift[M::E];
      M::load_part(scale, units, t, c, 1.f, g);
      M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
      for (int k = 0; k < M::E; ++k) {
        const int j = c * M::E + k;
        const bool live = M::index(j, t) < units;
        const float xc = impl == kNormLayer ? v[j] - s.mean : v[j];
        const float y = impl == kNormLayer ? xc * (s.rstd * g[k]) + b[k] : xc * (s.rstd * g[k]);
        const float dy = live ? h[j] * activate_slope(y, act) : 0.f;
        of_scale[k] = dy * (xc * s.rstd);
        of_shift[k] = dy;
        h[j] = dy * g[k];
        v[j] = live ? xc : 0.f;
        sum_h = sum_h + h[j];
        sum_hx = sum_hx + h[j] * v[j];
      }
      if constexpr (kRows > 1) {
#pragma unroll
        for (int k = 0; k < M::E; ++k) {
          dscale[c * M::E + k] = dscale[c * M::E + k] + of_scale[k];
          dshift[c * M::E + k] = dshift[c * M::E + k] + of_shift[k];
        }
      } else if (partials) {
        float so_far[M::E];
        M::load_part(first ? nullptr : my_scale, units, t, c, 0.f, so_far);
#pragma unroll
        for (int k = 0; k < M::E; ++k) so_far[k] = so_far[k] + of_scale[k];
        M::store_part(my_scale, units, t, c, so_far);
        M::load_part(first ? nullptr : my_shift, units, t, c, 0.f, so_far);
#pragma unroll
        for (int k = 0; k < M::E; ++k) so_far[k] = so_far[k] + of_shift[k];
        M::store_part(my_shift, units, t, c, so_far);
      }
      __builtin_amdgcn_sched_barrier(0);                           // a part at a time: its temporaries do not pile up
    }
    row_sum2<TPR>(sum_h, sum_hx, lds);
    if (dx) {
      const float r3 = s.rstd * s.rstd * s.rstd;
      const float pull = impl == kNormLayer ? (s.slope * r3) * sum_hx / n : r3 * sum_hx / n;
      const float centre = impl == kNormLayer ? sum_h / n : 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) v[j] = s.rstd * (h[j] - centre) - v[j] * pull;
      M::store(dx + row * units, units, t, v);
    }
  }
  if constexpr (kRows > 1) {
    if (!partials) return;                                         // uniform over the launch
    // each wave's sums, added in the order of the waves
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      float (&mine)[kHeld] = which ? dshift : dscale;
      if (sub > 0) {
#pragma unroll
        for (int j = 0; j < PER; ++j) meet[((sub - 1) * PER + j) * TPR + t] = mine[j];
      }
      __syncthreads();
      if (sub == 0) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
#pragma unroll
          for (int w = 0; w < kRows - 1; ++w) mine[j] = mine[j] + meet[(w * PER + j) * TPR + t];
        }
        M::store(which ? my_shift : my_scale, units, t, mine);
      }
      __syncthreads();
    }
  }
}

// The gradient of a row wider than kHeldUnits: the same arithmetic in the same
// order per thread, but nothing is held between the passes -- the statistics from
// a first read of x, the two sums and the column sums from a second read of x and
// gout, dx from a third (a row is at most 64 KiB of x: the cache has it).  The
// column sums go to the workgroup's own row of `partials` as above.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void norm_act_grad_wide_kernel(
    const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const T* __restrict__ gout, T* __restrict__ dx, float* partials, int32_t rows, int32_t units, int32_t impl,
    int32_t act, float eps) {
  constexpr int E = 16 / sizeof(T);
  using M = Map<T, kBlock, E, VEC>;                                // one chunk at a time, the chunk index at run time
  __shared__ float lds[2 * (kBlock / kWave)];
  const int t = threadIdx.x;
  const int chunks = (units + kBlock * E - 1) / (kBlock * E);
  const float n = static_cast<float>(units);
  const int64_t part = static_cast<int64_t>(gridDim.x) * units;
  float* const my_scale = partials ? partials + static_cast<int64_t>(blockIdx.x) * units : nullptr;
  float* const my_shift = partials ? my_scale + part : nullptr;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * units;
    const T* gr = gout + row * units;
    float sum = 0.f, sum2 = 0.f;
    for (int c = 0; c < chunks; ++c) {
      float v[E];
      M::load_part(xr, units, t, c, 0.f, v);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        sum = sum + v[k];
        sum2 = sum2 + v[k] * v[k];
      }
    }
    row_sum2<kBlock>(sum, sum2, lds);
    const Stats s = stats_of(sum, sum2, units, impl, eps);
    const bool first = row == blockIdx.x;
    float sum_h = 0.f, sum_hx = 0.f;
    for (int c = 0; c < chunks; ++c) {
      float v[E], h[E], g[E], b[E], of_scale[E], of_shift[E];
      M::load_part(xr, units, t, c, 0.f, v);
      M::load_part(gr, units, t, c, 0.f, h);
      M::load_part(scale, units, t, c, 1.f, g);
      M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const bool live = (c * kBlock + t) * E + k < units;
        const float xc = impl == kNormLayer ? v[k] - s.mean : v[k];
        const float y = impl == kNormLayer ? xc * (s.rstd * g[k]) + b[k] : xc * (s.rstd * g[k]);
        const float dy = live ? h[k] * activate_slope(y, act) : 0.f;
        of_scale[k] = dy * (xc * s.rstd);
        of_shift[k] = dy;
        const float hk = dy * g[k];
        sum_h = sum_h + hk;
        sum_hx = sum_hx + hk * (live ? xc : 0.f);
      }
      if (partials) {
        float so_far[E];
        M::load_part(first ? nullptr : my_scale, units, t, c, 0.f, so_far);
#pragma unroll
        for (int k = 0; k < E; ++k) so_far[k] = so_far[k] + of_scale[k];
        M::store_part(my_scale, units, t, c, so_far);
        M::load_part(first ? nullptr : my_shift, units, t, c, 0.f, so_far);
#pragma unroll
        for (int k = 0; k < E; ++k) so_far[k] = so_far[k] + of_shift[k];
        M::store_part(my_shift, units, t, c, so_far);
      }
    }
    row_sum2<kBlock>(sum_h, sum_hx, lds);
    if (!dx) continue;                                             // uniform over the launch
    const float r3 = s.rstd * s.rstd * s.rstd;
    const float pull = impl == kNormLayer ? (s.slope * r3) * sum_hx / n : r3 * sum_hx / n;
    const float centre = impl == kNormLayer ? sum_h / n : 0.f;
    for (int c = 0; c < chunks; ++c) {
      float v[E], h[E], g[E], b[E];
      M::load_part(xr, units, t, c, 0.f, v);
      M::load_part(gr, units, t, c, 0.f, h);
      M::load_part(scale, units, t, c, 1.f, g);
      M::load_part(impl == kNormLayer ? shift : nullptr, units, t, c, 0.f, b);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float xc = impl == kNormLayer ? v[k] - s.mean : v[k];
        const float y = impl == kNormLayer ? xc * (s.rstd * g[k]) + b[k] : xc * (s.rstd * g[k]);
        const float hk = (h[k] * activate_slope(y, act)) * g[k];
        v[k] = s.rstd * (hk - centre) - xc * pull;
      }
      M::store_part(dx + row * units, units, t, c, v);
    }
  }
}

LaunchCount g_count;

bool fits(int64_t rows, int64_t units, int32_t impl, int32_t act) {
  return rows >= 1 && units >= 1 && units <= kNormActMaxUnits && rows <= INT32_MAX / units &&
         (impl == kNormRms || impl == kNormLayer) && act >= kActNone && act <= kActRelu;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// threads per row and values per thread by the row's width
#define EMB_NORM_BY_WIDTH(CALL, u)            \
  do {                                        \
    if ((u) <= 512) { CALL(64, 8); }          \
    else if ((u) <= 1024) { CALL(64, 16); }   \
    else if ((u) <= 2048) { CALL(256, 8); }   \
    else if ((u) <= 4096) { CALL(256, 16); }  \
    else if ((u) <= 8192) { CALL(256, 32); }  \
    else { CALL(1024, 16); }                  \
  } while (0)
static_assert(kNormActWaveUnits == 64 * 16 && kNormActMaxUnits == 1024 * 16, "the ladder above");
constexpr int kHeldUnits = 256 * 32;              // wider rows: the gradient kernel that holds nothing

// ... and of the rows a workgroup holds in registers (the gradient)
#define EMB_NORM_HELD_BY_WIDTH(CALL, u)       \
  do {                                        \
    if ((u) <= 512) { CALL(64, 8); }          \
    else if ((u) <= 1024) { CALL(64, 16); }   \
    else if ((u) <= 2048) { CALL(256, 8); }   \
    else if ((u) <= 4096) { CALL(256, 16); }  \
    else { CALL(256, 32); }                   \
  } while (0)

int threads_of(int64_t units) { return units <= kHeldUnits ? kBlock : 1024; }      // of the forward launch
int rows_per_block(int64_t units) { return units <= kNormActWaveUnits ? kBlock / kWave : 1; }

}  // namespace

int64_t norm_act_launches() { return g_count.value(); }

hipError_t launch_norm_act(const void* x, const float* scale, const float* shift, bool bf16, int64_t rows,
                           int64_t units, int32_t impl, int32_t act, float eps, void* out, hipStream_t stream) {
  if (!fits(rows, units, impl, act) || !x || !out) return hipErrorInvalidValue;
  const int64_t per = rows_per_block(units), blocks = (rows + per - 1) / per;
  const dim3 grid(static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(threads_of(units));
  const int32_t r = static_cast<int32_t>(rows), u = static_cast<int32_t>(units);
  const bool vec = units % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(out) && aligned16(scale) && aligned16(shift);
#define EMB_FORWARD_AS(T_, TPR_, PER_, VEC_)                                                                    \
  hipLaunchKernelGGL((norm_act_kernel<T_, TPR_, PER_, VEC_>), grid, block, 0, stream, static_cast<const T_*>(x), \
                     scale, shift, static_cast<T_*>(out), r, u, impl, act, eps)
#define EMB_FORWARD(TPR_, PER_)                         \
  if (bf16 && vec) EMB_FORWARD_AS(bf16_t, TPR_, PER_, true);   \
  else if (bf16) EMB_FORWARD_AS(bf16_t, TPR_, PER_, false);    \
  else if (vec) EMB_FORWARD_AS(float, TPR_, PER_, true);       \
  else EMB_FORWARD_AS(float, TPR_, PER_, false)
  EMB_NORM_BY_WIDTH(EMB_FORWARD, units);
#undef EMB_FORWARD
#undef EMB_FORWARD_AS
  return g_count.launched();
}

hipError_t launch_norm_act_grad(const void* x, const float* scale, const float* shift, const void* gout, bool bf16,
                                int64_t rows, int64_t units, int32_t impl, int32_t act, float eps, void* dx,
                                float* dscale, float* dshift, float* partials, hipStream_t stream) {
  if (!fits(rows, units, impl, act) || !x || !gout) return hipErrorInvalidValue;
  if (!dx && !dscale && !dshift) return hipErrorInvalidValue;
  const bool params = dscale || dshift;
  if (params && !partials) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(norm_act_partials(rows, units))), block(kBlock);
  const int32_t r = static_cast<int32_t>(rows), u = static_cast<int32_t>(units);
  float* part = params ? partials : nullptr;
  const bool vec = units % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(gout) && aligned16(dx) &&
                   aligned16(scale) && aligned16(shift) && aligned16(part);
#define EMB_GRAD_AS(T_, TPR_, PER_, VEC_)                                                                            \
  hipLaunchKernelGGL((norm_act_grad_kernel<T_, TPR_, PER_, VEC_>), grid, block, 0, stream, static_cast<const T_*>(x), \
                     scale, shift, static_cast<const T_*>(gout), static_cast<T_*>(dx), part, r, u, impl, act, eps)
#define EMB_GRAD(TPR_, PER_)                               \
  if (bf16 && vec) EMB_GRAD_AS(bf16_t, TPR_, PER_, true);  \
  else if (bf16) EMB_GRAD_AS(bf16_t, TPR_, PER_, false);   \
  else if (vec) EMB_GRAD_AS(float, TPR_, PER_, true);      \
  else EMB_GRAD_AS(float, TPR_, PER_, false)
#define EMB_GRAD_WIDE(T_, VEC_)                                                                                      \
  hipLaunchKernelGGL((norm_act_grad_wide_kernel<T_, VEC_>), grid, block, 0, stream, static_cast<const T_*>(x), scale, \
                     shift, static_cast<const T_*>(gout), static_cast<T_*>(dx), part, r, u, impl, act, eps)
  if (units > kHeldUnits) {
    if (bf16 && vec) EMB_GRAD_WIDE(bf16_t, true);
    else if (bf16) EMB_GRAD_WIDE(bf16_t, false);
    else if (vec) EMB_GRAD_WIDE(float, true);
    else EMB_GRAD_WIDE(float, false);
  } else {
    EMB_NORM_HELD_BY_WIDTH(EMB_GRAD, units);
  }
#undef EMB_GRAD_WIDE
#undef EMB_GRAD
#undef EMB_GRAD_AS
  hipError_t status = g_count.launched();
  if (status != hipSuccess || !params) return status;
  const dim3 rgrid(static_cast<unsigned>((units + kReduceCols - 1) / kReduceCols), 2);
  hipLaunchKernelGGL(norm_act_reduce_kernel, rgrid, dim3(kBlock), 0, stream, part, dscale, dshift,
                     static_cast<int32_t>(grid.x), u);
  return g_count.launched();
}

}  // namespace emb
