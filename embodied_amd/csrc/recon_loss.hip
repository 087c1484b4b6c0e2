// The three terms of DreamerV3's world-model loss that are sums of elementwise
// errors (dreamerv3/agent.py:170-182):
//   image   Agg(MSE(sigmoid(x)), 3, sum).loss(f32(frame) / 255)     (rssm.py:349, 353-356)
//   vector  Agg(MSE(x, symlog), 1, sum).loss(target)              (heads.py:127-130)
//   con     Binary(logit).loss(con)                               (outs.py:189-201)
// (embodied/jax/outs.py:40-58 Agg, 129-141 MSE) as one kernel family over
// (rows, units): one read of x and of the target forward -- the uint8 frame is
// widened and divided by 255 in registers -- and one more read of both plus one
// write backward.  With torch ops the same is a chain of full-size float32
// temporaries.
//
// Three geometries, chosen on the host by the row's width (recon_loss.h names
// the boundaries): W lanes per row for tiny rows, a wave per row, a workgroup
// per row.  Rows of at most 64 units are read and written one element per lane
// (consecutive lanes, consecutive elements; their gradient is a flat elementwise
// pass); what follows is the wave and the workgroup per row.  A lane works on
// LOGICAL chunks of V = 16 / sizeof(x) consecutive elements of its row -- chunk c
// of the row belongs to lane c % lanes -- and adds
// their terms in element order; the lanes are then summed by a butterfly and the
// waves in wave order.  So the order of the additions depends on (units, dtypes)
// alone, never on where the buffers start.  Each chunk is loaded in the widest
// pieces its address allows (the whole chunk, halves, ... single elements): a
// view that starts on an odd byte or half-word is read in narrower pieces, not
// past its ends, and gives the same bits.  No atomics, no traffic between
// workgroups: the same bits run to run.
#include "recon_loss.h"
#include "wave_util.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // waves per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups of 4 waves on each of 256 CUs; more rows: grid stride

using segment::bf16_t;
using segment::quiet_nan;
using segment::wave_sum;
using segment::widen;                             // the bf16 arm; float and uint8 here
static_assert(kWave == segment::kLanes, "the wave helpers shuffle over one wave64");

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(uint8_t v) { return static_cast<float>(v); }

__device__ __forceinline__ void narrow(float& out, float v) { out = v; }
__device__ __forceinline__ void narrow(bf16_t& out, float v) { out = segment::bf16_bits(v); }

// N elements that sit on a multiple of their own size: one load or store.
template <typename E, int N>
struct alignas(sizeof(E) * N) Pack {
  E e[N];
};

// How many elements past `p` are known to share an aligned power-of-two block: the
// lowest set bit of the address counted in elements, at most 64.
template <typename E>
__device__ __forceinline__ int aligned_elements(const E* p) {
  const uint64_t e = (reinterpret_cast<uint64_t>(p) / sizeof(E)) | 64u;
  return static_cast<int>(e & (~e + 1));
}

template <typename E, int V, int A>
__device__ __forceinline__ void load_pieces(const E* p, float (&out)[V]) {
#pragma unroll
  for (int k = 0; k < V / A; ++k) {
    const Pack<E, A> piece = *reinterpret_cast<const Pack<E, A>*>(p + k * A);
#pragma unroll
    for (int i = 0; i < A; ++i) out[k * A + i] = widen(piece.e[i]);
  }
}

// out[0 .. V) = p[0 .. V) widened, read in pieces of min(V, a) elements; `a` is
// uniform over the row, the branches are scalar.
template <typename E, int V>
__device__ __forceinline__ void load_chunk(const E* p, int a, float (&out)[V]) {
  if (a >= V) {
    load_pieces<E, V, V>(p, out);
  } else if (V >= 4 && a >= V / 2) {
    load_pieces<E, V, (V >= 4 ? V / 2 : 1)>(p, out);
  } else if (V >= 8 && a >= V / 4) {
    load_pieces<E, V, (V >= 8 ? V / 4 : 1)>(p, out);
  } else {
    load_pieces<E, V, 1>(p, out);
  }
}

template <typename E, int V, int A>
__device__ __forceinline__ void store_pieces(E* p, const float (&in)[V]) {
#pragma unroll
  for (int k = 0; k < V / A; ++k) {
    Pack<E, A> piece;
#pragma unroll
    for (int i = 0; i < A; ++i) narrow(piece.e[i], in[k * A + i]);
    *reinterpret_cast<Pack<E, A>*>(p + k * A) = piece;
  }
}

template <typename E, int V>
__device__ __forceinline__ void store_chunk(E* p, int a, const float (&in)[V]) {
  if (a >= V) {
    store_pieces<E, V, V>(p, in);
  } else if (V >= 4 && a >= V / 2) {
    store_pieces<E, V, (V >= 4 ? V / 2 : 1)>(p, in);
  } else if (V >= 8 && a >= V / 4) {
    store_pieces<E, V, (V >= 8 ? V / 4 : 1)>(p, in);
  } else {
    store_pieces<E, V, 1>(p, in);
  }
}

// t of the raw target: the float32 division the reference writes (agent.py:181).
__device__ __forceinline__ float scaled(float raw, float div) { return div == 1.f ? raw : raw / div; }

__device__ __forceinline__ float symlog(float t) { return copysignf(log1pf(fabsf(t)), t); }      // nets.py symlog

// What the sigmoid ops share: diff = sigmoid(x) - t and slope = sigmoid(x) (1 - sigmoid(x)),
// formed so that nothing cancels.  |x| >= 1: from e = exp(-|x|), q = e / (1 + e) the
// sigmoid of -|x|, exact in relative terms however large |x| is.  |x| < 1: from
// h = sigmoid(x) - 1/2 = tanh(x / 2) / 2, so that sigmoid(x) near 1/2 is not rounded
// at 2^-25 before a target near 1/2 is taken from it (1/2 - t is exact for t in
// [1/4, 1]).
struct Sigmoid {
  float diff, slope;
};
__device__ __forceinline__ Sigmoid sigmoid_minus(float x, float t) {
  if (fabsf(x) < 1.f) {
    const float h = 0.5f * tanhf(0.5f * x);
    return {(0.5f - t) + h, 0.25f - h * h};
  }
  const float e = expf(-fabsf(x)), one = 1.f + e, q = e / one;
  return {x >= 0.f ? (1.f - t) - q : q - t, q / one};
}

// One element's term of the loss.  A NaN or infinite x: NaN.
__device__ __forceinline__ float term_of(int op, float x, float raw, float div) {
  if (!(fabsf(x) < INFINITY)) return quiet_nan();
  const float t = scaled(raw, div);
  switch (op) {
    case kReconMse: {
      const float d = x - t;
      return d * d;
    }
    case kReconMseSymlog: {
      const float d = x - symlog(t);
      return d * d;
    }
    case kReconSigmoidMse: {
      const float d = sigmoid_minus(x, t).diff;
      return d * d;
    }
    default: {                                                     // outs.py:197-201, Output.loss = -logp
      const float soft = log1pf(expf(-fabsf(x)));
      const float logp = fminf(x, 0.f) - soft, lognotp = fminf(-x, 0.f) - soft;
      return -(t * logp + (1.f - t) * lognotp);
    }
  }
}

// d term / d x, times the row's upstream gradient g.
__device__ __forceinline__ float slope_of(int op, float x, float raw, float div, float g) {
  if (!(fabsf(x) < INFINITY)) return quiet_nan();
  const float t = scaled(raw, div);
  switch (op) {
    case kReconMse:
      return (2.f * (x - t)) * g;
    case kReconMseSymlog:
      return (2.f * (x - symlog(t))) * g;
    case kReconSigmoidMse: {
      const Sigmoid s = sigmoid_minus(x, t);
      return ((2.f * s.diff) * s.slope) * g;
    }
    default:
      return sigmoid_minus(x, t).diff * g;
  }
}

// ---- tiny rows: W lanes per row, 64 / W rows per wave ------------------------------

template <typename TX, typename TT>
__global__ __launch_bounds__(kThreads) void recon_segment_kernel(const TX* __restrict__ x, const TT* __restrict__ target,
                                                                 float* __restrict__ loss, int64_t rows, int32_t units,
                                                                 int32_t width, int32_t op, float div) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int sl = lane % width, seg = lane / width, segs = kWave / width;
  const int64_t passes = (rows + segs - 1) / segs;
  for (int64_t pass = static_cast<int64_t>(blockIdx.x) * kWaves + wave; pass < passes;
       pass += static_cast<int64_t>(gridDim.x) * kWaves) {         // uniform over the wave: the shuffles see 64 lanes
    const int64_t row = pass * segs + seg;
    const bool live = row < rows && sl < units;
    float v = 0.f;
    if (live) {
      const int64_t at = row * units + sl;
      v = term_of(op, widen(x[at]), widen(target[at]), div);
    }
    for (int o = width / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kWave);
    if (live && sl == 0) loss[row] = v;
  }
}

template <typename TX, typename TT>
__global__ __launch_bounds__(kThreads) void recon_flat_grad_kernel(const TX* __restrict__ x, const TT* __restrict__ target,
                                                                   const float* __restrict__ gout, TX* __restrict__ grad,
                                                                   int64_t count, int32_t units, int32_t op, float div) {
  for (int64_t at = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; at < count;
       at += static_cast<int64_t>(gridDim.x) * kThreads)
    narrow(grad[at], slope_of(op, widen(x[at]), widen(target[at]), div, gout[at / units]));
}

// ---- a wave or a workgroup per row ------------------------------------------------

// BLOCK: the workgroup's 256 threads on one row; otherwise each wave on its own.
template <typename TX, typename TT, bool BLOCK>
__global__ __launch_bounds__(kThreads) void recon_row_kernel(const TX* __restrict__ x, const TT* __restrict__ target,
                                                             float* __restrict__ loss, int64_t rows, int32_t units,
                                                             int32_t op, float div) {
  constexpr int V = 16 / sizeof(TX);
  constexpr int kLanes = BLOCK ? kThreads : kWave;
  __shared__ float partial[kWaves];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int me = BLOCK ? static_cast<int>(threadIdx.x) : lane;
  const int chunks = units / V, rest = units % V;
  const int64_t first = BLOCK ? blockIdx.x : static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  const int64_t step = BLOCK ? gridDim.x : static_cast<int64_t>(gridDim.x) * kWaves;
  for (int64_t row = first; row < rows; row += step) {              // uniform over the wave (BLOCK: the workgroup)
    const TX* xr = x + row * units;
    const TT* tr = target + row * units;
    const int ax = aligned_elements(xr), at = aligned_elements(tr);
    float acc = 0.f;
    for (int c = me; c < chunks; c += kLanes) {
      float xv[V], tv[V];
      load_chunk<TX, V>(xr + c * V, ax, xv);
      load_chunk<TT, V>(tr + c * V, at, tv);
#pragma unroll
      for (int j = 0; j < V; ++j) acc = acc + term_of(op, xv[j], tv[j], div);
    }
    if (rest && me == chunks % kLanes)                              // the row's tail: the lane whose chunk it would be
      for (int j = chunks * V; j < units; ++j) acc = acc + term_of(op, widen(xr[j]), widen(tr[j]), div);
    acc = wave_sum(acc);
    if constexpr (BLOCK) {
      if (lane == 0) partial[wave] = acc;
      __syncthreads();
      if (threadIdx.x == 0) loss[row] = ((partial[0] + partial[1]) + partial[2]) + partial[3];
      __syncthreads();                                              // the next row writes `partial` again
    } else {
      if (lane == 0) loss[row] = acc;
    }
  }
}

template <typename TX, typename TT, bool BLOCK>
__global__ __launch_bounds__(kThreads) void recon_row_grad_kernel(const TX* __restrict__ x, const TT* __restrict__ target,
                                                                  const float* __restrict__ gout, TX* __restrict__ grad,
                                                                  int64_t rows, int32_t units, int32_t op, float div) {
  constexpr int V = 16 / sizeof(TX);
  constexpr int kLanes = BLOCK ? kThreads : kWave;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int me = BLOCK ? static_cast<int>(threadIdx.x) : lane;
  const int chunks = units / V, rest = units % V;
  const int64_t first = BLOCK ? blockIdx.x : static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  const int64_t step = BLOCK ? gridDim.x : static_cast<int64_t>(gridDim.x) * kWaves;
  for (int64_t row = first; row < rows; row += step) {
    const TX* xr = x + row * units;
    const TT* tr = target + row * units;
    TX* gr = grad + row * units;
    const int ax = aligned_elements(xr), at = aligned_elements(tr), ag = aligned_elements(gr);
    const float g = gout[row];
    for (int c = me; c < chunks; c += kLanes) {
      float xv[V], tv[V], out[V];
      load_chunk<TX, V>(xr + c * V, ax, xv);
      load_chunk<TT, V>(tr + c * V, at, tv);
#pragma unroll
      for (int j = 0; j < V; ++j) out[j] = slope_of(op, xv[j], tv[j], div, g);
      store_chunk<TX, V>(gr + c * V, ag, out);
    }
    if (rest && me == chunks % kLanes)
      for (int j = chunks * V; j < units; ++j) narrow(gr[j], slope_of(op, widen(xr[j]), widen(tr[j]), div, g));
  }
}

segment::LaunchCount g_count;

bool fits(int x_dtype, int target_dtype, int64_t rows, int64_t units, int op) {
  return (x_dtype == kReconF32 || x_dtype == kReconBf16) && target_dtype >= kReconF32 && target_dtype <= kReconU8 &&
         op >= kReconMse && op <= kReconBinary && rows >= 1 && units >= 1 && rows <= INT32_MAX / units;
}

unsigned capped(int64_t blocks) { return static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks); }

int segment_width(int64_t units) {
  int w = 1;
  while (w < units) w *= 2;
  return w;
}

// CALL(TX, TT) for the six (x, target) element types
#define EMB_RECON_BY_DTYPE(CALL, xd, td)                 \
  do {                                                   \
    if ((xd) == kReconF32) {                             \
      if ((td) == kReconF32) { CALL(float, float); }     \
      else if ((td) == kReconBf16) { CALL(float, bf16_t); } \
      else { CALL(float, uint8_t); }                     \
    } else {                                             \
      if ((td) == kReconF32) { CALL(bf16_t, float); }    \
      else if ((td) == kReconBf16) { CALL(bf16_t, bf16_t); } \
      else { CALL(bf16_t, uint8_t); }                    \
    }                                                    \
  } while (0)

}  // namespace

int64_t recon_loss_launches() { return g_count.value(); }

hipError_t launch_recon_loss(const void* x, int x_dtype, const void* target, int target_dtype, float div,
                             int64_t rows, int64_t units, int op, float* loss, hipStream_t stream) {
  if (!fits(x_dtype, target_dtype, rows, units, op) || !x || !target || !loss) return hipErrorInvalidValue;
  const dim3 block(kThreads);
  const int32_t u = static_cast<int32_t>(units);
  if (units <= kReconSegmentMaxUnits) {
    const int32_t width = segment_width(units);
    const int64_t segs = kWave / width, passes = (rows + segs - 1) / segs;
    const dim3 grid(capped((passes + kWaves - 1) / kWaves));
#define EMB_SEGMENT(TX_, TT_)                                                                         \
  hipLaunchKernelGGL((recon_segment_kernel<TX_, TT_>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), loss, rows, u, width, op, div)
    EMB_RECON_BY_DTYPE(EMB_SEGMENT, x_dtype, target_dtype);
#undef EMB_SEGMENT
  } else if (units <= kReconWaveMaxUnits) {
    const dim3 grid(capped((rows + kWaves - 1) / kWaves));
#define EMB_WAVE(TX_, TT_)                                                                               \
  hipLaunchKernelGGL((recon_row_kernel<TX_, TT_, false>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), loss, rows, u, op, div)
    EMB_RECON_BY_DTYPE(EMB_WAVE, x_dtype, target_dtype);
#undef EMB_WAVE
  } else {
    const dim3 grid(capped(rows));
#define EMB_BLOCK(TX_, TT_)                                                                             \
  hipLaunchKernelGGL((recon_row_kernel<TX_, TT_, true>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), loss, rows, u, op, div)
    EMB_RECON_BY_DTYPE(EMB_BLOCK, x_dtype, target_dtype);
#undef EMB_BLOCK
  }
  return g_count.launched();
}

hipError_t launch_recon_loss_grad(const void* x, int x_dtype, const void* target, int target_dtype, float div,
                                  int64_t rows, int64_t units, int op, const float* gout, void* grad,
                                  hipStream_t stream) {
  if (!fits(x_dtype, target_dtype, rows, units, op) || !x || !target || !gout || !grad) return hipErrorInvalidValue;
  const dim3 block(kThreads);
  const int32_t u = static_cast<int32_t>(units);
  if (units <= kReconSegmentMaxUnits) {
    const int64_t count = rows * units;
    const dim3 grid(capped((count + kThreads - 1) / kThreads));
#define EMB_FLAT(TX_, TT_)                                                                               \
  hipLaunchKernelGGL((recon_flat_grad_kernel<TX_, TT_>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), gout, static_cast<TX_*>(grad), count, u, op, div)
    EMB_RECON_BY_DTYPE(EMB_FLAT, x_dtype, target_dtype);
#undef EMB_FLAT
  } else if (units <= kReconWaveMaxUnits) {
    const dim3 grid(capped((rows + kWaves - 1) / kWaves));
#define EMB_WAVE(TX_, TT_)                                                                                    \
  hipLaunchKernelGGL((recon_row_grad_kernel<TX_, TT_, false>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), gout, static_cast<TX_*>(grad), rows, u, op, div)
    EMB_RECON_BY_DTYPE(EMB_WAVE, x_dtype, target_dtype);
#undef EMB_WAVE
  } else {
    const dim3 grid(capped(rows));
#define EMB_BLOCK(TX_, TT_)                                                                                  \
  hipLaunchKernelGGL((recon_row_grad_kernel<TX_, TT_, true>), grid, block, 0, stream, static_cast<const TX_*>(x), \
                     static_cast<const TT_*>(target), gout, static_cast<TX_*>(grad), rows, u, op, div)
    EMB_RECON_BY_DTYPE(EMB_BLOCK, x_dtype, target_dtype);
#undef EMB_BLOCK
  }
  return g_count.launched();
}

}  // namespace emb
