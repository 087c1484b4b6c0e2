// Many small independent reductions in one launch (stat_rows.h): the scalar
// book-keeping of a DreamerV3 train step that no other kernel covers --
//   dreamerv3/agent.py:424-442  the metrics of imag_loss: means, a std, an
//                               abs-mean, min / max / rate of the normalised return
//   dreamerv3/agent.py:239-240  loss/{k} = v.mean() and loss = sum(mean_k * scale_k)
// With torch ops these are 25 to 30 launches forward, each at the launch floor.
//
//   stat_rows   one workgroup per entry: mean, population std, abs-mean, min,
//               max and rate = count(|x'| >= 1) / n of x' = the entry under its
//               affine map, whose (offset, scale) is READ ON THE DEVICE (words
//               3-4 of a DeviceNormalize state never take a host round trip).
//               With `total` one more workgroup re-reduces every entry and adds
//               mean_k * weight_k left to right: it waits for no other workgroup,
//               so the bits do not depend on the order in which they finish.
//   mean_fill   the backward of those means: (g * scale_k) / n_k into K buffers.
//
// Sums are float64 per lane in element order, a wave butterfly, then the waves in
// their order (normalize_device.h is the precedent): no atomics, the same bits
// run to run.  A contiguous entry on a 16-byte boundary is read with 16-byte
// loads; any other entry with 4-byte loads, its rows walked by their stride.
#include "stat_rows.h"
#include "wave_util.h"

// float32 operations one by one, in the order written: min, max and the count
// agree bit for bit with a float32 restatement
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = kStatThreads / kWave;
constexpr int kFillThreads = 256;
constexpr int kFillMaxBlocks = 64;      // per entry; more elements: grid stride

struct Lane {
  double sum = 0.0, sq = 0.0, abs = 0.0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int32_t ones = 0, nans = 0;
};

struct Stats {
  float v[kStatValues];
};

struct Shared {
  double sums[kWaves][3];
  float lo[kWaves], hi[kWaves];
  int32_t ones[kWaves], nans[kWaves];
};

template <int MODE>
__device__ __forceinline__ float mapped(float x, float offset, float scale) {
  if constexpr (MODE == EMB_STAT_MUL_ADD) return x * scale + offset;
  else if constexpr (MODE == EMB_STAT_SUB_DIV) return (x - offset) / scale;      // a true division
  else return x;
}

// fminf / fmaxf drop a NaN: it is counted instead, and decides min and max at the end
__device__ __forceinline__ void take(Lane& a, float v) {
  const double d = v;
  a.sum += d;
  a.sq += d * d;
  a.abs += fabs(d);
  a.lo = fminf(a.lo, v);
  a.hi = fmaxf(a.hi, v);
  a.ones += fabsf(v) >= 1.0f ? 1 : 0;      // false for a NaN
  a.nans += v != v ? 1 : 0;
}

template <int MODE>
__device__ __forceinline__ void walk(const StatEntry& e, float offset, float scale, Lane& a) {
  const float* x = reinterpret_cast<const float*>(e.x);
  const int32_t tid = threadIdx.x;
  if (e.rows == 1) {
    const int32_t n = e.cols;
    if ((e.x & 15) == 0) {
      const int32_t nvec = n / kStatVector;
#pragma unroll 2
      for (int32_t v = tid; v < nvec; v += kStatThreads) {
        const float4 q = *reinterpret_cast<const float4*>(x + static_cast<int64_t>(v) * kStatVector);
        take(a, mapped<MODE>(q.x, offset, scale));
        take(a, mapped<MODE>(q.y, offset, scale));
        take(a, mapped<MODE>(q.z, offset, scale));
        take(a, mapped<MODE>(q.w, offset, scale));
      }
      for (int64_t i = static_cast<int64_t>(nvec) * kStatVector + tid; i < n; i += kStatThreads)
        take(a, mapped<MODE>(x[i], offset, scale));
    } else {
      for (int64_t i = tid; i < n; i += kStatThreads) take(a, mapped<MODE>(x[i], offset, scale));
    }
  } else {
    const uint32_t cols = static_cast<uint32_t>(e.cols);
    const int64_t n = static_cast<int64_t>(e.rows) * e.cols;      // <= 2^31 - 1 (stat_entry_error)
    for (int64_t i = tid; i < n; i += kStatThreads) {
      const uint32_t r = static_cast<uint32_t>(i) / cols, c = static_cast<uint32_t>(i) - r * cols;
      take(a, mapped<MODE>(x[static_cast<int64_t>(r) * e.stride + c], offset, scale));
    }
  }
}

// The six statistics of one entry, valid in thread 0.  Every thread of the
// workgroup calls it; the same entry gives the same bits in whichever workgroup.
__device__ __forceinline__ Stats reduce_entry(const StatEntry& e, Shared& lds) {
  Lane a;
  if (e.mode == EMB_STAT_NONE) {
    walk<EMB_STAT_NONE>(e, 0.f, 1.f, a);
  } else {
    const float* pair = reinterpret_cast<const float*>(e.affine);
    const float offset = pair[0], scale = pair[1];
    if (e.mode == EMB_STAT_MUL_ADD) walk<EMB_STAT_MUL_ADD>(e, offset, scale, a);
    else walk<EMB_STAT_SUB_DIV>(e, offset, scale, a);
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {      // a butterfly: a fixed order of additions
    a.sum += __shfl_xor(a.sum, m, kWave);
    a.sq += __shfl_xor(a.sq, m, kWave);
    a.abs += __shfl_xor(a.abs, m, kWave);
    a.lo = fminf(a.lo, __shfl_xor(a.lo, m, kWave));
    a.hi = fmaxf(a.hi, __shfl_xor(a.hi, m, kWave));
    a.ones += __shfl_xor(a.ones, m, kWave);
    a.nans += __shfl_xor(a.nans, m, kWave);
  }
  const int wave = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
    lds.sums[wave][0] = a.sum;
    lds.sums[wave][1] = a.sq;
    lds.sums[wave][2] = a.abs;
    lds.lo[wave] = a.lo;
    lds.hi[wave] = a.hi;
    lds.ones[wave] = a.ones;
    lds.nans[wave] = a.nans;
  }
  __syncthreads();
  Stats s{};
  if (threadIdx.x == 0) {
    Lane t;
    for (int w = 0; w < kWaves; ++w) {             // the waves in their order
      t.sum += lds.sums[w][0];
      t.sq += lds.sums[w][1];
      t.abs += lds.sums[w][2];
      t.lo = fminf(t.lo, lds.lo[w]);
      t.hi = fmaxf(t.hi, lds.hi[w]);
      t.ones += lds.ones[w];
      t.nans += lds.nans[w];
    }
    const double n = static_cast<double>(static_cast<int64_t>(e.rows) * e.cols);
    const double mean = t.sum / n;
    const double var = t.sq / n - mean * mean;
    const float nan = segment::quiet_nan();
    s.v[0] = static_cast<float>(mean);
    s.v[1] = static_cast<float>(var < 0.0 ? 0.0 : sqrt(var));      // a NaN stays one
    s.v[2] = static_cast<float>(t.abs / n);
    s.v[3] = t.nans ? nan : t.lo;                  // jnp.min / jnp.max return a NaN that is there
    s.v[4] = t.nans ? nan : t.hi;
    s.v[5] = static_cast<float>(t.ones) / static_cast<float>(n);
  }
  __syncthreads();                                 // the next call writes lds again
  return s;
}

__global__ __launch_bounds__(kStatThreads) void stat_rows_kernel(float* __restrict__ out, float* __restrict__ total,
                                                                 int32_t count, const StatTable table) {
  __shared__ Shared lds;
  if (blockIdx.x < static_cast<uint32_t>(count)) {
    const StatEntry e = table.e[blockIdx.x];
    const Stats s = reduce_entry(e, lds);
    if (threadIdx.x == 0) {
      float* row = out + static_cast<int64_t>(blockIdx.x) * kStatValues;
#pragma unroll
      for (int k = 0; k < kStatValues; ++k) row[k] = s.v[k];
    }
  } else {
    // The total's workgroup reduces every entry again: it reads no other
    // workgroup's result, and forms each mean with the same instructions.
    float sum = 0.f;                               // Python's sum() starts from 0 (agent.py:240)
    for (int32_t k = 0; k < count; ++k) {
      const StatEntry e = table.e[k];
      const Stats s = reduce_entry(e, lds);
      sum = sum + s.v[0] * e.weight;
    }
    if (threadIdx.x == 0) total[0] = sum;
  }
}

__global__ __launch_bounds__(kFillThreads) void mean_fill_kernel(const float* __restrict__ g, const FillTable table) {
  const emb_fill_entry_t e = table.e[blockIdx.y];
  const float value = (g[0] * e.scale) / static_cast<float>(e.n);
  float* out = static_cast<float*>(e.out);
  const int64_t n = e.n;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kFillThreads + threadIdx.x;
  const int64_t threads = static_cast<int64_t>(gridDim.x) * kFillThreads;
  // scalars up to the first 16-byte boundary, 16-byte stores, scalars behind the last one
  const int64_t head = min(static_cast<int64_t>(((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) / 4), n);
  const int64_t nvec = (n - head) / kStatVector;
  const int64_t tail = head + nvec * kStatVector;
  if (tid < head) out[tid] = value;
  const float4 four = make_float4(value, value, value, value);
  for (int64_t v = tid; v < nvec; v += threads) *reinterpret_cast<float4*>(out + head + v * kStatVector) = four;
  if (tid < n - tail) out[tail + tid] = value;
}

segment::LaunchCount g_count;

}  // namespace

int64_t stat_rows_launches() { return g_count.value(); }

hipError_t launch_stat_rows(const StatTable& table, int count, float* out, float* total, hipStream_t stream) {
  if (count < 1 || count > kStatMaxEntries || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stat_rows_kernel, dim3(count + (total ? 1 : 0)), dim3(kStatThreads), 0, stream, out, total,
                     static_cast<int32_t>(count), table);
  return g_count.launched();
}

hipError_t launch_mean_fill(const FillTable& table, int count, const float* g, hipStream_t stream) {
  if (count < 1 || count > kStatMaxEntries || !g) return hipErrorInvalidValue;
  int64_t most = 1;
  for (int k = 0; k < count; ++k) most = table.e[k].n > most ? table.e[k].n : most;
  const int64_t want = (most + kFillThreads * kStatVector - 1) / (kFillThreads * kStatVector);
  const int blocks = static_cast<int>(want < kFillMaxBlocks ? want : kFillMaxBlocks);
  hipLaunchKernelGGL(mean_fill_kernel, dim3(blocks, count), dim3(kFillThreads), 0, stream, g, table);
  return g_count.launched();
}

}  // namespace emb
