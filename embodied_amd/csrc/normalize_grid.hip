// The running return normaliser (normalize.hip) from kNormGridMin values on, over
// the whole chip: norm_grid_plan(n) workgroups of kNormGridThreads lanes, each on
// one contiguous tile of x for the whole call.  No workgroup ever waits for
// another -- no grid barrier, no flag, no cooperative launch: the phases are
// launches of their own, ordered by the stream.
//
//   meanstd  sums     grid   per-lane float64 (s, s2) as normalize.hip forms them, wave
//                            shuffles, one (s, s2) per workgroup to scratch
//            finish   1 wg   the partials added in index order, norm_step, norm_store
//   perc     hist<1>  grid   the tile's top 11 key bits histogrammed in LDS, the non-zero
//                            bins added to the global level-0 histogram (u32 atomics:
//                            integer sums commute, the result is the same bits every run)
//            hist<2>  grid   every workgroup scans level 0 for the four ranks k_lo,
//            hist<3>         k_lo + 1, k_hi, k_hi + 1 (one wave each), then histograms the
//                            next digit of the keys under each DISTINCT prefix: rows
//                            [4][bins] in LDS, added to level 1; the same again for level 2
//            finish   1 wg   the last digit, the four keys, a + (b - a) * frac, norm_step
//   out      out      grid   (x - (sub ? sub : offset)) / scale over the same tiles, from
//                            state words 3-4; with update = 0 it is the only launch: every
//                            workgroup forms (offset, scale) from words 0-2, which nobody
//                            writes then, and workgroup 0 stores words 3-4
//
// All four ranks are selected because a rank and its successor can lie on both
// sides of a digit boundary.  lo / hi are the bits of the one-workgroup kernel;
// the float64 sums of meanstd are associated differently from it (per tile, then
// in tile order), so mean / sqrs may differ from it in the last float32 bit --
// and are the same bits from run to run: no float atomics.
//
// Scratch: the library's own, one block per (device, stream), hipMalloc'ed on that
// stream's first large call and kept until the process ends: the partial sums and
// the three histogram levels (kScratchBytes).  The histograms are cleared at the
// head of every perc update, so a call that died half way cannot poison the next:
// by hipMemsetAsync, or, while the stream is being captured, by a small kernel (a
// memset node is not what a graph should replay).  A captured stream that has no
// block yet gets none (no allocation inside a capture): the caller then launches
// the one-workgroup kernel.
#include "normalize_device.h"   // (float32 operations one by one: fp contract off)
#include "norm_select.h"        // to_key, from_key, hist_add, kNormBins

#include <map>
#include <mutex>
#include <utility>

namespace emb {
namespace {

constexpr int kT = kNormGridThreads;
constexpr int kRanks = kNormGridRanks;
constexpr uint32_t kLowBins = 1024;                           // the last digit: 10 bits
// scratch, in 32-bit words: partial sums (double2 per workgroup), then the levels
constexpr uint32_t kPartialWords = kNormGridMax * 4;
constexpr uint32_t kHist0 = 0, kHist1 = kNormBins, kHist2 = kHist1 + kRanks * kNormBins;
constexpr uint32_t kHistWords = kHist2 + kRanks * kLowBins;
constexpr size_t kScratchBytes = (kPartialWords + kHistWords) * sizeof(uint32_t);
static_assert(kT == kRanks * kNormWave, "one wave per rank");
static_assert(kNormGridMax <= kT, "the finish stages one partial per lane");

struct Tile {
  uint32_t begin, end;
};
__device__ __forceinline__ Tile tile_of(uint32_t n, uint32_t tile) {
  const uint64_t begin = static_cast<uint64_t>(blockIdx.x) * tile;       // a multiple of 4
  const uint32_t b = begin < n ? static_cast<uint32_t>(begin) : n;
  return {b, n - b < tile ? n : b + tile};
}

// f(valid, value) for every value of the tile, in wave-uniform control flow;
// float4 loads where x is 16-byte aligned, the same values one by one where not.
template <typename F>
__device__ __forceinline__ void for_tile(const float* x, Tile t, F f) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? (t.end - t.begin) / 4 : 0;
  const float4* x4 = reinterpret_cast<const float4*>(x + t.begin);
  for (uint32_t base = 0; base < n4; base += kT) {
    const uint32_t i = base + tid;
    const bool valid = i < n4;
    const float4 v = valid ? x4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    f(valid, v.x);
    f(valid, v.y);
    f(valid, v.z);
    f(valid, v.w);
  }
  for (uint32_t base = t.begin + n4 * 4; base < t.end; base += kT) {
    const uint32_t i = base + tid;
    const bool valid = i < t.end;
    f(valid, valid ? x[i] : 0.f);
  }
}

// One wave: the bin of h[0 .. 64 * kPer) that holds the key of rank `want`, and
// that rank among the bin's keys.  Lane l owns bins [l * kPer, (l + 1) * kPer) in
// registers; every lane returns the same pair.  A rank past the histogram's
// total (never, with histograms of this call) gives the last bin: an index that
// is always in range.
struct Found {
  uint32_t bin, rest;
};
template <int kPer>
__device__ __forceinline__ Found wave_find(const uint32_t* h, uint32_t want) {
  const uint32_t lane = threadIdx.x % kNormWave;
  uint32_t c[kPer];
#pragma unroll
  for (int j = 0; j < kPer; j += 4) {
    const uint4 v = reinterpret_cast<const uint4*>(h)[(lane * kPer + j) / 4];
    c[j] = v.x, c[j + 1] = v.y, c[j + 2] = v.z, c[j + 3] = v.w;
  }
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) mine += c[j];
  uint32_t incl = mine;
  for (int o = 1; o < kNormWave; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o);
    if (static_cast<int>(lane) >= o) incl += up;
  }
  uint32_t below = incl - mine;
  const bool here = want >= below && want < incl;
  uint32_t bin = 64 * kPer - 1, rest = 0;
  bool found = false;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (here && !found && want < below + c[j]) bin = lane * kPer + j, rest = want - below, found = true;
    below += c[j];
  }
  const unsigned long long who = __ballot(found);
  const int from = who ? __ffsll(static_cast<long long>(who)) - 1 : 0;
  bin = __shfl(bin, from), rest = __shfl(rest, from);
  if (!who) bin = 64 * kPer - 1, rest = 0;
  return {bin, rest};
}

__device__ __forceinline__ uint32_t pick(uint4 v, uint32_t i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// The first rank that shares rank r's prefix: the histogram row both use.
__device__ __forceinline__ uint32_t row_of(const uint32_t* pre, uint32_t r) {
  uint32_t row = r;
  for (int q = kRanks - 1; q >= 0; --q)
    if (pre[q] == pre[r]) row = q;
  return row;
}

// Wave r resolves the first kLevels digits of rank r's key from the global
// histograms; on return pre[0 .. 4) (LDS) holds the four prefixes for every lane
// and *rest this wave's rank among the keys under its prefix.
template <int kLevels>
__device__ __forceinline__ void grid_resolve(const uint32_t* hists, uint4 ranks, uint32_t* pre, uint32_t* rest) {
  const uint32_t lane = threadIdx.x % kNormWave, wave = threadIdx.x / kNormWave;
  Found f = wave_find<kNormBins / kNormWave>(hists + kHist0, pick(ranks, wave));
  uint32_t prefix = f.bin << 21;
  if constexpr (kLevels >= 2) {
    if (lane == 0) pre[wave] = prefix;
    __syncthreads();
    const uint32_t row = row_of(pre, wave);
    __syncthreads();
    f = wave_find<kNormBins / kNormWave>(hists + kHist1 + row * kNormBins, f.rest);
    prefix |= f.bin << 10;
  }
  if constexpr (kLevels >= 3) {
    if (lane == 0) pre[wave] = prefix;
    __syncthreads();
    const uint32_t row = row_of(pre, wave);
    __syncthreads();
    f = wave_find<kLowBins / kNormWave>(hists + kHist2 + row * kLowBins, f.rest);
    prefix |= f.bin;
  }
  if (lane == 0) pre[wave] = prefix;
  __syncthreads();
  *rest = f.rest;
}

// Pass kPass of the select: digit kPass of the tile's keys (of those under one of
// the prefixes the earlier levels gave), LDS histogram, then the global one.
template <int kPass>
__global__ __launch_bounds__(kT) void norm_grid_hist_kernel(const float* x, uint32_t n, uint32_t tile,
                                                            uint32_t* hists, uint4 ranks) {
  constexpr int kRows = kPass == 1 ? 1 : kRanks;
  constexpr uint32_t kBins = kPass == 3 ? kLowBins : kNormBins;
  constexpr int kShift = kPass == 1 ? 21 : kPass == 2 ? 10 : 0;
  constexpr uint32_t kMask = kPass == 1 ? 0u : kPass == 2 ? 0xFFE00000u : 0xFFFFFC00u;
  constexpr uint32_t kLevel = kPass == 1 ? kHist0 : kPass == 2 ? kHist1 : kHist2;
  __shared__ uint32_t hist[kRows * kBins];
  __shared__ uint32_t pre[kRanks];
  const uint32_t tid = threadIdx.x;

  uint32_t prefix[kRows] = {};
  bool own[kRows] = {};
  if constexpr (kPass > 1) {
    uint32_t rest;
    grid_resolve<kPass - 1>(hists, ranks, pre, &rest);
#pragma unroll
    for (int r = 0; r < kRows; ++r) prefix[r] = pre[r], own[r] = row_of(pre, r) == static_cast<uint32_t>(r);
  }
  if constexpr (kPass == 1) own[0] = true;
#pragma unroll
  for (int r = 0; r < kRows; ++r)          // only the rows in use are zeroed, filled and added
    if (own[r])
      for (uint32_t i = tid; i < kBins; i += kT) hist[r * kBins + i] = 0;
  __syncthreads();
  for_tile(x, tile_of(n, tile), [&](bool valid, float v) {
    const uint32_t key = to_key(v), bin = (key >> kShift) & (kBins - 1);
    if constexpr (kPass == 1) {
      hist_add(hist, valid, bin);
    } else {
#pragma unroll
      for (int r = 0; r < kRows; ++r)
        if (own[r]) hist_add(hist + r * kBins, valid && (key & kMask) == prefix[r], bin);     // (own: workgroup-uniform)
    }
  });
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRows; ++r)
    if (own[r])
      for (uint32_t i = tid; i < kBins; i += kT) {
        const uint32_t count = hist[r * kBins + i];
        if (count) atomicAdd(&hists[kLevel + r * kBins + i], count);
      }
}

// The histograms' zeros where a memset may not be recorded (a captured stream).
__global__ __launch_bounds__(kT) void norm_grid_clear_kernel(uint4* hists) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i < kHistWords / 4) hists[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kT) void norm_grid_sums_kernel(const float* x, uint32_t n, uint32_t tile, double* partial) {
  __shared__ double waves[kT / kNormWave][2];
  const uint32_t tid = threadIdx.x;
  const Tile t = tile_of(n, tile);
  double s = 0.0, s2 = 0.0;
  const uint32_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? (t.end - t.begin) / 4 : 0;
  const float4* x4 = reinterpret_cast<const float4*>(x + t.begin);
  for (uint32_t i = tid; i < n4; i += kT) {
    const float4 v = x4[i];
    s += (static_cast<double>(v.x) + static_cast<double>(v.y)) + (static_cast<double>(v.z) + static_cast<double>(v.w));
    s2 += (static_cast<double>(v.x * v.x) + static_cast<double>(v.y * v.y)) +
          (static_cast<double>(v.z * v.z) + static_cast<double>(v.w * v.w));   // squares in float32, as jnp.square
  }
  for (uint32_t i = t.begin + n4 * 4 + tid; i < t.end; i += kT) {
    const float v = x[i];
    s += static_cast<double>(v);
    s2 += static_cast<double>(v * v);
  }
  for (int o = kNormWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o), s2 += __shfl_xor(s2, o);
  if (tid % kNormWave == 0) waves[tid / kNormWave][0] = s, waves[tid / kNormWave][1] = s2;
  __syncthreads();
  if (tid == 0) {
    s = 0.0, s2 = 0.0;
    for (int w = 0; w < kT / kNormWave; ++w) s += waves[w][0], s2 += waves[w][1];
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = s2;
  }
}

// One workgroup: the batch statistics from what the grid left in scratch, then
// the EMA step and the state words, by the device functions of normalize.hip.
__global__ __launch_bounds__(kT) void norm_grid_finish_kernel(
    const uint32_t* hists, const double* partial, float* state, uint32_t n, uint32_t groups, uint32_t flags,
    float keep, float rate, float limit, uint4 ranks, float frac_lo, float frac_hi) {
  __shared__ double sums[kNormGridMax][2];
  __shared__ uint32_t pre[kRanks];
  const uint32_t tid = threadIdx.x;
  const uint32_t impl = flags & 3u;
  const bool debias = flags & 8u;
  const float v0 = state[0], v1 = state[1], vc = state[2];
  float new0 = 0.f, new1 = 0.f;
  if (impl == kNormMeanStd) {
    if (tid < groups) sums[tid][0] = partial[2 * tid], sums[tid][1] = partial[2 * tid + 1];
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, s2 = 0.0;
      for (uint32_t g = 0; g < groups; ++g) s += sums[g][0], s2 += sums[g][1];     // index order: the same bits every run
      new0 = static_cast<float>(s / static_cast<double>(n));
      new1 = static_cast<float>(s2 / static_cast<double>(n));
    }
  } else {
    uint32_t rest;
    grid_resolve<3>(hists, ranks, pre, &rest);
    // statistic k + 1 is the same key while the run of equal keys lasts: then a, as norm_select2
    const float a0 = from_key(pre[0]), b0 = from_key(pre[1]);
    const float a1 = from_key(pre[2]), b1 = from_key(pre[3]);
    new0 = frac_lo == 0.f || pre[1] == pre[0] ? a0 : a0 + (b0 - a0) * frac_lo;
    new1 = frac_hi == 0.f || pre[3] == pre[2] ? a1 : a1 + (b1 - a1) * frac_hi;
  }
  if (tid == 0) {
    const NormWords w = norm_step(v0, v1, vc, new0, new1, impl, true, debias, NormParams{keep, rate, limit});
    norm_store(state, w, true, debias);
  }
}

__global__ __launch_bounds__(kT) void norm_grid_out_kernel(const float* x, const float* sub, float* out, float* state,
                                                           uint32_t n, uint32_t tile, uint32_t flags, float keep,
                                                           float rate, float limit) {
  const uint32_t tid = threadIdx.x;
  const bool update = flags & 4u, debias = flags & 8u;
  float offset, scale;
  if (update) {        // the finish kernel of this call left them
    offset = state[3], scale = state[4];
  } else {             // nobody writes words 0-2 in this call
    const NormWords w = norm_step(state[0], state[1], state[2], 0.f, 0.f, flags & 3u, false, debias,
                                  NormParams{keep, rate, limit});
    offset = w.offset, scale = w.scale;
    if (blockIdx.x == 0 && tid == 0) norm_store(state, w, false, debias);
  }
  const Tile t = tile_of(n, tile);       // out may be x: every element is read and written by the same lane
  const bool wide = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) |
                      reinterpret_cast<uintptr_t>(sub)) & 15) == 0;
  const uint32_t n4 = wide ? (t.end - t.begin) / 4 : 0;
  for (uint32_t i = tid; i < n4; i += kT) {
    const float4 v = reinterpret_cast<const float4*>(x + t.begin)[i];
    float4 s = make_float4(offset, offset, offset, offset);
    if (sub) s = reinterpret_cast<const float4*>(sub + t.begin)[i];
    reinterpret_cast<float4*>(out + t.begin)[i] =
        make_float4((v.x - s.x) / scale, (v.y - s.y) / scale, (v.z - s.z) / scale, (v.w - s.w) / scale);
  }
  for (uint32_t i = t.begin + n4 * 4 + tid; i < t.end; i += kT) out[i] = (x[i] - (sub ? sub[i] : offset)) / scale;
}

std::mutex g_mutex;
std::map<std::pair<int, hipStream_t>, uint32_t*> g_blocks;     // never freed: see the head of this file

}  // namespace

hipError_t launch_normalize_grid(const float* x, int64_t n, float* state, int impl, bool update,
                                 bool debias, float keep, float rate, float limit, NormRank lo, NormRank hi,
                                 const float* sub, float* out, hipStream_t stream, int64_t* launched, bool* taken) {
  *taken = false;
  int device = 0;
  hipError_t status = hipGetDevice(&device);
  if (status != hipSuccess) return status;
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  status = hipStreamIsCapturing(stream, &capture);
  if (status != hipSuccess) return status;
  const bool capturing = capture != hipStreamCaptureStatusNone;
  uint32_t* block = nullptr;
  {
    std::lock_guard<std::mutex> guard(g_mutex);
    uint32_t*& slot = g_blocks[{device, stream}];
    if (!slot) {
      if (capturing) return hipSuccess;                        // the caller's one-workgroup kernel
      status = hipMalloc(reinterpret_cast<void**>(&slot), kScratchBytes);
      if (status != hipSuccess) {
        slot = nullptr;
        return status;
      }
    }
    block = slot;
  }
  *taken = true;
  double* partial = reinterpret_cast<double*>(block);
  uint32_t* hists = block + kPartialWords;
  const NormGridPlan plan = norm_grid_plan(n);
  const uint32_t count = static_cast<uint32_t>(n), last = count - 1;
  const uint32_t flags = static_cast<uint32_t>(impl) | (update ? 4u : 0u) | (debias ? 8u : 0u);
  const uint4 ranks = make_uint4(lo.k, lo.k < last ? lo.k + 1 : last, hi.k, hi.k < last ? hi.k + 1 : last);
  const dim3 grid(plan.groups), one(1), threads(kT);
  auto counted = [&] {
    const hipError_t error = hipGetLastError();
    if (error == hipSuccess) ++*launched;
    return error;
  };
  if (update && impl == kNormPerc) {
    if (capturing) {
      hipLaunchKernelGGL(norm_grid_clear_kernel, dim3((kHistWords / 4 + kT - 1) / kT), threads, 0, stream,
                         reinterpret_cast<uint4*>(hists));
      if ((status = counted()) != hipSuccess) return status;
    } else if ((status = hipMemsetAsync(hists, 0, kHistWords * sizeof(uint32_t), stream)) != hipSuccess) {
      return status;
    }
    hipLaunchKernelGGL(norm_grid_hist_kernel<1>, grid, threads, 0, stream, x, count, plan.tile, hists, ranks);
    if ((status = counted()) != hipSuccess) return status;
    hipLaunchKernelGGL(norm_grid_hist_kernel<2>, grid, threads, 0, stream, x, count, plan.tile, hists, ranks);
    if ((status = counted()) != hipSuccess) return status;
    hipLaunchKernelGGL(norm_grid_hist_kernel<3>, grid, threads, 0, stream, x, count, plan.tile, hists, ranks);
    if ((status = counted()) != hipSuccess) return status;
  }
  if (update && impl == kNormMeanStd) {
    hipLaunchKernelGGL(norm_grid_sums_kernel, grid, threads, 0, stream, x, count, plan.tile, partial);
    if ((status = counted()) != hipSuccess) return status;
  }
  if (update) {
    hipLaunchKernelGGL(norm_grid_finish_kernel, one, threads, 0, stream, static_cast<const uint32_t*>(hists),
                       static_cast<const double*>(partial), state, count, plan.groups, flags, keep, rate, limit,
                       ranks, lo.frac, hi.frac);
    if ((status = counted()) != hipSuccess) return status;
  }
  if (out) {
    hipLaunchKernelGGL(norm_grid_out_kernel, grid, threads, 0, stream, x, sub, out, state, count, plan.tile, flags,
                       keep, rate, limit);
    if ((status = counted()) != hipSuccess) return status;
  }
  return hipSuccess;
}

}  // namespace emb
