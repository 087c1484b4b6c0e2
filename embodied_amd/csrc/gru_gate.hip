// The gate at the end of RSSM._core (dreamerv3/rssm.py:152-159): `dyngru`'s
// (rows, 3 * deter) output split by block into reset / cand / update, two
// sigmoids, a tanh and the convex update of deter.
//   forward  one launch; the split is index arithmetic, nothing is copied
//   grad     one launch that recomputes the gates from x and deter and writes dx
//            (all three thirds of every block) and ddeter
// With torch ops that is three strided copies and about ten elementwise launches
// forward, and twice as many backward.
//
// One thread takes E neighbouring j of one block: 16 bytes (4 float32, 8
// bfloat16) where h = deter / blocks is a multiple of that and every pointer is
// aligned, one element otherwise.  Every element index is below 2^31 (checked on
// the host), the grid is capped and strides.  Elementwise: a NaN or a saturated
// gate touches its own element alone.
#include "gru_gate.h"
#include "wave_util.h"

// float32 operations one by one, as twohot.hip
#pragma clang fp contract(off)

namespace emb {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups on each of 256 CUs; more elements: grid stride

using namespace segment;

// E elements of T at p: one 16-byte access (E = 16 / sizeof(T)) or one element (E = 1)
template <int E>
__device__ __forceinline__ void load_n(const float* p, float (&v)[E]) {
  if constexpr (E == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}
template <int E>
__device__ __forceinline__ void load_n(const bf16_t* p, float (&v)[E]) {
  if constexpr (E == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __uint_as_float(w[k] << 16);
      v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
  } else {
    v[0] = load(p, 0);
  }
}
template <int E>
__device__ __forceinline__ void store_n(float* p, const float (&v)[E]) {
  if constexpr (E == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}
template <int E>
__device__ __forceinline__ void store_n(bf16_t* p, const float (&v)[E]) {
  if constexpr (E == 8) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = bf16_bits(v[2 * k]) | (static_cast<uint32_t>(bf16_bits(v[2 * k + 1])) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    store(p, 0, v[0]);
  }
}

// Where item i (E outputs) sits: `at` in deter / out, `gate` in x (its reset; cand
// and update are h and 2h further), rssm.py:153-154.  All below 2^31.
struct Place {
  uint32_t at, gate;
};
template <int E>
__device__ __forceinline__ Place place(int64_t item, uint32_t width, uint32_t h) {
  const uint32_t at = static_cast<uint32_t>(item) * E;
  const uint32_t row = at / width, col = at - row * width;
  const uint32_t k = col / h, j = col - k * h;
  return {at, row * (3u * width) + 3u * h * k + j};
}

template <typename T, int E>
__global__ __launch_bounds__(kThreads) void gru_gate_kernel(const T* __restrict__ x, const T* __restrict__ deter,
                                                            T* __restrict__ out, int64_t items, uint32_t width,
                                                            uint32_t h) {
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; item < items;
       item += static_cast<int64_t>(gridDim.x) * kThreads) {
    const Place p = place<E>(item, width, h);
    float reset[E], cand[E], update[E], d[E];
    load_n<E>(x + p.gate, reset);
    load_n<E>(x + p.gate + h, cand);
    load_n<E>(x + p.gate + 2 * h, update);
    load_n<E>(deter + p.at, d);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float r = sigmoid(reset[k]);                           // rssm.py:155
      const float c = tanhf(r * cand[k]);                          // rssm.py:156
      const float u = sigmoid(update[k] - 1.f);                    // rssm.py:157
      d[k] = u * c + (1.f - u) * d[k];                             // rssm.py:158
    }
    store_n<E>(out + p.at, d);
  }
}

// With r, c, u as above, pre = r cand and g = gout:
//   ddeter  = g (1 - u)
//   dupdate = g (c - deter) u (1 - u)
//   dcand   = g u (1 - c^2) r
//   dreset  = g u (1 - c^2) cand r (1 - r)
// every factor is bounded for a saturated gate: nothing divides.
template <typename T, int E>
__global__ __launch_bounds__(kThreads) void gru_gate_grad_kernel(const T* __restrict__ x, const T* __restrict__ deter,
                                                                 const T* __restrict__ gout, T* __restrict__ dx,
                                                                 T* __restrict__ ddeter, int64_t items, uint32_t width,
                                                                 uint32_t h) {
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; item < items;
       item += static_cast<int64_t>(gridDim.x) * kThreads) {
    const Place p = place<E>(item, width, h);
    float reset[E], cand[E], update[E], d[E], g[E];
    load_n<E>(x + p.gate, reset);
    load_n<E>(x + p.gate + h, cand);
    load_n<E>(x + p.gate + 2 * h, update);
    load_n<E>(deter + p.at, d);
    load_n<E>(gout + p.at, g);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float r = sigmoid(reset[k]);
      const float c = tanhf(r * cand[k]);
      const float u = sigmoid(update[k] - 1.f);
      const float dpre = (g[k] * u) * (1.f - c * c);
      update[k] = (g[k] * (c - d[k])) * (u * (1.f - u));
      reset[k] = (dpre * cand[k]) * (r * (1.f - r));
      cand[k] = dpre * r;
      d[k] = g[k] * (1.f - u);
    }
    if (dx) {
      store_n<E>(dx + p.gate, reset);
      store_n<E>(dx + p.gate + h, cand);
      store_n<E>(dx + p.gate + 2 * h, update);
    }
    if (ddeter) store_n<E>(ddeter + p.at, d);
  }
}

LaunchCount g_count;

bool fits(int64_t rows, int64_t width, int64_t blocks) {
  return rows >= 1 && width >= 1 && blocks >= 1 && width % blocks == 0 && width <= INT32_MAX / 3 &&
         rows <= INT32_MAX / (3 * width);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int grid_of(int64_t items) {
  const int64_t blocks = (items + kThreads - 1) / kThreads;
  return static_cast<int>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace

int64_t gru_gate_launches() { return g_count.value(); }

hipError_t launch_gru_gate(const void* x, const void* deter, bool bf16, int64_t rows, int64_t width, int64_t blocks,
                           void* out, hipStream_t stream) {
  if (!fits(rows, width, blocks) || !x || !deter || !out) return hipErrorInvalidValue;
  const int64_t h = width / blocks, count = rows * width;
  const bool vec = h % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(deter) && aligned16(out);
  const uint32_t w = static_cast<uint32_t>(width), hh = static_cast<uint32_t>(h);
#define EMB_GATE(T_, E_)                                                                                        \
  hipLaunchKernelGGL((gru_gate_kernel<T_, E_>), dim3(grid_of(count / E_)), dim3(kThreads), 0, stream,           \
                     static_cast<const T_*>(x), static_cast<const T_*>(deter), static_cast<T_*>(out), count / E_, w, hh)
  if (bf16 && vec) EMB_GATE(bf16_t, 8);
  else if (bf16) EMB_GATE(bf16_t, 1);
  else if (vec) EMB_GATE(float, 4);
  else EMB_GATE(float, 1);
#undef EMB_GATE
  return g_count.launched();
}

hipError_t launch_gru_gate_grad(const void* x, const void* deter, const void* gout, bool bf16, int64_t rows,
                                int64_t width, int64_t blocks, void* dx, void* ddeter, hipStream_t stream) {
  if (!fits(rows, width, blocks) || !x || !deter || !gout || (!dx && !ddeter)) return hipErrorInvalidValue;
  const int64_t h = width / blocks, count = rows * width;
  const bool vec = h % (bf16 ? 8 : 4) == 0 && aligned16(x) && aligned16(deter) && aligned16(gout) && aligned16(dx) &&
                   aligned16(ddeter);
  const uint32_t w = static_cast<uint32_t>(width), hh = static_cast<uint32_t>(h);
#define EMB_GATE_GRAD(T_, E_)                                                                                     \
  hipLaunchKernelGGL((gru_gate_grad_kernel<T_, E_>), dim3(grid_of(count / E_)), dim3(kThreads), 0, stream,        \
                     static_cast<const T_*>(x), static_cast<const T_*>(deter), static_cast<const T_*>(gout),      \
                     static_cast<T_*>(dx), static_cast<T_*>(ddeter), count / E_, w, hh)
  if (bf16 && vec) EMB_GATE_GRAD(bf16_t, 8);
  else if (bf16) EMB_GATE_GRAD(bf16_t, 1);
  else if (vec) EMB_GATE_GRAD(float, 4);
  else EMB_GATE_GRAD(float, 1);
#undef EMB_GATE_GRAD
  return g_count.launched();
}

}  // namespace emb
