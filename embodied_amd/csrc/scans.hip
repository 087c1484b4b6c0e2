#include "scan_segment.h"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace emb {
namespace {

// ------------------------------------------------------------ return scans --
//
// y_t = a_t + b_t * y_{t+1}.  A segment of W lanes owns one row; lane = time
// step (scan_segment.h: the Kogge-Stone over the affine maps, the four-element
// loads and stores, the four-steps-per-lane piece); rows longer than W are
// walked right-to-left in W-wide pieces with the running y carried in a
// register.

// What differs between the scans: how (a_t, b_t) are formed from the inputs,
// the seed y_n, and what is stored.
// (Sizes: GaeOp<false> is exactly 64 bytes and LambdaOp 56, so that a scan's
// whole argument block arrives through the kernel-argument preload: with
// host-resident arguments anything beyond 64 bytes is a PCIe read in front of
// the first instruction of every wave.  B and T ride inside the op for that.)
struct NoGroups {};
struct Groups { int64_t group, gs_rew, gs_flag; };
template <bool kGrouped>
struct GaeOp : std::conditional_t<kGrouped, Groups, NoGroups> {   // ppo/agent.py:188-201
  const float* rew; const float* val; const uint8_t* last; const uint8_t* term;
  float* adv; float* tar;
  int32_t T, B; float live_scale, lam;
  // kGrouped: rew / last / term come straight out of a grouped packed batch
  // (distributed.py): row b then starts (b / group) * gs + (b % group) * T
  // elements into its key (gs_rew in floats, gs_flag in bytes).
  // `val` (the critic's output) and the results are always dense.
  // The op travels to the kernel as SCALAR arguments (unpack -> make): the
  // kernel-argument preload takes scalars and pointers, not by-value structs.
  template <typename F>
  void unpack(F&& f) const {
    if constexpr (kGrouped) f(rew, val, last, term, adv, tar, T, B, live_scale, lam, this->group, this->gs_rew, this->gs_flag);
    else f(rew, val, last, term, adv, tar, T, B, live_scale, lam);
  }
  template <typename... G>
  __host__ __device__ static GaeOp make(const float* rew, const float* val, const uint8_t* last,
                                        const uint8_t* term, float* adv, float* tar, int32_t T, int32_t B,
                                        float live_scale, float lam, G... groups) {
    GaeOp op;
    op.rew = rew; op.val = val; op.last = last; op.term = term; op.adv = adv; op.tar = tar;
    op.T = T; op.B = B; op.live_scale = live_scale; op.lam = lam;
    if constexpr (kGrouped) {
      const int64_t g[3] = {groups...};
      op.group = g[0]; op.gs_rew = g[1]; op.gs_flag = g[2];
    }
    return op;
  }
  __device__ float seed(int64_t) const { return 0.f; }
  __device__ void where(int64_t b, int64_t t, int64_t& ir, int64_t& il) const {
    ir = il = b * T + t;
    if constexpr (kGrouped) {
      const int64_t g = b / this->group, j = b - g * this->group;
      ir = g * this->gs_rew + j * T + t;
      il = g * this->gs_flag + j * T + t;
    }
  }
  __device__ void coef(int64_t b, int64_t t, float& a, float& bc, float& keep) const {
    const int64_t i = b * T + t;
    int64_t ir, il;
    where(b, t, ir, il);
    const bool tm = term[il + 1] != 0;
    const float live = tm ? 0.f : live_scale;
    const float cont = (tm || last[il + 1] != 0) ? 0.f : lam;
    keep = val[i];
    a = rew[ir + 1] + live * val[i + 1] - keep;
    bc = live * cont;
  }
  __device__ void store(int64_t b, int64_t t, float y, float keep) const {
    adv[b * (T - 1) + t] = y;
    tar[b * (T - 1) + t] = y + keep;
  }
  // Elements t0 .. t0+3 of row b (`valid` of them exist): same arithmetic as
  // coef/store, the row's index math done once.
  __device__ void coef4(int64_t b, int t0, int valid, float* a, float* bc, float* keep) const {
    const int64_t i = b * T + t0;
    int64_t ir, il;
    where(b, t0, ir, il);
    gae_coef4(val, i, rew, ir, term, last, il, valid, live_scale, lam, [](float v) { return v; }, a, bc, keep);
  }
  __device__ void store4(int64_t b, int t0, int valid, const float* y, const float* keep) const {
    float z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = y[k] + keep[k];
    emb::store4(adv + b * (T - 1) + t0, valid, y);
    emb::store4(tar + b * (T - 1) + t0, valid, z);
  }
};
static_assert(sizeof(GaeOp<false>) == 64, "the dense GAE op is covered by the kernel-argument preload");

struct LambdaOp {   // dreamerv3/agent.py:482-490
  const uint8_t* last; const uint8_t* term; const float* rew; const float* boot;
  float* ret; int32_t T, B; float disc, lam;
  template <typename F>
  void unpack(F&& f) const { f(last, term, rew, boot, ret, T, B, disc, lam); }
  __host__ __device__ static LambdaOp make(const uint8_t* last, const uint8_t* term, const float* rew,
                                           const float* boot, float* ret, int32_t T, int32_t B,
                                           float disc, float lam) {
    return LambdaOp{last, term, rew, boot, ret, T, B, disc, lam};
  }
  __device__ float seed(int64_t b) const { return boot[b * T + T - 1]; }
  __device__ void coef(int64_t b, int64_t t, float& a, float& bc, float& keep) const {
    const int64_t i = b * T + t;
    const float live = (1.f - static_cast<float>(term[i + 1] != 0)) * disc;
    const float cont = (1.f - static_cast<float>(last[i + 1] != 0)) * lam;
    keep = 0.f;
    a = rew[i + 1] + (1.f - cont) * live * boot[i + 1];
    bc = live * cont;
  }
  __device__ void store(int64_t b, int64_t t, float y, float) const { ret[b * (T - 1) + t] = y; }
  __device__ void coef4(int64_t b, int t0, int valid, float* a, float* bc, float* keep) const {
    const int64_t i = b * T + t0 + 1;
    float r[4], bt[4];
    uint8_t tm[4], ls[4];
    if (valid >= 4) {
      // the usual lane: all four loads issued back to back, one wait (as GaeOp)
      const F4 r4 = gload<F4>(rew + i);
      const F4 b4 = gload<F4>(boot + i);
      const B4 t4 = gload<B4>(term + i);
      const B4 l4 = gload<B4>(last + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r[k] = r4[k];
        bt[k] = b4[k];
        tm[k] = t4[k];
        ls[k] = l4[k];
      }
    } else {
      load4(rew + i, valid, r);
      load4(boot + i, valid, bt);
      load4(term + i, valid, tm);
      load4(last + i, valid, ls);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float live = (1.f - static_cast<float>(tm[k] != 0)) * disc;
      const float cont = (1.f - static_cast<float>(ls[k] != 0)) * lam;
      keep[k] = 0.f;
      a[k] = r[k] + (1.f - cont) * live * bt[k];
      bc[k] = live * cont;
    }
  }
  __device__ void store4(int64_t b, int t0, int valid, const float* y, const float*) const {
    emb::store4(ret + b * (T - 1) + t0, valid, y);
  }
};
static_assert(sizeof(LambdaOp) <= 64, "covered by the kernel-argument preload");

// The lambda-return of imag_loss (dreamerv3/agent.py:401-405 through :482-490):
// last = 0 and term = 1 - con with `con` the continue head's float probability,
// which the one-byte flags of LambdaOp cannot carry.
struct ContLambdaOp {
  const float* rew; const float* con; const float* boot;
  float* ret; int32_t T, B; float disc, lam;
  template <typename F>
  void unpack(F&& f) const { f(rew, con, boot, ret, T, B, disc, lam); }
  __host__ __device__ static ContLambdaOp make(const float* rew, const float* con, const float* boot,
                                               float* ret, int32_t T, int32_t B, float disc, float lam) {
    return ContLambdaOp{rew, con, boot, ret, T, B, disc, lam};
  }
  __device__ float seed(int64_t b) const { return boot[b * T + T - 1]; }
  __device__ void coef(int64_t b, int64_t t, float& a, float& bc, float& keep) const {
    const int64_t i = b * T + t;
    const float term = 1.f - con[i + 1];
    const float live = (1.f - term) * disc;
    const float cont = lam;
    keep = 0.f;
    a = rew[i + 1] + (1.f - cont) * live * boot[i + 1];
    bc = live * cont;
  }
  __device__ void store(int64_t b, int64_t t, float y, float) const { ret[b * (T - 1) + t] = y; }
  __device__ void coef4(int64_t b, int t0, int valid, float* a, float* bc, float*) const {
    lambda_cont_coef4(rew, con, boot, b * T + t0, valid, disc, lam, [](float v) { return v; }, a, bc);
  }
  __device__ void store4(int64_t b, int t0, int valid, const float* y, const float*) const {
    emb::store4(ret + b * (T - 1) + t0, valid, y);
  }
};
static_assert(sizeof(ContLambdaOp) <= 64, "covered by the kernel-argument preload");

// Short rows: a W-lane segment per row, rows longer than W walked right to
// left with the running value in a register.

template <int W, typename Op, typename... Args>
__global__ __launch_bounds__(kThreads) void scan_rows_kernel(Args... args) {
  const Op op = Op::make(args...);
  const int64_t B = op.B, n = op.T - 1;
  const int sl = threadIdx.x % W;
  const int64_t b = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / W;
  const bool row_ok = b < B;
  float carry = row_ok ? op.seed(b) : 0.f;
  for (int64_t base = ((n - 1) / W) * W; base >= 0; base -= W) {
    const int64_t t = base + sl;
    const bool ok = row_ok && t < n;
    float a = 0.f, bc = 1.f, keep = 0.f;     // (0, 1) = identity map
    if (ok) op.coef(b, t, a, bc, keep);
    affine_suffix<W>(a, bc, sl);
    const float y = fmaf(bc, carry, a);
    if (ok) op.store(b, t, y, keep);
    carry = __shfl(y, 0, W);
  }
}
//
// FOUR elements per lane: at large B the one-element-per-lane form above is
// bound by its instruction count, not by HBM ((65 536, 64): ~220 VALU
// instructions per wave and row, most of them 64-bit index arithmetic and
// shuffle addressing, 19.3 us = 50 % of peak): here the row's index math is done
// once per four elements, the loads are 16-byte / 4-byte vectors, the four
// elements of a lane are folded sequentially (3 fma pairs) and the Kogge-Stone
// runs over W = rowlen/4 lanes (4 rounds for T = 64 instead of 6).
template <int W, typename Op>
__device__ __forceinline__ void scan_rows4_body(const Op& op, uint32_t block) {
  const int64_t B = op.B;
  const int n = op.T - 1;
  const int sl = threadIdx.x % W;
  const int64_t b = (static_cast<int64_t>(block) * kThreads + threadIdx.x) / W;
  const int t0 = 4 * sl;
  const bool row_ok = b < B;
  const int valid = row_ok ? (n - t0 >= 4 ? 4 : (n - t0 > 0 ? n - t0 : 0)) : 0;
  float y[4], keep[4] = {0.f, 0.f, 0.f, 0.f};
  scan_piece4<W>(op, b, t0, valid, sl, [&] { return row_ok ? op.seed(b) : 0.f; }, y, keep);
  if (valid > 0) op.store4(b, t0, valid, y, keep);
}
template <int W, typename Op, typename... Args>
__global__ __launch_bounds__(kThreads) void scan_rows4_kernel(Args... args) {
  scan_rows4_body<W>(Op::make(args...), blockIdx.x);
}

// Several lambda-return problems of one train step in ONE launch (DreamerV3
// computes the replay returns (B, T) and the imagined returns (B*K, H+1) in the
// same step, dreamerv3/agent.py:401-405,464-466): at these sizes each scan is
// pure launch latency, so two launches cost twice what one does.  Workgroups
// [first[i], first[i+1]) belong to problem i; every problem runs the
// four-steps-per-lane form with its own segment width.
constexpr int kScanMulti = 4;
struct LambdaMulti {
  LambdaOp op[kScanMulti];
  int32_t first[kScanMulti + 1];
  int32_t width[kScanMulti];
};
__global__ __launch_bounds__(kThreads) void lambda_multi_kernel(const LambdaMulti m) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < kScanMulti; ++k)
    if (blockIdx.x >= static_cast<uint32_t>(m.first[k])) i = k;
  const uint32_t block = blockIdx.x - static_cast<uint32_t>(m.first[i]);
  // (a copy selected with a uniform index: the by-value argument stays in SGPRs)
  LambdaOp op = m.op[0];
#pragma unroll
  for (int k = 1; k < kScanMulti; ++k)
    if (i == k) op = m.op[k];
  int width = m.width[0];
#pragma unroll
  for (int k = 1; k < kScanMulti; ++k)
    if (i == k) width = m.width[k];
  switch (width) {
    case 4: scan_rows4_body<4>(op, block); break;
    case 8: scan_rows4_body<8>(op, block); break;
    case 16: scan_rows4_body<16>(op, block); break;
    case 32: scan_rows4_body<32>(op, block); break;
    default: scan_rows4_body<64>(op, block); break;
  }
}

// Long rows: one workgroup of `waves` wavefronts per row.  Each wave reduces its
// 64 steps to one affine map, the per-wave maps are staged in LDS, every wave
// folds the maps to its right into its carry, and the workgroup walks the row
// right to left in pieces of 64 * waves steps with the carry handed on through
// LDS.
template <typename Op, typename... Args>
__global__ __launch_bounds__(1024) void scan_long_rows_kernel(Args... args) {
  const Op op = Op::make(args...);
  const int64_t n = op.T - 1;
  __shared__ float s_a[16], s_b[16], s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t span = 64 * waves;
  if (threadIdx.x == 0) s_carry = op.seed(b);
  for (int64_t base = ((n - 1) / span) * span; base >= 0; base -= span) {
    const int64_t t = base + threadIdx.x;
    const bool ok = t < n;
    float a = 0.f, bc = 1.f, keep = 0.f;
    if (ok) op.coef(b, t, a, bc, keep);
    affine_suffix<64>(a, bc, lane);
    if (lane == 0) {
      s_a[wave] = a;
      s_b[wave] = bc;
    }
    __syncthreads();
    float carry = s_carry;
    for (int w = waves - 1; w > wave; --w) carry = fmaf(s_b[w], carry, s_a[w]);
    const float y = fmaf(bc, carry, a);
    if (ok) op.store(b, t, y, keep);
    __syncthreads();
    if (threadIdx.x == 0) s_carry = y;
    // the next iteration's first __syncthreads orders this write before its reads
  }
}

template <typename Op>
hipError_t launch_scan(const Op& op, hipStream_t stream) {
  const int64_t B = op.B, n = op.T - 1;
  if (n > 256) {
    const int waves = static_cast<int>(std::min<int64_t>(16, (n + 63) / 64));
    op.unpack([&](auto... a) {
      hipLaunchKernelGGL((scan_long_rows_kernel<Op, decltype(a)...>), dim3(static_cast<uint32_t>(B)),
                         dim3(64 * waves), 0, stream, a...);
    });
    return hipGetLastError();
  }
  // Short rows in small batches (Dreamer's imagined returns, (1024, 16)) stay
  // with one element per lane: 64 workgroups instead of 16, 3.4 us against 3.7.
  if (n <= 16 && B <= 8192) {
    const int64_t rows_per_block = kThreads / 16;
    const dim3 grid(static_cast<uint32_t>((B + rows_per_block - 1) / rows_per_block));
    op.unpack([&](auto... a) {
      hipLaunchKernelGGL((scan_rows_kernel<16, Op, decltype(a)...>), grid, dim3(kThreads), 0, stream, a...);
    });
    return hipGetLastError();
  }
  const int W = n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64;
  const int64_t rows_per_block = kThreads / W;
  const dim3 grid(static_cast<uint32_t>((B + rows_per_block - 1) / rows_per_block));
  op.unpack([&](auto... a) {
#define EMB_SCAN4(W_) \
  hipLaunchKernelGGL((scan_rows4_kernel<W_, Op, decltype(a)...>), grid, dim3(kThreads), 0, stream, a...)
    switch (W) {
      case 4: EMB_SCAN4(4); break;
      case 8: EMB_SCAN4(8); break;
      case 16: EMB_SCAN4(16); break;
      case 32: EMB_SCAN4(32); break;
      default: EMB_SCAN4(64); break;
    }
#undef EMB_SCAN4
  });
  return hipGetLastError();
}

// Time-major: lane = batch column (coalesced), the T-step recurrence runs
// sequentially in the reference's own order.
__global__ __launch_bounds__(kThreads) void director_score_kernel(
    const float* __restrict__ rew, const float* __restrict__ cont,
    const float* __restrict__ value, int64_t T, int64_t B, float discount, float lam,
    float* __restrict__ ret) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (b >= B) return;
  float v = value[(T - 1) * B + b];
  for (int64_t t = T - 2; t >= 0; --t) {
    const float d = cont[(t + 1) * B + b] * discount;
    const float interm = rew[t * B + b] + d * value[(t + 1) * B + b] * (1.f - lam);
    v = interm + d * lam * v;
    ret[t * B + b] = v;
  }
}

// Director manager steps (director/hierarchy.py:240-256), time-major: for every
// window j of k steps and column b:  w_i = prod_{i'<=i} cont[jk+i'],
// reward_out[j-1] = mean_i(shifted_reward[jk+i] * w_i)  (j >= 1; the reward is
// shifted by one step: shifted[0] = 0, shifted[t] = reward[t-1]),
// cont_out[j] = prod_i cont[jk+i].  Lane = column (coalesced), k is small.
__global__ __launch_bounds__(kThreads) void abstract_traj_kernel(
    const float* __restrict__ reward, const float* __restrict__ cont, int64_t T, int64_t B,
    int k, float* __restrict__ reward_out, float* __restrict__ cont_out) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (b >= B) return;
  float w = 1.f, acc = 0.f;
  for (int i = 0; i < k; ++i) {
    const int64_t t = j * k + i;
    w *= cont[t * B + b];
    const float r = (t == 0 || !reward) ? 0.f : reward[(t - 1) * B + b];
    acc += r * w;
  }
  if (cont_out) cont_out[j * B + b] = w;
  if (reward_out && j >= 1) reward_out[(j - 1) * B + b] = acc / static_cast<float>(k);
}

}  // namespace

hipError_t launch_gae(const float* rew, const float* val, const uint8_t* last,
                      const uint8_t* term, int64_t B, int64_t T, float live_scale, float lam,
                      float* adv, float* tar, hipStream_t stream, int64_t group,
                      int64_t group_stride_bytes) {
  if (B <= 0 || T < 2) return hipSuccess;
  if (group < 0 || (group && group_stride_bytes % 4 != 0) || B > INT32_MAX || T > INT32_MAX)
    return hipErrorInvalidValue;
  // (make() fills the fields both forms share; the grouped one adds its strides)
  const int32_t t = static_cast<int32_t>(T), b = static_cast<int32_t>(B);
  if (group)
    return launch_scan(GaeOp<true>::make(rew, val, last, term, adv, tar, t, b, live_scale, lam, group,
                                         group_stride_bytes / 4, group_stride_bytes), stream);
  return launch_scan(GaeOp<false>::make(rew, val, last, term, adv, tar, t, b, live_scale, lam), stream);
}

hipError_t launch_lambda_return(const uint8_t* last, const uint8_t* term, const float* rew,
                                const float* boot, int64_t B, int64_t T, float disc, float lam,
                                float* ret, hipStream_t stream) {
  if (B <= 0 || T < 2) return hipSuccess;
  if (B > INT32_MAX || T > INT32_MAX) return hipErrorInvalidValue;
  return launch_scan(LambdaOp{last, term, rew, boot, ret, static_cast<int32_t>(T),
                              static_cast<int32_t>(B), disc, lam}, stream);
}

hipError_t launch_lambda_return_cont(const float* rew, const float* con, const float* boot, int64_t B,
                                     int64_t T, float disc, float lam, float* ret, hipStream_t stream) {
  if (B <= 0 || T < 2) return hipSuccess;
  if (B > INT32_MAX || T > INT32_MAX) return hipErrorInvalidValue;
  return launch_scan(ContLambdaOp{rew, con, boot, ret, static_cast<int32_t>(T), static_cast<int32_t>(B),
                                  disc, lam}, stream);
}

hipError_t launch_lambda_return_multi(int n_problems, const LambdaProblem* problems, hipStream_t stream) {
  if (n_problems < 1) return hipSuccess;
  bool together = n_problems <= kScanMulti;
  for (int i = 0; i < n_problems; ++i) {
    const LambdaProblem& q = problems[i];
    if (q.B > INT32_MAX || q.T > INT32_MAX) return hipErrorInvalidValue;
    together = together && q.T - 1 <= 256;        // long rows have a kernel of their own
  }
  if (!together || n_problems == 1) {
    for (int i = 0; i < n_problems; ++i) {
      const LambdaProblem& q = problems[i];
      const hipError_t err = launch_lambda_return(q.last, q.term, q.rew, q.boot, q.B, q.T, q.disc, q.lam,
                                                  q.ret, stream);
      if (err != hipSuccess) return err;
    }
    return hipSuccess;
  }
  LambdaMulti m;
  std::memset(&m, 0, sizeof(m));
  int64_t blocks = 0;
  int used = 0;
  for (int i = 0; i < n_problems; ++i) {
    const LambdaProblem& q = problems[i];
    if (q.B <= 0 || q.T < 2) continue;
    const int64_t n = q.T - 1;
    const int W = n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64;
    m.op[used] = LambdaOp{q.last, q.term, q.rew, q.boot, q.ret, static_cast<int32_t>(q.T),
                          static_cast<int32_t>(q.B), q.disc, q.lam};
    m.width[used] = W;
    m.first[used] = static_cast<int32_t>(blocks);
    const int64_t rows_per_block = kThreads / W;
    blocks += (q.B + rows_per_block - 1) / rows_per_block;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    ++used;
  }
  if (used == 0) return hipSuccess;
  for (int k = used; k <= kScanMulti; ++k) m.first[k] = static_cast<int32_t>(blocks);
  hipLaunchKernelGGL(lambda_multi_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, stream, m);
  return hipGetLastError();
}

hipError_t launch_director_score(const float* rew, const float* cont, const float* value,
                                 int64_t T, int64_t B, float discount, float lam, float* ret,
                                 hipStream_t stream) {
  if (B <= 0 || T < 2) return hipSuccess;
  hipLaunchKernelGGL(director_score_kernel, dim3(static_cast<uint32_t>((B + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, stream, rew, cont, value, T, B, discount, lam, ret);
  return hipGetLastError();
}

hipError_t launch_abstract_traj(const float* reward, const float* cont, int64_t T, int64_t B,
                                int k, float* reward_out, float* cont_out, hipStream_t stream) {
  if (B <= 0 || T <= 0) return hipSuccess;
  if (k < 1 || T % k != 0) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((B + kThreads - 1) / kThreads), static_cast<uint32_t>(T / k));
  hipLaunchKernelGGL(abstract_traj_kernel, grid, dim3(kThreads), 0, stream, reward, cont, T, B, k,
                     reward_out, cont_out);
  return hipGetLastError();
}

}  // namespace emb
