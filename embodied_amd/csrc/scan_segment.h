// The segment scan of the return scans, shared by scans.hip and ppo_targets.hip.
//
// y_t = a_t + b_t * y_{t+1}.  A segment of W lanes owns one row (or a piece of
// one); reverse inclusive Kogge-Stone over the affine maps
// (a1,b1) o (a2,b2) = (a1 + b1*a2, b1*b2) with __shfl_down inside the segment.
// Episode boundaries need no flags: b_t = 0.
// Internal linkage: every translation unit gets its own copy.
#pragma once

#include "device_util.h"

namespace emb {
namespace {

// Composite map of lanes [sl, W) of a segment: returns (A, B) with
// y_sl = A + B * y_{segment end + 1}.
template <int W>
__device__ __forceinline__ void affine_suffix(float& a, float& b, int sl) {
#pragma unroll
  for (int off = 1; off < W; off <<= 1) {
    const float ap = __shfl_down(a, off, W);
    const float bp = __shfl_down(b, off, W);
    if (sl + off < W) {
      a = fmaf(b, ap, a);
      b = b * bp;
    }
  }
}

// Four consecutive elements of a row at once.  Rows start wherever b*T puts
// them, so the vector types promise dword (floats) resp. byte (flags)
// alignment only; gfx950 serves such global loads in one instruction.
typedef float F4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint8_t B4 __attribute__((ext_vector_type(4), aligned(1)));
// (A branch-free form -- the short lane reads the four elements that END at
// its last one and shifts them down -- measured slower: 15.6 us against 13.4 at
// (65 536, 64), no gain at small sizes.)
__device__ __forceinline__ void load4(const float* p, int valid, float* out) {
  if (valid >= 4) {
    const F4 x = gload<F4>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = x[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = k < valid ? gload<float>(p + k) : 0.f;
  }
}
__device__ __forceinline__ void load4(const uint8_t* p, int valid, uint8_t* out) {
  if (valid >= 4) {
    const B4 x = gload<B4>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = x[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = k < valid ? gload<uint8_t>(p + k) : uint8_t{0};
  }
}
__device__ __forceinline__ void store4(float* p, int valid, const float* y) {
  if (valid >= 4) {
    F4 x;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = y[k];
    gstore<F4>(p, x);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) gstore<float>(p + k, y[k]);
  }
}

// GAE's maps (ppo/agent.py:194-199) for `valid` (1..4) consecutive steps of one
// row: the first step's value is val[i], its reward rew[ir] and its flags
// term[il], last[il]; a step's maps take the NEXT step's reward and flags and
// val[i + valid], the last one's successor (it exists: the row has one more value
// than steps).  `value` maps every critic output as it is loaded (the
// identity, or a de-normalisation).
template <typename Value>
__device__ __forceinline__ void gae_coef4(const float* val, int64_t i, const float* rew, int64_t ir,
                                          const uint8_t* term, const uint8_t* last, int64_t il, int valid,
                                          float live_scale, float lam, Value value, float* a, float* bc,
                                          float* keep) {
  float v[5], r[4];
  uint8_t tm[4], ls[4];
  float after;
  if (valid >= 4) {
    // the usual lane: all five loads issued back to back, one wait
    const F4 v4 = gload<F4>(val + i);
    after = gload<float>(val + i + 4);
    const F4 r4 = gload<F4>(rew + ir + 1);
    const B4 t4 = gload<B4>(term + il + 1);
    const B4 l4 = gload<B4>(last + il + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = v4[k];
      r[k] = r4[k];
      tm[k] = t4[k];
      ls[k] = l4[k];
    }
  } else {
    load4(val + i, valid, v);
    after = gload<float>(val + i + valid);
    load4(rew + ir + 1, valid, r);
    load4(term + il + 1, valid, tm);
    load4(last + il + 1, valid, ls);
  }
  after = value(after);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = value(v[k]);
  v[4] = after;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float next = k + 1 == valid ? after : v[k + 1];
    const bool t_ = tm[k] != 0;
    const float live = t_ ? 0.f : live_scale;
    const float cont = (t_ || ls[k] != 0) ? 0.f : lam;
    keep[k] = v[k];
    a[k] = r[k] + live * next - v[k];
    bc[k] = live * cont;
  }
}

// The lambda-return's maps with a FLOAT continuation (dreamerv3/agent.py:401-405
// through :485-489 with last = 0 and term = 1 - con, con the continue head's
// probability) for `valid` (1..4) consecutive steps of one row whose first step
// is t0 = i - row start: a step's maps take the NEXT step's reward, continuation
// and bootstrap value.  The reference's operations in its order: term = 1 - con,
// live = (1 - term) * disc, cont = lam.  The row's seed is boot[:, -1].  `value`
// maps every bootstrap value as it is loaded, as gae_coef4's.
template <typename Value>
__device__ __forceinline__ void lambda_cont_coef4(const float* rew, const float* con, const float* boot,
                                                  int64_t i, int valid, float disc, float lam, Value value,
                                                  float* a, float* bc) {
  float r[4], c[4], bt[4];
  if (valid >= 4) {
    // the usual lane: all three loads issued back to back, one wait
    const F4 r4 = gload<F4>(rew + i + 1);
    const F4 c4 = gload<F4>(con + i + 1);
    const F4 b4 = gload<F4>(boot + i + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r[k] = r4[k];
      c[k] = c4[k];
      bt[k] = b4[k];
    }
  } else {
    load4(rew + i + 1, valid, r);
    load4(con + i + 1, valid, c);
    load4(boot + i + 1, valid, bt);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float term = 1.f - c[k];
    const float live = (1.f - term) * disc;
    const float cont = lam;
    a[k] = r[k] + (1.f - cont) * live * value(bt[k]);
    bc[k] = live * cont;
  }
}

// One piece of a row, FOUR steps per lane: lane sl of the segment owns steps
// t0 .. t0+3 of row b (`valid` of them exist; 0 = a lane right of the row's
// end or of a row that does not exist), right() is y just right of the piece.
// The lane's four elements are folded sequentially (3 fma pairs), the
// Kogge-Stone runs over the W lanes' maps, then y[0..3] are formed from the
// right neighbour's first value.  keep[] is what op.coef4 hands to op.store4.
template <int W, typename Op, typename Step, typename Seed>
__device__ __forceinline__ void scan_piece4(const Op& op, int64_t b, Step t0, int valid, int sl, Seed right,
                                            float* y, float* keep) {
  float a[4] = {0.f, 0.f, 0.f, 0.f}, bc[4] = {1.f, 1.f, 1.f, 1.f};
  if (valid > 0) op.coef4(b, t0, valid, a, bc, keep);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k >= valid) {            // (0, 1) = identity map right of the row's end
      a[k] = 0.f;
      bc[k] = 1.f;
    }
  // this lane's four elements as one map, then the maps of the lanes to the right
  float A = a[3], Bm = bc[3];
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    A = fmaf(bc[k], A, a[k]);
    Bm = bc[k] * Bm;
  }
  affine_suffix<W>(A, Bm, sl);
  const float seed = right();
  const float first = fmaf(Bm, seed, A);               // y at t0
  float carry = __shfl_down(first, 1, W);              // y at t0 + 4 = the next lane's first
  if (sl == W - 1) carry = seed;
  y[3] = fmaf(bc[3], carry, a[3]);
#pragma unroll
  for (int k = 2; k >= 0; --k) y[k] = fmaf(bc[k], y[k + 1], a[k]);
}

}  // namespace
}  // namespace emb
