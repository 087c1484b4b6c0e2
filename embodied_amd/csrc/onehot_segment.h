// What one wave64 does with ONE operand of the Categorical / OneHot kernels
// (onehot_kl.hip, policy_loss.hip): a group of `classes` logits in a segment of W
// lanes, W the next power of two >= classes (2 .. 64), so a wave works on 64 / W
// groups at a time; 65 .. 256 classes: the whole wave on one group with 2 or 4
// values per lane.  Reductions are butterflies inside a segment, then one
// butterfly across the segments (wave_util.h).  Included by those translation
// units, which launch 4 such waves per workgroup and pick W and the values per
// lane from `classes` on the host by the ladder below.
#pragma once

#include "wave_util.h"           // bf16 load / store, seg_max, seg_sum, across_sum

// float32 operations one by one, as twohot.hip (holds to the end of the including file)
#pragma clang fp contract(off)

// CALL(W, NPER) for the narrowest segment of W lanes that holds a group of c (at
// most 256) logits, NPER values per lane once the wave is one segment.
#define EMB_SEGMENT_BY_WIDTH(CALL, c)    \
  do {                                   \
    if ((c) <= 2) { CALL(2, 1); }        \
    else if ((c) <= 4) { CALL(4, 1); }   \
    else if ((c) <= 8) { CALL(8, 1); }   \
    else if ((c) <= 16) { CALL(16, 1); } \
    else if ((c) <= 32) { CALL(32, 1); } \
    else if ((c) <= 64) { CALL(64, 1); } \
    else if ((c) <= 128) { CALL(64, 2); }\
    else { CALL(64, 4); }                \
  } while (0)

namespace emb {
namespace segment {

// One group of one side, lane sl of its segment holding elements sl, sl + W, ...:
// sm = softmax(x) (outs.py:213), prob and logp the distribution the reference's
// logp, kl and entropy work on -- outs.py:214-216 with unimix, the logits themselves
// (log_softmax in the log domain, finite for an underflowed class) without.
// After the mix the probabilities sum to 1 up to rounding, so the second softmax
// / log_softmax of outs.py:228, 231-232, 237-239 is the identity and is not repeated.
// Lanes past `classes` hold zeros; a segment past the row's groups (!live) works on
// zeros and reads nothing.
template <int NPER>
struct Side {
  float sm[NPER], prob[NPER], logp[NPER];
};

template <typename T, int W, int NPER>
__device__ __forceinline__ Side<NPER> side(const T* x, bool live, int sl, int classes, float unimix, float keep,
                                           float uni) {
  Side<NPER> s;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    s.logp[j] = i < classes ? (live ? load(x, i) : 0.f) : -INFINITY;
    m = fmaxf(m, s.logp[j]);
  }
  m = seg_max<W>(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = sl + W * j;
    s.sm[j] = i < classes ? expf(s.logp[j] - m) : 0.f;
    sum = sum + s.sm[j];
  }
  sum = seg_sum<W>(sum);
  const float lsum = logf(sum);
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const bool ok = sl + W * j < classes;
    const float sm = s.sm[j] / sum;
    s.sm[j] = ok ? sm : 0.f;
    if (unimix != 0.f) {
      const float prob = keep * sm + uni;
      s.prob[j] = ok ? prob : 0.f;
      s.logp[j] = ok ? logf(prob) : 0.f;
    } else {
      s.prob[j] = s.sm[j];
      s.logp[j] = ok ? (s.logp[j] - m) - lsum : 0.f;
    }
  }
  return s;
}

}  // namespace segment
}  // namespace emb
