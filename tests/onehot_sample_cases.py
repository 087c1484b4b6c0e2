"""Seeded inputs of the sample fixture (tests/golden/onehot_sample.npz) and three
restatements the sample kernels are held against.

Shared by `tools/gen_onehot_sample_golden.py` (which feeds the inputs to the
reference's own `Categorical.__init__`, `Categorical.pred` and
`OneHot._onehot_with_grad`) and by the tests (which regenerate them and check the
digests stored in the fixture).  This project's own code, none of the reference's:

  philox4x32 / uniforms   numpy Philox4x32-10, held to the Random123 known answers
  select64 / accepted     the inverse CDF in float64 and the acceptance rule
  restate                 torch-CPU float64 of outs.py:210-217, 219-220, 265-270;
                          its autograd is the gradient oracle
  define32                the float32 definition in numpy: what the kernels compute
"""
import collections

import numpy as np
import torch

from tests.policy_loss_cases import grad_ratio  # noqa: F401  (the same gradient bar)
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# (groups, classes), groups 0: no group axis where the API allows it.  Every
# segment width (2 .. 64), classes short of a segment (3, 5, 18), one class, 2 and
# 4 values per lane (96, 256), groups that do not fill a wave (3), more than one
# pass of a wave (33 groups at W = 2, 32 at W = 32), and one past what the kernels
# take (257: the composed path only)
SHAPES = ((0, 1), (0, 2), (1, 3), (3, 5), (33, 2), (3, 16), (3, 18), (32, 32), (0, 64), (3, 96), (1, 256), (3, 257))
FUSED_SHAPES = SHAPES[:-1]
ROWS = (1, 3, 37)
SCALES = (0.1, 1.0, 5.0, 30.0, 1e4)
UNIMIX = (0.0, 0.01)
N = 2                                             # rows of a fixture case

Case = collections.namedtuple('Case', 'groups classes scale unimix')
CASES = tuple(Case(g, c, scale, u) for g, c in SHAPES for scale in SCALES for u in UNIMIX)

# The families whose float32 DEFINITION misses the gradient bar (the host test
# measures it): none is exempt unless listed here with its reason.  Each entry is
# (unimix, scale).
GRAD_EXEMPT = ()


def grad_held(unimix, scale):
  return (unimix, scale) not in GRAD_EXEMPT


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.groups}x{c.classes}_s{c.scale:g}_u{c.unimix:g}'


def logits_of(rows, groups, classes, scale, rng):
  """(rows, [groups,] classes) float32: scale * N(0, 1); the first group's largest
  logit appears twice (classes >= 3: at classes 1 and classes - 1), so an argmax
  has a tie to break."""
  shape = (rows, groups, classes) if groups else (rows, classes)
  x = (scale * rng.standard_normal(shape)).astype(f32)
  first = x.reshape(-1, classes)[0]
  if classes >= 3:
    first[1] = first[classes - 1] = first.max() + f32(scale)
  return x


def inputs(case):
  """What the reference's classes are fed: the logits, an index per group to build
  the straight-through value for, and an upstream gradient."""
  c = CASES[case]
  rng = np.random.default_rng([case, c.groups, c.classes, 7])
  logits = logits_of(N, c.groups, c.classes, c.scale, rng)
  return {'logits': logits, 'index': rng.integers(0, c.classes, logits.shape[:-1]).astype(np.int32)}


def gout_of(shape, rng):
  """Upstream gradient of the one-hot, float32; every fifth group is zeros."""
  g = rng.standard_normal(shape).astype(f32)
  g.reshape(-1, shape[-1])[::5] = 0
  return g


# ---- the stream ---------------------------------------------------------------

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (      # Random123's kat_vectors for philox4x32-10: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32(counter, key, rounds=10):
  """Philox4x32: `counter` four and `key` two uint32 arrays (or ints) of one shape
  -> four uint32 arrays."""
  c = [np.asarray(v, np.uint64) & 0xffffffff for v in counter]
  k = [np.asarray(v, np.uint64) & 0xffffffff for v in key]
  mask = np.uint64(0xffffffff)
  for _ in range(rounds):
    p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
    k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
  return tuple(v.astype(np.uint32) for v in c)


def uniforms(seed, offset, first, count):
  """(count,) float32: u of the groups first .. first + count - 1 -- key
  (seed low, seed high), counter (g low, g high, offset low, offset high),
  u = (word 0 >> 8) * 2^-24."""
  g = np.uint64(first) + np.arange(count, dtype=np.uint64)
  lo, hi = (lambda v: np.uint64(v) & np.uint64(0xffffffff)), (lambda v: np.uint64(v) >> np.uint64(32))
  shaped = lambda v: np.broadcast_to(v, g.shape)
  word = philox4x32((g & np.uint64(0xffffffff), g >> np.uint64(32), shaped(lo(offset)), shaped(hi(offset))),
                    (shaped(lo(seed)), shaped(hi(seed))))[0]
  return ((word >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)).astype(f32)


# ---- the draw -----------------------------------------------------------------

def tol_of(classes):
  """The acceptance rule's slack on the CDF: at most `classes` float32 additions of
  terms that sum to 1, half an ulp of at most 1 (2^-24) each, plus a few ulps for
  the softmax and the blend."""
  return (classes + 8) * 2.0 ** -23


def probs64(logits, unimix):
  """(1 - unimix) softmax(x) + unimix / classes in float64 over float32 (or
  bfloat16-rounded) logits."""
  x = np.asarray(logits, np.float64)
  e = np.exp(x - x.max(-1, keepdims=True))
  p = e / e.sum(-1, keepdims=True)
  return (1 - unimix) * p + unimix / x.shape[-1] if unimix else p


def cdf64(probs):
  c = np.cumsum(np.asarray(probs, np.float64), -1)
  return c / c[..., -1:]


def select64(probs, u):
  """The smallest k with C64_k > u per group (`probs` (..., classes) float64, `u`
  (...)); the last class with p > 0 if there is none."""
  c = cdf64(probs)
  hit = (c > np.asarray(u, np.float64)[..., None]) & (probs > 0)
  last = probs.shape[-1] - 1 - np.argmax((probs > 0)[..., ::-1], -1)
  return np.where(hit.any(-1), np.argmax(hit, -1), last)


def accepted(probs, u, k, tol):
  """Per group (ok, near): ok -- C64[k - 1] - tol <= u < C64[k] + tol, 0 <= k <
  classes and p[k] > 0; near -- u lies within tol of a boundary of the CDF, where
  either neighbour may be taken."""
  c = cdf64(probs)
  u = np.asarray(u, np.float64)
  k = np.asarray(k, np.int64)
  inside = (k >= 0) & (k < probs.shape[-1])
  kk = np.clip(k, 0, probs.shape[-1] - 1)[..., None]
  below = np.where(kk[..., 0] > 0, np.take_along_axis(c, np.maximum(kk - 1, 0), -1)[..., 0], 0.0)
  above = np.take_along_axis(c, kk, -1)[..., 0]
  ok = inside & (below - tol <= u) & (u < above + tol) & (np.take_along_axis(probs, kk, -1)[..., 0] > 0)
  near = (np.abs(c[..., :-1] - u[..., None]) <= tol).any(-1) if probs.shape[-1] > 1 else np.zeros(u.shape, bool)
  return ok, near


def softmax32(logits):
  x = np.asarray(logits, f32)
  e = np.exp(x - x.max(-1, keepdims=True), dtype=f32)
  return (e / e.sum(-1, keepdims=True, dtype=f32)).astype(f32)


def define32(logits, unimix, u=None, gout=None):
  """The float32 definition in numpy: dict of probs (the blend), cdf (sequential
  float32 prefix sum), index (with `u`), argmax, and grad (with `gout`) =
  keep s (g - sum_k s_k g_k)."""
  x = np.asarray(logits, f32)
  classes = x.shape[-1]
  s = softmax32(x)
  keep, uni = f32(1) - f32(unimix), f32(unimix) * (f32(1) / f32(classes))
  p = (keep * s + uni).astype(f32) if unimix else s
  out = {'probs': p, 'cdf': np.cumsum(p, -1, dtype=f32), 'argmax': np.argmax(x, -1)}
  if u is not None:
    c = out['cdf']
    hit = (c > (np.asarray(u, f32)[..., None] * c[..., -1:]).astype(f32)) & (p > 0)
    last = classes - 1 - np.argmax((p > 0)[..., ::-1], -1)
    out['index'] = np.where(hit.any(-1), np.argmax(hit, -1), last)
  if gout is not None:
    g = np.asarray(gout, f32)
    dot = (s * g).sum(-1, keepdims=True, dtype=f32)
    out['grad'] = (keep * (s * (g - dot))).astype(f32)
  return out


# ---- the reference expression ---------------------------------------------------

def restate(logits, unimix, index=None, gout=None, dtype=torch.float64):
  """outs.py:210-217 (`Categorical.__init__`), 219-220 (`pred`) and 265-270
  (`_onehot_with_grad`) on torch CPU in `dtype` over float32 (or bfloat16-rounded)
  logits: dict of numpy arrays probs (the mixed probabilities), argmax, and with
  `index` value = sg(onehot) + (probs - sg(probs)), with `gout` as well
  grad = d sum(value * gout) / d logits by autograd."""
  x = torch.from_numpy(np.ascontiguousarray(logits)).to(dtype).requires_grad_()
  dist = x
  if unimix:
    probs = torch.softmax(x, -1)
    uniform = torch.ones_like(probs) / probs.shape[-1]
    probs = (1 - unimix) * probs + unimix * uniform
    dist = torch.log(probs)
  out = {'probs': torch.softmax(dist, -1).detach(), 'argmax': torch.argmax(dist, -1)}
  if index is not None:
    onehot = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(index, np.int64)), x.shape[-1]).to(dtype)
    probs = torch.softmax(dist, -1)
    value = onehot.detach() + (probs - probs.detach())
    out['value'] = value.detach()
    if gout is not None:
      (value * torch.from_numpy(np.ascontiguousarray(gout)).to(dtype)).sum().backward()
      out['grad'] = x.grad
  return {k: v.numpy() for k, v in out.items()}


def closed_form64(logits, unimix, gout):
  """(1 - unimix) s (g - sum_k s_k g_k), s = softmax(x), in float64."""
  s = probs64(logits, 0.0)
  g = np.asarray(gout, np.float64)
  return (1 - unimix) * s * (g - (s * g).sum(-1, keepdims=True))


def group_scale(gout, unimix):
  """s = (1 - unimix) max |g| over the group: the size of what multiplies its gradient."""
  return (1 - unimix) * np.abs(np.asarray(gout, np.float64)).max(-1)


# ---- the statistical test -------------------------------------------------------

STAT_GROUPS = 65536
STAT_CLASSES = (5, 32, 256)
STAT_SEEDS = {5: 0x1234567890abcdef, 32: 0xfedcba9876543210, 256: 0x0f1e2d3c4b5a6978}
STAT_OFFSET = 3


def stat_logits(classes):
  """One row of `classes` logits, 1.5 * N(0, 1), seeded."""
  return (1.5 * np.random.default_rng([classes, 11]).standard_normal(classes)).astype(f32)


def chi_square(counts, probs):
  """(statistic, degrees of freedom) of Pearson's chi-square over the classes with
  an expected count of at least 5, the rest pooled into one cell."""
  counts, expected = np.asarray(counts, np.float64), np.asarray(probs, np.float64) * np.sum(counts)
  big = expected >= 5
  obs, exp = list(counts[big]), list(expected[big])
  if (~big).any():
    obs.append(counts[~big].sum())
    exp.append(expected[~big].sum())
  obs, exp = np.array(obs), np.array(exp)
  keep = exp > 0
  assert obs[~keep].sum() == 0
  return float((((obs - exp) ** 2)[keep] / exp[keep]).sum()), int(keep.sum()) - 1


def chi_square_bound(dof):
  """The 1 - 10^-6 quantile of the chi-square distribution."""
  from scipy.stats import chi2
  return float(chi2.isf(1e-6, dof))
