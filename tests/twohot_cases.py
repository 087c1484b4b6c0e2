"""Seeded inputs of the TwoHot fixture (tests/golden/twohot.npz) and a float64
restatement of the head for the shapes the fixture does not hold.

Shared by `tools/gen_twohot_golden.py` (which feeds the inputs to the
reference's own `TwoHot` class) and by the tests (which regenerate them and
check the digests stored in the fixture, so the fixture can never be compared
against other inputs).  `reference64` is this project's own numpy code; the host
test holds it against the fixture's float64 values on every case, and only then
do the GPU tests use it for other shapes and for bfloat16-rounded inputs.
"""
import collections

import numpy as np

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)

f32 = np.float32

BINS = (255, 256, 65, 64, 63, 2, 1)
KINDS = ('normal', 'wide', 'peaked', 'zero')     # N(0,1), 8 N(0,1), Gaussians in the index, all-zero
TARGETS = 2                                      # target sets per case: loss_sum takes both
ROWS = 37
ROWS_LARGE = 512                                 # one case: more rows than one workgroup sweep of a small grid

Case = collections.namedtuple('Case', 'n kind rows')
CASES = tuple(Case(n, kind, ROWS_LARGE if (n, kind) == (255, 'normal') else ROWS) for n in BINS for kind in KINDS)
# the last three rows of the first target set of every case
SPECIAL = (np.inf, -np.inf, np.nan)


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.rows}x{c.n}_{c.kind}'


def symexp(x):
  return np.sign(x) * np.expm1(np.abs(x))


def logits_of(kind, rows, n, rng):
  if kind == 'normal':
    return rng.standard_normal((rows, n)).astype(f32)
  if kind == 'wide':
    return (8 * rng.standard_normal((rows, n))).astype(f32)
  if kind == 'peaked':
    centre = rng.uniform(0, max(n - 1, 1), (rows, 1))
    width = rng.uniform(0.5, 3.0, (rows, 1))
    return (-0.5 * np.square((np.arange(n)[None] - centre) / width)).astype(f32)
  assert kind == 'zero', kind
  return np.zeros((rows, n), f32)


def targets_of(rows, bins, rng, special=False):
  """Even rows exactly on a bin, odd rows symexp(U(-22, 22)): beyond both outer
  bins (symexp(20)) as well; with `special` the last three rows +inf, -inf, NaN."""
  on_bin = bins[rng.integers(0, len(bins), rows)]
  free = symexp(rng.uniform(-22, 22, rows)).astype(f32)
  target = np.where(np.arange(rows) % 2 == 0, on_bin, free).astype(f32)
  if special:
    target[-len(SPECIAL):] = SPECIAL
  return target


def inputs(case, bins):
  """logits (rows, n) and TARGETS target sets (rows,), all float32."""
  c = CASES[case]
  assert bins.dtype == f32 and bins.shape == (c.n,)
  rng = np.random.default_rng([case, c.n, c.rows])
  out = {'logits': logits_of(c.kind, c.rows, c.n, rng)}
  for k in range(TARGETS):
    out[f'target{k}'] = targets_of(c.rows, bins, rng, special=k == 0)
  return out


def reference64(logits, bins, targets):
  """outs.py:273-330 in float64 numpy over float32 (or bfloat16-rounded) values:
  dict(pred, scale = sum |p_i b_i|, lse, probs, loss [k], twohot [k])."""
  x = np.asarray(logits, np.float64)
  b = np.asarray(bins, np.float64)
  n = x.shape[-1]
  m = x.max(-1, keepdims=True)
  e = np.exp(x - m)
  s = e.sum(-1, keepdims=True)
  probs = e / s
  lse = (m + np.log(s))[..., 0]
  pb = probs * b
  half = n // 2
  pairs = pb[..., :half][..., ::-1] + pb[..., n - half:]
  pred = pairs.sum(-1) + (pb[..., half] if n % 2 else 0.0)
  out = dict(pred=pred, scale=np.abs(pb).sum(-1), lse=lse, probs=probs, loss=[], twohot=[])
  log_pred = x - lse[..., None]
  for target in targets:
    t = np.asarray(target, np.float64)
    below = np.clip((b <= t[..., None]).sum(-1) - 1, 0, n - 1)
    above = np.clip(n - (b > t[..., None]).sum(-1), 0, n - 1)
    equal = below == above
    with np.errstate(invalid='ignore'):
      to_below = np.where(equal, 1.0, np.abs(b[below] - t))
      to_above = np.where(equal, 1.0, np.abs(b[above] - t))
      total = to_below + to_above
      w_below, w_above = to_above / total, to_below / total
      twohot = np.eye(n)[below] * w_below[..., None] + np.eye(n)[above] * w_above[..., None]
      out['twohot'].append(twohot)
      out['loss'].append(-(twohot * log_pred).sum(-1))
  return out


def grad64(ref, coefs, gout):
  """The closed form of d sum_k coefs[k] * loss_k / d logits, times gout (...)."""
  hot = sum(c * t for c, t in zip(coefs, ref['twohot']))
  return np.asarray(gout, np.float64)[..., None] * (sum(coefs) * ref['probs'] - hot)


def bf16_round(x):
  """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
  u = np.ascontiguousarray(x, f32).view(np.uint32)
  r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
  return r.view(f32)
