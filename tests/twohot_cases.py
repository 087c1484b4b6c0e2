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


def spots64(bins, target):
  """outs.py:314-324 in float64: (below, above, w_below, w_above) of `target` (rows,)."""
  b, t = np.asarray(bins, np.float64), np.asarray(target, np.float64)
  n = len(b)
  below = np.clip((b <= t[..., None]).sum(-1) - 1, 0, n - 1)
  above = np.clip(n - (b > t[..., None]).sum(-1), 0, n - 1)
  equal = below == above
  with np.errstate(invalid='ignore'):
    to_below = np.where(equal, 1.0, np.abs(b[below] - t))
    to_above = np.where(equal, 1.0, np.abs(b[above] - t))
    total = to_below + to_above
    return below, above, to_above / total, to_below / total


def reference64(logits, bins, targets):
  """outs.py:273-330 in float64 numpy over float32 (or bfloat16-rounded) values:
  dict(pred, scale = sum |p_i b_i|, lse, probs, loss [k], twohot [k], loss2 [k]).
  `loss` is the definition, -(twohot * log_pred).sum(-1) over the whole row (a
  -inf logit under a zero weight is 0 * -inf = NaN); `loss2` is the same sum over
  the two bins `below` and `above` alone, what the fused loss documents for such
  rows.  The two agree wherever every logit of the row is finite."""
  x = np.asarray(logits, np.float64)
  b = np.asarray(bins, np.float64)
  lead, n = x.shape[:-1], x.shape[-1]
  x = x.reshape(-1, n)
  rows = np.arange(len(x))
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(-1, keepdims=True)
    probs = e / s
    lse = (m + np.log(s))[..., 0]
    pb = probs * b
    half = n // 2
    pairs = pb[..., :half][..., ::-1] + pb[..., n - half:]
    pred = pairs.sum(-1) + (pb[..., half] if n % 2 else 0.0)
    out = dict(pred=pred.reshape(lead), scale=np.abs(pb).sum(-1).reshape(lead), lse=lse.reshape(lead),
               probs=probs.reshape(*lead, n), loss=[], twohot=[], loss2=[])
    log_pred = x - lse[..., None]
    for target in targets:
      below, above, w_below, w_above = spots64(b, np.asarray(target, np.float64).reshape(-1))
      # one_hot(below) * w_below + one_hot(above) * w_above without the (rows, n, n) of np.eye(n)[...]:
      # a NaN weight (a NaN target) is 0 * NaN = NaN in every bin, as there
      twohot = np.zeros_like(x)
      np.add.at(twohot, (rows, below), w_below)
      np.add.at(twohot, (rows, above), w_above)
      twohot[np.isnan(w_below) | np.isnan(w_above)] = np.nan
      out['twohot'].append(twohot.reshape(*lead, n))
      out['loss'].append(-(twohot * log_pred).sum(-1).reshape(lead))
      out['loss2'].append(-(w_below * log_pred[rows, below] + w_above * log_pred[rows, above]).reshape(lead))
  return out


def grad64(ref, coefs, gout):
  """The closed form of d sum_k coefs[k] * loss_k / d logits, times gout (...)."""
  hot = sum(c * t for c, t in zip(coefs, ref['twohot']))
  return np.asarray(gout, np.float64)[..., None] * (sum(coefs) * ref['probs'] - hot)


def composed32(logits, bins, targets, coefs, gout):
  """The composed path restated in float32 numpy, every operation rounded to
  float32: (sum_k coefs[k] * loss_k, its gradient times gout).  What float32 can
  do with another order of operations: the bars must leave it room."""
  x, b = np.asarray(logits, f32), np.asarray(bins, f32)
  n = x.shape[-1]
  rows = np.arange(len(x))
  m = x.max(-1, keepdims=True)
  log_pred = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=f32)))
  assert log_pred.dtype == f32
  total, hot = None, np.zeros_like(x)
  for target, coef in zip(targets, coefs):
    t = np.asarray(target, f32)
    below = np.clip((b <= t[..., None]).sum(-1) - 1, 0, n - 1)
    above = np.clip(n - (b > t[..., None]).sum(-1), 0, n - 1)
    equal = below == above
    to_below = np.where(equal, f32(1), np.abs(b[below] - t))
    to_above = np.where(equal, f32(1), np.abs(b[above] - t))
    span = to_below + to_above
    twohot = np.zeros_like(x)
    np.add.at(twohot, (rows, below), to_above / span)
    np.add.at(twohot, (rows, above), to_below / span)
    term = f32(coef) * -(twohot * log_pred).sum(-1, dtype=f32)
    total = term if total is None else total + term
    hot = hot + f32(coef) * twohot
  csum = f32(coefs[0])
  for coef in coefs[1:]:
    csum = csum + f32(coef)
  grad = np.asarray(gout, f32)[:, None] * (csum * np.exp(log_pred) - hot)
  assert total.dtype == grad.dtype == f32
  return total, grad


def bf16_round(x):
  """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
  u = np.ascontiguousarray(x, f32).view(np.uint32)
  r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
  return r.view(f32)


# ---- the second fixture, tests/golden/twohot_edges.npz: bins other than the
# symexp set, non-finite and extreme logits, targets at every edge of the counts

EDGE_ROWS = 16
EDGE_TARGETS = 4
EDGE_SETS = (('asym', 6), ('asym', 7), ('asym', 64), ('ties', 6), ('ties', 7), ('ties', 64), ('symexp', 64))
EDGE_LOGITS = ('normal', 'edge')
# the rows of an 'edge' case, repeated: one -inf logit in the `below` bin of the
# row's first target, in its `above` bin, elsewhere; a row of -inf; one +inf;
# one NaN; |logit| up to 1e4; N(0,1) rows stand between them
EDGE_KINDS = ('ninf_below', 'finite', 'ninf_above', 'big', 'ninf_else', 'all_ninf', 'pinf', 'nan')
POISONED = tuple(k not in ('finite', 'big') for k in EDGE_KINDS)

EdgeCase = collections.namedtuple('EdgeCase', 'bins n logits')
EDGE_CASES = tuple(EdgeCase(kind, n, logits) for kind, n in EDGE_SETS for logits in EDGE_LOGITS)
DENORMAL = float(np.finfo(f32).smallest_subnormal)


def edge_tag(case):
  c = EDGE_CASES[case]
  return f'e{case}_{c.bins}{c.n}_{c.logits}'


def custom_bins(kind, n):
  """'asym': the running sum of seeded positive steps, shifted so that zero lies
  inside but not in the middle; 'ties': the same with bins 0, 1 equal, a run of
  three equal values from n // 2 - 1 on (never zero) and the last two equal (for
  n = 6 that run and the last pair join into four)."""
  assert kind in ('asym', 'ties') and n >= 6, (kind, n)
  steps = np.random.default_rng([11, n]).uniform(0.05, 1.5, n)
  bins = (np.cumsum(steps) - 0.3 * steps.sum()).astype(f32)
  if kind == 'ties':
    run = n // 2 - 1
    bins[1] = bins[0]
    bins[run:run + 3] = bins[run]
    bins[-1] = bins[-2]
    assert bins[run] != 0
  assert np.all(np.diff(bins) >= 0) and np.isfinite(bins).all() and not np.array_equal(bins, -bins[::-1])
  return bins


def edge_bins(kind, n, symexp_bins):
  """The bins of an edge case; `symexp_bins(n)` supplies the symexp set (the
  reference's own method in the generator, `outs.symexp_twohot_bins` in the tests)."""
  return np.asarray(symexp_bins(n), f32) if kind == 'symexp' else custom_bins(kind, n)


def edge_targets(rows, bins, rng, zeros=False):
  """Four kinds in seeded order: on a bin (every eighth row the middle of the
  'ties' run); between a neighbouring pair (equal neighbours: inside the run);
  beyond an end; an outer bin or the float next to it on the far side.  With
  `zeros` the first six rows are 0.0, -0.0, the smallest denormal of either
  sign and +-bins[-1]."""
  n = len(bins)
  kinds = rng.permutation(rows) % 4
  index = rng.integers(0, n, rows)
  index[::8] = n // 2
  pair = rng.integers(0, n - 1, rows)
  frac = rng.uniform(0.05, 0.95, rows)
  between = bins[pair].astype(np.float64) + frac * (bins[pair + 1].astype(np.float64) - bins[pair])
  far = rng.uniform(0.1, 10.0, rows)
  beyond = np.where(np.arange(rows) % 2 == 0, bins[0] - far, bins[-1] + far)
  outer = np.stack([np.full(rows, bins[0]), np.full(rows, bins[-1]),
                    np.full(rows, np.nextafter(bins[0], f32(-np.inf))),
                    np.full(rows, np.nextafter(bins[-1], f32(np.inf)))])[rng.integers(0, 4, rows), np.arange(rows)]
  target = np.choose(kinds, [bins[index], between, beyond, outer]).astype(f32)
  if zeros:
    target[:6] = (0.0, -0.0, DENORMAL, -DENORMAL, bins[-1], -bins[-1])
  return target


def edge_logits(kind, rows, bins, target, rng):
  """(rows, n) float32: N(0,1), or row r of kind EDGE_KINDS[r % 8] relative to `target`."""
  n = len(bins)
  logits = rng.standard_normal((rows, n)).astype(f32)
  if kind == 'normal':
    return logits
  assert kind == 'edge', kind
  below, above, _, _ = spots64(bins, target)
  for r in range(rows):
    row = EDGE_KINDS[r % len(EDGE_KINDS)]
    if row == 'ninf_below':
      logits[r, below[r]] = -np.inf
    elif row == 'ninf_above':
      logits[r, above[r]] = -np.inf
    elif row == 'ninf_else':
      logits[r, rng.choice([i for i in range(n) if i not in (below[r], above[r])])] = -np.inf
    elif row == 'all_ninf':
      logits[r] = -np.inf
    elif row == 'pinf':
      logits[r, rng.integers(0, n)] = np.inf
    elif row == 'nan':
      logits[r, rng.integers(0, n)] = np.nan
    elif row == 'big':
      logits[r] = (1e4 * rng.uniform(-1, 1, n)).astype(f32)
  return logits


def edge_inputs(case, bins, rows=EDGE_ROWS):
  """logits (rows, n) and EDGE_TARGETS target sets (rows,), all float32."""
  c = EDGE_CASES[case]
  assert bins.dtype == f32 and bins.shape == (c.n,)
  rng = np.random.default_rng([case, c.n, rows, 5])
  out = {f'target{k}': edge_targets(rows, bins, rng, zeros=c.bins == 'symexp' and k == 0) for k in range(EDGE_TARGETS)}
  out['logits'] = edge_logits(c.logits, rows, bins, out['target0'], rng)
  return out
