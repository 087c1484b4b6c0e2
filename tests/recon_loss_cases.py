"""Seeded inputs of the reconstruction-loss fixture (tests/golden/recon_loss.npz)
and the restatements the kernels of csrc/recon_loss.hip are held against.

Shared by `tools/gen_recon_loss_golden.py` (which feeds the fixture's inputs to
the reference's own `Agg`, `MSE`, `Binary` and `symlog`) and by the tests (which
regenerate them and check the digests stored in the fixture).  This project's
own code, none of the reference's:

  restate          torch-CPU float64 of each op, written so that nothing cancels at
                   large |x|; its autograd is the gradient oracle of the kernels
  restate_rounded  float64 around sigmoid(x) rounded to the compute dtype where the
                   reference rounds it (rssm.py:349) and around the roundings of
                   its backward there: the oracle of the composed path
  closed_form64    the table of the gradient in float64 numpy
  define32         the float32 definition in numpy: what the kernels compute
"""
import collections

import numpy as np
import torch

from tests.policy_loss_cases import BF16_GRAD, grad_ratio  # noqa: F401  (the same gradient bar)
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

OPS = ('mse', 'symlog', 'sigmoid', 'binary')
# the issue's widths, and one on either side of every geometry constant of
# csrc/recon_loss.h: kReconSegmentMaxUnits = 64 (63, 64, 65 are among the issue's)
# and kReconWaveMaxUnits = 2048
SEGMENT_MAX, WAVE_MAX = 64, 2048
WIDTHS = (1, 2, 3, 7, 63, 64, 65, 255, 1024, 1025, 2047, 2048, 2049, 4099, 12288, 12291, 27648)
ROWS = (1, 3, 37)
SCALES = (0.1, 1.0, 5.0, 30.0)
KINDS = ('f32', 'bf16')

Case = collections.namedtuple('Case', 'op units rows scale')


def _grid():
  """Every op x width x rows, each with two of the four scales so that every
  (op, width) meets all four."""
  out = []
  for op in OPS:
    for i, units in enumerate(WIDTHS):
      for j, rows in enumerate(ROWS):
        for scale in (SCALES[(i + j) % 4], SCALES[(i + j + 2) % 4]):
          out.append(Case(op, units, rows, scale))
  return tuple(out)


GRID = _grid()

# The fixture: two rows of each op at widths on both sides of 64, every scale.
N = 2
FIXTURE_WIDTHS = (1, 3, 64, 65, 1025)
CASES = tuple(Case(op, units, N, scale) for op in OPS for units in FIXTURE_WIDTHS for scale in SCALES)
ELEMENTWISE_MAX = 64                              # per-element losses are stored up to this width

# The (op, units) families whose float32 DEFINITION misses a bar (the host test
# measures it): none is exempt unless listed here with its reason.
LOSS_EXEMPT = ()
GRAD_EXEMPT = ()


def loss_held(op, units):
  return (op, units) not in LOSS_EXEMPT


def grad_held(op, units):
  return (op, units) not in GRAD_EXEMPT


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.op}_{c.units}_s{c.scale:g}'


def x_of(rows, units, scale, rng):
  return (scale * rng.standard_normal((rows, units))).astype(f32)


def target_of(op, rows, units, rng):
  """sigmoid: uint8 frames with 0 and 255 among them; binary: uint8 labels in
  {0, 1}; symlog: floats with 0, +-1e-3 and +-1e6 among them; mse: floats."""
  count = rows * units
  if op == 'sigmoid':
    t = rng.integers(0, 256, count).astype(np.uint8)
    t[:2] = [0, 255][:count]
    t[-2:] = [255, 0][-min(count, 2):]
  elif op == 'binary':
    t = rng.integers(0, 2, count).astype(np.uint8)
  else:
    t = (3 * rng.standard_normal(count)).astype(f32)
    if op == 'symlog':
      special = np.array([0.0, 1e-3, -1e-3, 1e6, -1e6], f32)
      at = rng.permutation(count)[:5]
      t[at] = special[:len(at)]
  return t.reshape(rows, units)


def gout_of(rows, rng):
  """Upstream gradient of the rows, float32; every fifth row is zero."""
  g = rng.standard_normal(rows).astype(f32)
  g[4::5] = 0
  return g


def data(op, units, rows, scale, kind='f32', salt=0):
  """Seeded x (bfloat16-rounded for kind 'bf16'), raw target and upstream gradient."""
  rng = np.random.default_rng([OPS.index(op), units, rows, int(scale * 10), kind == 'bf16', salt])
  x = x_of(rows, units, scale, rng)
  if kind == 'bf16':
    x = bf16_round(x)
  return {'x': x, 'target': target_of(op, rows, units, rng), 'gout': gout_of(rows, rng)}


def inputs(case):
  c = CASES[case]
  d = data(c.op, c.units, c.rows, c.scale, 'f32', salt=7 + case)
  return {'x': d['x'], 'target': d['target']}


def div_of(op):
  return 255.0 if op == 'sigmoid' else 1.0


def t32(op, target):
  """The float32 target the ops work on: float32(raw) / div in float32 (agent.py:181)."""
  t = np.asarray(target).astype(f32)
  return (t / f32(255)).astype(f32) if op == 'sigmoid' else t


# ---- float64 ----------------------------------------------------------------------

def _terms64(op, x, t):
  """The per-element loss in torch float64; `t` is the float32 target, widened."""
  logsigmoid = torch.nn.functional.logsigmoid
  if op == 'mse':
    return torch.square(x - t)
  if op == 'symlog':
    return torch.square(x - torch.sign(t) * torch.log1p(torch.abs(t)))
  if op == 'sigmoid':
    # sigmoid(x) - t without the cancellation of 1 - 1e-20: 1 - sigmoid(x) = sigmoid(-x)
    diff = torch.where(x >= 0, (1 - t) - torch.exp(logsigmoid(-x)), torch.exp(logsigmoid(x)) - t)
    return torch.square(diff)
  return -(t * logsigmoid(x) + (1 - t) * logsigmoid(-x))


def restate(op, x, target, gout=None):
  """dict of numpy float64: loss (rows,), abs = sum_j |term_j| (rows,), terms
  (rows, units) and, with `gout`, grad = d sum(loss * gout) / d x by autograd."""
  xt = torch.from_numpy(np.ascontiguousarray(x, f32)).to(torch.float64).requires_grad_()
  t = torch.from_numpy(t32(op, target)).to(torch.float64)
  terms = _terms64(op, xt, t)
  loss = terms.sum(-1)
  out = {'loss': loss.detach(), 'abs': terms.detach().abs().sum(-1), 'terms': terms.detach()}
  if gout is not None:
    (loss * torch.from_numpy(np.asarray(gout, np.float64))).sum().backward()
    out['grad'] = xt.grad
  return {k: v.numpy() for k, v in out.items()}


def sigmoid_of(x, kind='f32'):
  """torch's own sigmoid of `x` in the compute dtype (here: on the CPU), widened to
  float32: the y of `restate_rounded`."""
  xt = torch.from_numpy(np.ascontiguousarray(x, f32))
  return torch.sigmoid(xt.to(torch.bfloat16) if kind == 'bf16' else xt).to(torch.float32).numpy()


def restate_rounded(op, x, target, gout=None, kind='f32', y=None):
  """The composed path's oracle.  Every op but sigmoid: `restate`.  Sigmoid: the
  reference rounds y = sigmoid(x) to the compute dtype (rssm.py:349) and
  differentiates it there, and so does torch; both are restated in float64 AROUND
  those roundings, which are taken as they are made:
    y     the compute dtype's own sigmoid -- `y`, the device's `torch.sigmoid(x)`
          widened to float32 where the caller has it (the GPU tests hold it to the
          float64 sigmoid separately), else torch's on the CPU
    loss  sum (y - t)^2 in float64
    up    2 (y - t) g as float32 forms it, (y - t) rounded, then the product -- both
          correctly rounded operations, the same bits wherever they run -- and
          rounded to the compute dtype, as the backward of the widening cast does
    grad  (up (1 - y)) y, the order torch's backward of sigmoid multiplies in: in
          bfloat16 it rounds 1 - y and the first product to bfloat16 (each an exact
          float32 result rounded once, so the same bits wherever it runs), and so does
          this; the last product is taken in float64, its rounding is the one the
          bar allows a bfloat16 gradient.  float32: all of it in float64."""
  if op != 'sigmoid':
    return restate(op, x, target, gout)
  y32 = sigmoid_of(x, kind) if y is None else np.asarray(y, f32)
  t = t32(op, target)
  terms = np.square(y32.astype(np.float64) - t.astype(np.float64))
  out = {'loss': terms.sum(-1), 'abs': terms.sum(-1), 'terms': terms}
  if gout is not None:
    up = (f32(2) * (y32 - t).astype(f32) * np.asarray(gout, f32)[:, None]).astype(f32)
    if kind == 'bf16':
      up = bf16_round(up)
    y64 = y32.astype(np.float64)
    if kind == 'bf16':
      first = bf16_round((up * bf16_round((f32(1) - y32).astype(f32))).astype(f32))
      out['grad'] = first.astype(np.float64) * y64
    else:
      out['grad'] = up.astype(np.float64) * (1 - y64) * y64
  return out


def closed_form64(op, x, target, gout):
  """The gradient table in float64 numpy."""
  x, t = np.asarray(x, np.float64), t32(op, target).astype(np.float64)
  g = np.asarray(gout, np.float64)[:, None]
  e = np.exp(-np.abs(x))
  q = e / (1 + e)                                                    # sigmoid(-|x|)
  diff = np.where(x >= 0, (1 - t) - q, q - t)                        # sigmoid(x) - t
  if op == 'mse':
    return 2 * (x - t) * g
  if op == 'symlog':
    return 2 * (x - np.sign(t) * np.log1p(np.abs(t))) * g
  if op == 'sigmoid':
    return 2 * diff * (q / (1 + e)) * g
  return diff * g


# ---- float32 ----------------------------------------------------------------------

def define32(op, x, target, gout=None):
  """The float32 definition in numpy: dict of loss (rows,) and, with `gout`, grad."""
  x, t = np.asarray(x, f32), t32(op, target)
  one, two = f32(1), f32(2)
  with np.errstate(over='ignore', under='ignore'):
    e = np.exp(-np.abs(x), dtype=f32)
    q = (e / (one + e)).astype(f32)
    diff = np.where(x >= 0, (one - t) - q, q - t).astype(f32)
    curve = (q / (one + e)).astype(f32)                              # sigmoid(x) (1 - sigmoid(x))
    h = (f32(0.5) * np.tanh(f32(0.5) * x, dtype=f32)).astype(f32)    # sigmoid(x) - 1/2, what the kernels use below |x| = 1
    near = np.abs(x) < 1
    diff = np.where(near, (f32(0.5) - t) + h, diff).astype(f32)
    curve = np.where(near, f32(0.25) - h * h, curve).astype(f32)
    if op == 'mse':
      d = (x - t).astype(f32)
      terms, slope = d * d, two * d
    elif op == 'symlog':
      d = (x - np.copysign(np.log1p(np.abs(t), dtype=f32), t)).astype(f32)
      terms, slope = d * d, two * d
    elif op == 'sigmoid':
      terms, slope = diff * diff, (two * diff) * curve
    else:
      soft = np.log1p(e, dtype=f32)
      logp, lognotp = np.minimum(x, 0) - soft, np.minimum(-x, 0) - soft
      terms, slope = -(t * logp + (one - t) * lognotp), diff
  out = {'loss': terms.astype(f32).sum(-1, dtype=f32)}
  if gout is not None:
    out['grad'] = (slope.astype(f32) * np.asarray(gout, f32)[:, None]).astype(f32)
  return out


# ---- the bars ----------------------------------------------------------------------

def loss_ratio(got, want):
  """Worst |got - want64| / (1e-5 sum_j |term_j|) over the rows; `want` is `restate`'s dict."""
  got = np.asarray(got, np.float64).reshape(-1)
  assert got.shape == want['loss'].shape and np.isfinite(got).all()
  err = np.abs(got - want['loss'])
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(1e-5 * want['abs'], 1e-300)), initial=0.0))


def row_scale(want_grad):
  """s = max |want| over the row."""
  return np.abs(np.asarray(want_grad, np.float64)).max(-1)


# ---- the composed path's float32 definition ------------------------------------------

def define32_composed(op, x, target, gout, kind='f32', y=None):
  """What the composed path computes, in numpy: the reference's operations one by
  one in float32, sigmoid(x) (`y`, else `sigmoid_of`) and its backward in the
  compute dtype (rssm.py:349)."""
  if op != 'sigmoid':
    out = define32(op, x, target, gout)
  else:
    t, g = t32(op, target), np.asarray(gout, f32)[:, None]
    y = sigmoid_of(x, kind) if y is None else np.asarray(y, f32)
    d = (y - t).astype(f32)
    up = (f32(2) * d * g).astype(f32)
    if kind == 'bf16':
      up = bf16_round(up)
    rest = (f32(1) - y).astype(f32)
    first = (up * (bf16_round(rest) if kind == 'bf16' else rest)).astype(f32)
    out = {'loss': (d * d).astype(f32).sum(-1, dtype=f32),
           'grad': ((bf16_round(first) if kind == 'bf16' else first) * y).astype(f32)}
  if kind == 'bf16':
    out['grad'] = bf16_round(out['grad'])
  return out

