"""Shapes and seeded inputs of the norm + activation tests, the fixture's cases
(tests/golden/norm_act.npz) and a numpy restatement with closed-form gradients.

Shared by `tools/gen_rssm_core_golden.py` (which feeds the fixture's inputs to the
reference's own `Norm.__call__` and `act`) and by the tests.  `evaluate` is this
project's own numpy code, every operation in one float type; `reference64` is
its float64 run.  The host test holds its forward against the fixture's float64
values and its gradients against central differences, and only then do the GPU
tests use it for the other shapes, for bfloat16-rounded inputs and for the
gradients.
"""
import collections

import numpy as np

from tests.rssm_kl_cases import forward_ratio  # noqa: F401  (the same forward bar)
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

IMPLS = ('rms', 'layer')
ACTS = ('none', 'silu', 'gelu', 'relu')
EPS = (1e-4, 1e-6)
SCALES = (1e-3, 1.0, 1e3)                        # of the input
# The lane count (63 .. 65), the vector widths (1 .. 3, 255 .. 257), the kernels'
# own switches -- 8 to 16 values per lane (512 / 513), wave to workgroup (1024 /
# 1025), 8 to 16 to 32 values per thread (2048 / 2049, 4096 / 4097), the gradient
# that holds its row to the one that streams it and the forward's workgroup of 256
# to one of 1024 (8192 / 8193) -- and the widest row (16 384)
UNITS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 1536, 2048, 2049, 4096, 4097, 8192, 8193, 12288,
         16384)
ROWS = (1, 3)
# several partial-sum workgroups with a ragged last one: 37 rows are 10 workgroups
# of 4 waves at 3 and 65 units and 37 of one row at 1025; 300 rows are 75 and 300
RAGGED = tuple((rows, units) for rows in (37, 300) for units in (3, 65, 1025))
# A `layer` row of fewer than SPREAD_BELOW values is drawn as an evenly spaced
# ladder over [-a, a], a in [0.7, 1.3], in a random order, plus 0.1 N(0, 1).
# Restricted: among 300 rows of 3 plain normal values some have a spread that is
# small against their mean, the one-pass variance cancels and the float32
# DEFINITION itself leaves the forward bar there (1.6 times, on the CPU as on the
# kernels); the ladder keeps every row's spread near its mean's size.
SPREAD_BELOW = 8
MAX_UNITS = 16384
# A `layer` row's mean is OFFSET standard deviations from 0.  Restricted: with a
# mean that is large against the spread the one-pass variance mean(x^2) - mean^2
# (nets.py:389-391) cancels in float32 and the float32 DEFINITION leaves the
# gradient bar; at half a standard deviation mean(x^2) / var = 1.25 and it does not.
OFFSET = 0.5
# every step of the kernels' width ladder with its column sums, (rows, units): a
# ragged last workgroup of 4 waves (301 rows) where a wave takes a row, and more
# rows than the gradient launch has workgroups (515 > 512) where a workgroup does,
# so the first three add a second row to their partial sums in memory
LADDER = ((301, 3), (301, 512), (301, 1024), (515, 1025), (515, 2049), (515, 4097), (515, 8192), (515, 8193),
          (515, 12288), (515, 16384))
# dscale and dshift are held to 1e-5 of the sum of |terms| only over SUM_ROWS rows or more.
# Restricted: with 3 rows a column's terms can all sit where the activation's slope
# is nearly 0 (gelu's 1 + tanh cancels there, relu's slope flips with the sign of a
# y that is 0 up to rounding), so sum |terms| is tiny against the float32
# DEFINITION's own absolute error and it leaves the bar (up to 23 times); over 300
# rows it stays at 0.04 of it.  Fewer rows are checked forward and in dx alone.
SUM_ROWS = 300

Case = collections.namedtuple('Case', 'units impl act affine eps scale')
# the fixture: every impl and activation at five widths, the other options in turn
_TURNS = tuple((affine, eps, scale) for affine in (True, False) for eps in EPS for scale in SCALES)
GOLDEN_UNITS, GOLDEN_ROWS = (1, 3, 65, 257, 1025), 3
CASES = tuple(Case(units, impl, act, *_TURNS[(5 * i + 3 * j + k) % len(_TURNS)])
              for i, units in enumerate(GOLDEN_UNITS) for j, impl in enumerate(IMPLS) for k, act in enumerate(ACTS))


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.units}_{c.impl}_{c.act}_{"affine" if c.affine else "plain"}_e{c.eps:g}_s{c.scale:g}'


def inputs_of(rows, units, impl, affine, scale, rng):
  """x (rows, units) = scale * (N(0, 1) + OFFSET for layer), scale = 1 + 0.3 N(0, 1),
  shift = 0.3 N(0, 1) for layer (None without `affine`), gout N(0, 1); all float32."""
  x = rng.standard_normal((rows, units))
  if impl == 'layer' and 1 < units < SPREAD_BELOW:
    ladder = np.linspace(-1, 1, units) * rng.uniform(0.7, 1.3, (rows, 1))
    x = rng.permuted(ladder, axis=1) + 0.1 * x
  if impl == 'layer':
    x = x + OFFSET
  out = {'x': (scale * x).astype(f32), 'gout': rng.standard_normal((rows, units)).astype(f32)}
  out['scale'] = (1 + 0.3 * rng.standard_normal(units)).astype(f32) if affine else None
  out['shift'] = (0.3 * rng.standard_normal(units)).astype(f32) if affine and impl == 'layer' else None
  return out


def inputs(case):
  c = CASES[case]
  return inputs_of(GOLDEN_ROWS, c.units, c.impl, c.affine, c.scale, np.random.default_rng([case, c.units]))


def present(inp):
  """The arrays of an input dict that are there (for the digest)."""
  return {k: v for k, v in inp.items() if v is not None}


def _sigmoid(x):
  with np.errstate(over='ignore'):
    return 1 / (1 + np.exp(-x))


_C, _K = 0.7978845608028654, 0.044715             # jax.nn.gelu(approximate=True)


def activation(name, y):
  """nets.py:26-39 -> jax.nn: (act(y), act'(y)) in the dtype of y."""
  one = y.dtype.type(1)
  if name == 'none':
    return y, np.ones_like(y)
  if name == 'silu':
    s = _sigmoid(y)
    return y * s, s * (one + y * (one - s))
  if name == 'gelu':
    half, c, k = y.dtype.type(0.5), y.dtype.type(_C), y.dtype.type(_K)
    th = np.tanh(c * (y + k * (y * y * y)))
    return y * (half * (one + th)), half * (one + th) + (half * y) * ((one - th * th) * (c * (one + 3 * k * (y * y))))
  if name == 'relu':
    return np.maximum(y, 0), (y > 0).astype(y.dtype)
  raise ValueError(name)


def evaluate(x, scale, shift, impl, act, eps, gout=None, dtype=np.float64):
  """nets.py:374-399 then nets.py:26-39 in `dtype` over float32 (or bfloat16-rounded)
  inputs.  Returns a dict: out, rstd (rows,), and with gout the closed-form dx,
  dscale, dshift and the sums of the absolute values of the two column sums'
  terms (dscale_abs, dshift_abs: what their bars are taken from)."""
  x = np.asarray(x, dtype)
  rows, units = x.shape
  g = np.ones(units, dtype) if scale is None else np.asarray(scale, dtype)
  b = np.zeros(units, dtype) if shift is None else np.asarray(shift, dtype)
  eps = dtype(eps)
  mean2 = np.square(x).mean(-1, keepdims=True)
  if impl == 'rms':
    xc, slope = x, dtype(0)
    rstd = 1 / np.sqrt(mean2 + eps)
    y = x * (rstd * g)
  else:
    mean = x.mean(-1, keepdims=True)
    raw = mean2 - np.square(mean)
    rstd = 1 / np.sqrt(np.maximum(0, raw) + eps)
    xc = x - mean
    y = xc * (rstd * g) + b
    slope = np.where(raw > 0, 1.0, np.where(raw == 0, 0.5, 0.0)).astype(dtype)      # of maximum(0, .)
  out, dact = activation(act, y)
  result = {'out': out, 'rstd': rstd[:, 0]}
  if gout is None:
    return result
  dy = np.asarray(gout, dtype) * dact
  h = dy * g
  pull = (rstd ** 3) * (h * xc).sum(-1, keepdims=True) / units
  if impl == 'rms':
    dx = rstd * h - xc * pull
  else:
    dx = rstd * (h - h.sum(-1, keepdims=True) / units) - xc * (slope * pull)
  terms = dy * (xc * rstd)
  result.update(dx=dx, dscale=terms.sum(0), dshift=dy.sum(0), dscale_abs=np.abs(terms).sum(0),
                dshift_abs=np.abs(dy).sum(0))
  return result


def reference64(x, scale, shift, impl, act, eps, gout=None):
  return evaluate(x, scale, shift, impl, act, eps, gout, np.float64)


BF16 = 2.0 ** -8          # a value stored as bfloat16 is rounded once more: half an ulp of 8 significant bits


def out_ratio(got, want, bf16=False):
  """Worst |got - want| / (1e-5 + 1e-5 |want|), a bfloat16 output with BF16 |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all() and np.isfinite(got).all()
  bar = 1e-5 + 1e-5 * np.abs(want) + (BF16 * np.abs(want) if bf16 else 0.0)
  return float(np.max(np.abs(got - want) / bar, initial=0.0))


def row_scale(gout, scale, rstd):
  """s = rstd max_j |gout_j scale_j| per row: the size of what a row's dx is made of."""
  g = 1.0 if scale is None else np.asarray(scale, np.float64)
  return np.asarray(rstd, np.float64) * np.abs(np.asarray(gout, np.float64) * g).max(-1)


def grad_ratio(got, want, s, bf16=False):
  """Worst |got - want| / (1e-5 s (1 + |want| / s)) = / (1e-5 (s + |want|)) per element,
  `s` (rows,) from `row_scale`; a bfloat16 result gets BF16 |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all() and np.isfinite(got).all()
  bar = 1e-5 * (np.asarray(s, np.float64)[:, None] + np.abs(want))
  if bf16:
    bar = bar + BF16 * np.abs(want)
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))


def sum_ratio(got, want, absolute):
  """Worst |got - want| / (1e-5 sum |terms|) of a column sum (dscale, dshift)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape and np.isfinite(got).all()
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(1e-5 * np.asarray(absolute), 1e-300)), initial=0.0))
