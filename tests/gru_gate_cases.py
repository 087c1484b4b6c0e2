"""Shapes, seeded inputs and a numpy restatement with closed-form gradients of
the blocked GRU gate at the end of `RSSM._core` (dreamerv3/rssm.py:152-159).

Shared by `tools/gen_rssm_core_golden.py` (which feeds the fixture's inputs to the
reference's own `RSSM._core`) and by the tests.  `evaluate` is this project's own
numpy code, every operation in one float type; `reference64` is its float64 run.
The host test holds its forward against the fixture's float64 values and its
gradients against central differences; the GPU tests use it for every shape and
for bfloat16-rounded inputs.
"""
import numpy as np

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# (deter, blocks): the debug config (h = 2), h = 3 (element by element), one block,
# h = 8 (16 bytes of bfloat16), h = 5, and the default model size
SHAPES = ((8, 4), (12, 4), (16, 1), (64, 8), (40, 8))
ROWS = (1, 3, 37)
LARGE = (3, 8192, 8)                              # rows, deter, blocks
# past one launch's first grid pass: 2048 workgroups of 256 threads take 524 288
# items of 4 float32; 65 rows of 32 768 are 532 480
STRIDED = (65, 32768, 8)
SCALES = (1.0, 5.0)
SATURATED = (30.0, -30.0, 90.0, -90.0)
BF16 = 2.0 ** -8          # a value stored as bfloat16 is rounded once more
# the fixture (tests/golden/gru_gate.npz): every shape at 3 rows and three input scales
GOLDEN_ROWS = 3
CASES = tuple((deter, blocks, scale) for deter, blocks in SHAPES for scale in (1.0, 5.0, 30.0))


def tag(case):
  deter, blocks, scale = CASES[case]
  return f'c{case}_{deter}x{blocks}_s{scale:g}'


def inputs(case):
  deter, blocks, scale = CASES[case]
  return inputs_of(GOLDEN_ROWS, deter, scale, np.random.default_rng([case, deter, blocks]))


def inputs_of(rows, deter, scale, rng):
  return {'x': (scale * rng.standard_normal((rows, 3 * deter))).astype(f32),
          'deter': rng.standard_normal((rows, deter)).astype(f32),
          'gout': rng.standard_normal((rows, deter)).astype(f32)}


def _sigmoid(x):
  with np.errstate(over='ignore'):
    return 1 / (1 + np.exp(-x))


def evaluate(x, deter, blocks, gout=None, dtype=np.float64):
  """rssm.py:153-158 in `dtype`: dict of out and, with gout, the closed-form dx and ddeter."""
  x, d = np.asarray(x, dtype), np.asarray(deter, dtype)
  rows, width = d.shape
  h = width // blocks
  grouped = x.reshape(rows, blocks, 3, h)                           # flat2group, then the split in three
  reset, cand, update = (grouped[:, :, i].reshape(rows, width) for i in range(3))
  one = dtype(1)
  r = _sigmoid(reset)
  c = np.tanh(r * cand)
  u = _sigmoid(update - one)
  result = {'out': u * c + (one - u) * d}
  if gout is None:
    return result
  g = np.asarray(gout, dtype)
  dpre = (g * u) * (one - c * c)
  parts = [(dpre * cand) * (r * (one - r)), dpre * r, (g * (c - d)) * (u * (one - u))]
  dx = np.stack([p.reshape(rows, blocks, h) for p in parts], 2).reshape(rows, 3 * width)
  result.update(dx=dx, ddeter=g * (one - u))
  return result


def reference64(x, deter, blocks, gout=None):
  return evaluate(x, deter, blocks, gout, np.float64)


def row_scale(gout, x, deter):
  """s = max_j |gout_j| max(1, max |x|, max |deter|) per row: every gradient element
  is gout times bounded gate factors times at most one of cand, c - deter."""
  big = np.maximum(1.0, np.maximum(np.abs(np.asarray(x, np.float64)).max(-1), np.abs(np.asarray(deter, np.float64)).max(-1)))
  return np.abs(np.asarray(gout, np.float64)).max(-1) * big


def out_ratio(got, want, bf16=False):
  """Worst |got - want| / (1e-5 + 1e-5 |want|), a bfloat16 output with BF16 |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
  bar = 1e-5 + 1e-5 * np.abs(want) + (BF16 * np.abs(want) if bf16 else 0.0)
  return float(np.max(np.abs(got - want) / bar, initial=0.0))


def grad_ratio(got, want, s, bf16=False):
  """Worst |got - want| / (1e-5 s (1 + |want| / s)); a bfloat16 result gets BF16 |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
  bar = 1e-5 * (np.asarray(s, np.float64)[:, None] + np.abs(want)) + (BF16 * np.abs(want) if bf16 else 0.0)
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))
