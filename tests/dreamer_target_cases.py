"""Seeded inputs of the DreamerV3-target fixture (tests/golden/dreamer_targets.npz).

Shared by `tools/gen_dreamer_targets_golden.py` (which feeds them to the
reference's own `imag_loss`, `lambda_return` and `Normalize`) and by the tests
(which regenerate them and check the digests stored in the fixture, so the
fixture can never be compared against other inputs).
"""
import collections

import numpy as np

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)

f32 = np.float32

STEPS = 4                                    # consecutive train steps, state carried
PARAMS = dict(horizon=333, lam=0.95)                       # dreamerv3/agent.py:389-390
NORM = dict(rate=0.01, limit=1e-8)                         # embodied/jax/utils.py:18-19

Case = collections.namedtuple('Case', 'shape retnorm valnorm advnorm contdisc slowtar tie')
_PERC = ('perc', {})
_WIDE = ('perc', {'perclo': 1.0, 'perchi': 99.0})          # debias stays the class's default: True
_MEANSTD = ('meanstd', {})
_NONE = ('none', {})
# (N, T): the shipped normalisers (dreamerv3/configs.yaml:111-113) on a small
# batch, all three normalisers, a tiny odd shape with other percentiles and
# value.pred() as the target value, T = 2, a row longer than one segment (256
# steps) and a many-row batch with disc = 1 - 1 / horizon, ties, and one row
# walked in five pieces.
CASES = (
    Case((16, 16), _PERC, _NONE, _NONE, True, True, False),
    Case((64, 16), _PERC, _MEANSTD, _MEANSTD, True, True, False),
    Case((3, 5), _WIDE, _NONE, _NONE, True, False, False),
    Case((7, 2), _PERC, _MEANSTD, _NONE, True, True, False),
    Case((5, 257), _PERC, _NONE, _NONE, False, True, False),
    Case((256, 16), _PERC, _MEANSTD, _MEANSTD, False, True, False),
    Case((32, 8), _PERC, _NONE, _NONE, True, True, True),
    Case((1, 1030), _PERC, _NONE, _NONE, True, True, False),
)
TIE_CASE = 6         # rew and both predictions constant, con = 1: ret depends on t alone, N equal keys per t
NONE_VALNORM_CASES = tuple(i for i, case in enumerate(CASES) if case.valnorm[0] == 'none')


def tag(case):
  c = CASES[case]
  N, T = c.shape
  return f'c{case}_{N}x{T}_{c.retnorm[0]}_{c.valnorm[0]}_{c.advnorm[0]}'


def inputs(case, step):
  """rew, pred, slow ~ N(0, 1) f32 (`slow` is what slowvalue.pred() returns);
  con ~ U[0.9, 1) f32 with about 3 % exact zeros and about 3 % exact ones.  The
  tie case: rew, pred and slow one constant each per step, con = 1."""
  c = CASES[case]
  N, T = c.shape
  rng = np.random.default_rng([case, step, N, T])
  rew = rng.standard_normal(c.shape).astype(f32)
  pred = rng.standard_normal(c.shape).astype(f32)
  slow = rng.standard_normal(c.shape).astype(f32)
  con = (0.9 + 0.1 * rng.random(c.shape)).astype(f32)
  con = np.minimum(con, np.nextafter(f32(1), f32(0)))      # [0.9, 1) after the rounding too
  pick = rng.random(c.shape)
  con[pick < 0.03] = 0.0
  con[pick > 0.97] = 1.0
  if c.tie:
    rew = np.full(c.shape, rew[0, 0], f32)
    pred = np.full(c.shape, pred[0, 0], f32)
    slow = np.full(c.shape, slow[0, 0], f32)
    con = np.ones(c.shape, f32)
  return dict(rew=rew, con=con, pred=pred, slow=slow)


def target_pred(case, inp):
  """The prediction that serves as the target value (dreamerv3/agent.py:400)."""
  return inp['slow'] if CASES[case].slowtar else inp['pred']
