"""Seeded inputs of the PPO-target fixture (tests/golden/ppo_targets.npz).

Shared by `tools/gen_ppo_targets_golden.py` (which feeds them to the
reference's own `ppo_loss` and `Normalize`) and by the tests (which regenerate
them and check the digests stored in the fixture, so the fixture can never be
compared against other inputs).
"""
import numpy as np

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)

f32 = np.float32

STEPS = 6                                    # consecutive train steps, state carried
PARAMS = dict(hor=200, lam=0.8, tarclip=10.0)              # ppo/agent.py:179
NORM = dict(rate=0.01, limit=1e-8)                         # embodied/jax/utils.py:18-19
# (B, T), tarclip: the benchmark's shape, tiny and odd ones, T = 2, several rows
# per wave, a row longer than one segment (256 steps), one row walked in five pieces
CASES = (
    ((16, 64), 10.0), ((3, 5), 10.0), ((7, 2), 10.0), ((64, 16), 10.0), ((5, 257), 10.0),
    ((1, 1030), 10.0), ((16, 64), 2.0))
CLIP_CASE = 6                                # tarclip = 2.0: the clip bites


def tag(case):
  (B, T), tarclip = CASES[case]
  return f'c{case}_{B}x{T}_clip{tarclip:g}'


def inputs(case, step):
  """rew, pred ~ N(0, 1) f32; last ~ Bernoulli(.05), term ~ Bernoulli(.03); rows
  0 and B-1 carry a flag at t = 1 and at t = T-1 (the first and the last step a
  flag can act on)."""
  shape = CASES[case][0]
  B, T = shape
  rng = np.random.default_rng([case, step, B, T])
  rew = rng.standard_normal(shape).astype(f32)
  pred = rng.standard_normal(shape).astype(f32)
  last = rng.random(shape) < 0.05
  term = rng.random(shape) < 0.03
  for row in (0, B - 1):
    last[row, 1] = True
    term[row, T - 1] = True
  return dict(rew=rew, pred=pred, last=last, term=term)
