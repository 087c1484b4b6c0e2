"""Seeded inputs of the Normal policy-head fixture (tests/golden/normal_policy.npz)
and a torch restatement of the actor's loss for the shapes the fixture does not
hold.

Shared by `tools/gen_normal_policy_golden.py` (which feeds the inputs to the
reference's own `imag_loss` with its own `Agg(Normal(...))` as `Head.bounded_normal`
/ `Head.normal_logstd` build it) and by the tests (which regenerate them and check
the digests stored in the fixture).  `reference64` is this project's own torch-CPU
code in float64; its autograd is the gradient oracle.  The host test holds its
forward against the fixture's float64 values on every case, and only then do the
GPU tests use it for other shapes, for bfloat16-rounded inputs and for the
gradients.

The forward bar is 1e-5 (1 + S) with S = sum_a (z^2 / 2 + |log std_a| + 1) from the
float64 run: logpi and ent are sums of A terms of either sign (log std is below 0
for std < 1, above it otherwise), so at A = 256 a result near 0 is made of terms
hundreds of times its size and 1e-5 |want| asks for more than float32 holds.
"""
import collections

import numpy as np
import torch

from tests.policy_loss_cases import BF16_GRAD, grad_ratio, row_scale  # noqa: F401  (the same gradient bar)
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# action dimensions, 0: no action axis (dims=0).  Every segment width (1, 2, 4, 8,
# 32, 64), fewer dimensions than a segment (3, 5, 6, 17, 33), 2 and 4 values per
# lane (65, 96, 256) and one past what the kernels take (257: the composed path only)
ACTIONS = (1, 2, 3, 5, 6, 17, 33, 64, 65, 96, 256, 257)
FUSED_ACTIONS = ACTIONS[:-1]
HEADS = tuple(('bounded', s) for s in (0.1, 1.0, 5.0, 30.0, 1e4)) + tuple(('logstd', s) for s in (0.1, 1.0, 3.0))
MINSTD, MAXSTD = 0.1, 1.0                        # dreamerv3/configs.yaml: policy_dist_cont's bounds
N, T = 5, 6                                      # the fixture's geometry; the reference drops the last step
ACTENT = 3e-4                                    # dreamerv3/configs.yaml, imag_loss's default
# as tests/policy_loss_cases.py: lam = 1 and contdisc make the lambda-return a plain
# sum, exact in float32, so both runs hand the policy loss the same advantages
PARAMS = dict(contdisc=True, slowtar=False, horizon=333, lam=1.0, actent=ACTENT, slowreg=1.0)
FIELDS = ('logpi', 'ent', 'loss')                # the rows of a case's array in the fixture

Case = collections.namedtuple('Case', 'actions kind scale')
CASES = tuple(Case(a, kind, scale) for a in ACTIONS for kind, scale in HEADS) + (Case(0, 'bounded', 1.0),)


def tag(case):
  c = CASES[case]
  return f'c{case}_a{c.actions}_{c.kind}_s{c.scale:g}'


def cases_of(actions):
  return [i for i, c in enumerate(CASES) if c.actions == actions]


def moments64(mean_raw, std_raw, kind, lo=MINSTD, hi=MAXSTD):
  """heads.py:150-152 / heads.py:161 in float64 numpy."""
  m, s = np.asarray(mean_raw, np.float64), np.asarray(std_raw, np.float64)
  if kind == 'bounded':
    with np.errstate(over='ignore'):
      return np.tanh(m), (hi - lo) / (1 + np.exp(-(s + 2.0))) + lo
  return m, np.exp(s)


def raw_of(n, t, actions, kind, scale, rng):
  """(mean_raw, std_raw, act), each (n, t[, actions]) float32: the raw outputs are
  scale * N(0, 1); the actions are drawn from the case's own distribution in
  float64 and stored as float32, every seventh row tripled and clipped to [-1, 1]."""
  shape = (n, t, actions) if actions else (n, t)
  mean_raw = (scale * rng.standard_normal(shape)).astype(f32)
  std_raw = (scale * rng.standard_normal(shape)).astype(f32)
  mean, std = moments64(mean_raw, std_raw, kind)
  act = mean + std * rng.standard_normal(shape)
  rows = act.reshape(n * t, -1)
  rows[::7] = np.clip(3 * rows[::7], -1, 1)
  return mean_raw, std_raw, rows.reshape(shape).astype(f32)


def inputs(case):
  """What `imag_loss` is fed: the head's raw outputs and the actions, and
  rewards, values (multiples of 1/8) and continuation flags (some of them 0)."""
  c = CASES[case]
  rng = np.random.default_rng([case, c.actions, 7])
  mean_raw, std_raw, act = raw_of(N, T, c.actions, c.kind, c.scale, rng)
  eighths = lambda: (rng.integers(-16, 17, (N, T)) / 8).astype(f32)
  return {'mean_raw': mean_raw, 'std_raw': std_raw, 'act': act,
          'rew': eighths(), 'pred': eighths(), 'con': (rng.random((N, T)) > 0.15).astype(f32)}


def restate(mean_raw, std_raw, act, adv, weight, actent, kind, dims, drop, gout=None, dtype=torch.float64,
            lo=MINSTD, hi=MAXSTD):
  """agent.py:411-415 for one continuous action key on torch CPU in `dtype` over
  float32 (or bfloat16-rounded) raw inputs (n, t[, actions]): dict of numpy arrays
  logpi, ent, loss, each (n, t - drop), S (the forward bar's scale, same shape)
  and, with an upstream gradient gout (n, t - drop), grad_mean and grad_std by
  autograd.  `act` None: no logpi term; `adv` / `weight` None: 1; weight is (n, t)
  or (n, t - drop)."""
  tensor = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
  m, s = tensor(mean_raw).requires_grad_(), tensor(std_raw).requires_grad_()
  if kind == 'bounded':                                                        # heads.py:150-152
    mean, std = torch.tanh(m), (hi - lo) * torch.sigmoid(s + 2.0) + lo
  else:                                                                        # heads.py:161
    mean, std = m, torch.exp(s)
  ent = 0.5 * torch.log(2 * np.pi * torch.square(std)) + 0.5                   # outs.py:178-179
  scale = torch.abs(torch.log(std)) + 1
  if act is None:
    logp = torch.zeros_like(ent)
  else:
    z = (tensor(act) - mean) / std                                             # outs.py:174-176
    logp = -z * z / 2 - torch.log(std) - 0.5 * np.log(2 * np.pi)
    scale = scale + z * z / 2
  if dims:
    logp, ent, scale = logp.sum(-1), ent.sum(-1), scale.sum(-1)
  kept = m.shape[1] - drop
  logpi, ent, scale = logp[:, :kept], ent[:, :kept], scale[:, :kept]
  one = torch.ones((), dtype=dtype)
  a = one if adv is None else tensor(adv)
  w = one if weight is None else tensor(weight)[:, :kept]
  loss = w * -(logpi * a + actent * ent)
  out = {'logpi': logpi.detach(), 'ent': ent.detach(), 'loss': loss.detach(), 'S': scale.detach()}
  if gout is not None:
    (loss * tensor(gout)).sum().backward()
    zeros = lambda x: torch.zeros_like(x) if x.grad is None else x.grad       # no action: the mean takes no part
    out['grad_mean'], out['grad_std'] = zeros(m), zeros(s)
  return {k: v.numpy() for k, v in out.items()}


def reference64(mean_raw, std_raw, act, adv, weight, actent, kind, dims, drop, gout=None, lo=MINSTD, hi=MAXSTD):
  return restate(mean_raw, std_raw, act, adv, weight, actent, kind, dims, drop, gout, torch.float64, lo, hi)


def forward_ratio(got, want, scale, factor=1.0):
  """Worst |got - want| / (1e-5 (1 + S) factor) per row; `factor` is
  |weight| (|adv| + actent) for the loss, 1 for logpi and ent."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all() and np.isfinite(got).all()
  bar = 1e-5 * (1 + np.asarray(scale, np.float64)) * factor
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))


def forward_ratios(got, want, adv, weight, actent):
  """The worst of the three forward ratios of one run; `want` is `reference64`'s
  dict, `weight` (n, t - drop) or None."""
  factor = (1.0 if weight is None else np.abs(np.asarray(weight, np.float64))) * (
      (1.0 if adv is None else np.abs(np.asarray(adv, np.float64))) + abs(actent))
  return max(forward_ratio(got['logpi'], want['logpi'], want['S']), forward_ratio(got['ent'], want['ent'], want['S']),
             forward_ratio(got['loss'], want['loss'], want['S'], factor))


def philox_words(seed, offset, first, count):
  """The four uint32 words of the Philox4x32-10 blocks at counters (e, offset)
  under key seed, e = first .. first + count - 1 (tests/onehot_sample_cases.py's
  numpy Philox, held there to Random123's known answers)."""
  from tests.onehot_sample_cases import philox4x32
  e = np.uint64(first) + np.arange(count, dtype=np.uint64)
  low, high = np.uint64(0xffffffff), np.uint64(32)
  shaped = lambda v: np.broadcast_to(np.uint64(v), e.shape)
  return philox4x32((e & low, e >> high, shaped(offset & 0xffffffff), shaped(offset >> 32)),
                    (shaped(seed & 0xffffffff), shaped(seed >> 32)))


def box_muller64(seed, offset, first, count):
  """The draw's definition in float64: eps = sqrt(-2 ln u1) cos(2 pi u2) with
  u1 = ((word 0 >> 8) + 1) 2^-24 and u2 = (word 1 >> 8) 2^-24."""
  words = philox_words(seed, offset, first, count)
  u1 = ((words[0] >> 8).astype(np.float64) + 1) * 2.0 ** -24
  u2 = (words[1] >> 8).astype(np.float64) * 2.0 ** -24
  return np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
