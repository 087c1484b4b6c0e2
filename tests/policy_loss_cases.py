"""Seeded inputs of the policy-loss fixture (tests/golden/policy_loss.npz) and a
torch restatement of the actor's loss for the shapes the fixture does not hold.

Shared by `tools/gen_policy_loss_golden.py` (which feeds the inputs to the
reference's own `imag_loss` with its own `Agg(Categorical(...))` as the policy)
and by the tests (which regenerate them and check the digests stored in the
fixture).  `reference64` is this project's own torch-CPU code in float64; its
autograd is the gradient oracle.  The host test holds its forward against the
fixture's float64 values on every case, and only then do the GPU tests use it
for other shapes, for bfloat16-rounded inputs and for the gradients.
"""
import collections

import numpy as np
import torch

from tests.rssm_kl_cases import forward_ratio  # noqa: F401  (the same forward bar)
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# (groups, classes), groups 0: no group axis (dims=0).  Every segment width (2, 4,
# 8, 32, 64) and fewer classes than a segment (3, 5, 18), 2 and 4 values per lane
# (96, 256), groups that are no multiple of the segments per wave (3) and more
# than one pass of the wave at W = 2 (33), and one past what the kernels take
# (257: the composed path only)
SHAPES = ((0, 2), (1, 3), (3, 5), (33, 2), (3, 18), (0, 64), (3, 96), (1, 256), (3, 257))
FUSED_SHAPES = SHAPES[:-1]
SCALES = (0.1, 1.0, 5.0, 30.0, 1e4)
UNIMIX = (0.0, 0.01)
N, T = 5, 6                                      # the fixture's geometry; the reference drops the last step
ACTENT = 3e-4                                    # dreamerv3/configs.yaml, imag_loss's default
# what imag_loss is given besides the policy: lam = 1 and contdisc make the
# lambda-return a plain sum, exact in float32 for the rewards and values below, so
# the float32 and the float64 run hand the policy loss the same advantages
PARAMS = dict(contdisc=True, slowtar=False, horizon=333, lam=1.0, actent=ACTENT, slowreg=1.0)
FIELDS = ('logpi', 'ent', 'loss')                # the rows of a case's array in the fixture

Case = collections.namedtuple('Case', 'groups classes scale unimix')
CASES = tuple(Case(g, c, scale, u) for g, c in SHAPES for scale in SCALES for u in UNIMIX)

# The families whose float32 DEFINITION misses the gradient bar (the host test
# measures it): none is exempt unless listed here with its reason.  Each entry is
# (unimix, scale); such a case is held to the forward bar and finite gradients.
GRAD_EXEMPT = ()


def grad_held(unimix, scale):
  return (unimix, scale) not in GRAD_EXEMPT


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.groups}x{c.classes}_s{c.scale:g}_u{c.unimix:g}'


def logits_of(n, t, groups, classes, scale, rng):
  """(n, t, [groups,] classes) float32: scale * N(0, 1)."""
  shape = (n, t, groups, classes) if groups else (n, t, classes)
  return (scale * rng.standard_normal(shape)).astype(f32)


def actions_of(n, t, groups, classes, rng):
  """(n, t[, groups]) int32, uniform over the classes; the first four (or as many
  as there are) are class 0, the last class, and two outside: -1 and `classes`."""
  shape = (n, t, groups) if groups else (n, t)
  act = rng.integers(0, classes, shape).astype(np.int32)
  flat = act.reshape(-1)
  edge = np.array([0, classes - 1, -1, classes], np.int32)[:flat.size]
  flat[:edge.size] = edge
  return act


def inputs(case):
  """What `imag_loss` is fed: the policy's logits and actions, and rewards,
  values (multiples of 1/8) and continuation flags (some of them 0, so some
  weights are)."""
  c = CASES[case]
  rng = np.random.default_rng([case, c.groups, c.classes])
  eighths = lambda: (rng.integers(-16, 17, (N, T)) / 8).astype(f32)
  return {'logits': logits_of(N, T, c.groups, c.classes, c.scale, rng),
          'act': actions_of(N, T, c.groups, c.classes, rng),
          'rew': eighths(), 'pred': eighths(), 'con': (rng.random((N, T)) > 0.15).astype(f32)}


def _dist(logits, unimix):
  """outs.py:210-217."""
  if unimix:
    probs = torch.softmax(logits, -1)
    uniform = torch.ones_like(probs) / probs.shape[-1]
    probs = (1 - unimix) * probs + unimix * uniform
    logits = torch.log(probs)
  return logits


def _logp(logits, act, dims):
  """outs.py:226-228 under Agg.logp (outs.py:63-64); jax.nn.one_hot as a comparison."""
  onehot = (act[..., None] == torch.arange(logits.shape[-1])).to(logits.dtype)
  logp = (torch.log_softmax(logits, -1) * onehot).sum(-1)
  return logp.sum(-1) if dims else logp


def _entropy(logits, dims):
  """outs.py:230-234 under Agg.entropy (outs.py:69-71)."""
  logprob = torch.log_softmax(logits, -1)
  prob = torch.softmax(logits, -1)
  entropy = -(prob * logprob).sum(-1)
  return entropy.sum(-1) if dims else entropy


def restate(logits, act, adv, weight, actent, unimix, dims, drop, gout=None, dtype=torch.float64):
  """agent.py:411-415 for one action key on torch CPU in `dtype` over float32 (or
  bfloat16-rounded) logits (n, t, [groups,] classes): dict of numpy arrays logpi,
  ent, loss, each (n, t - drop), and, with an upstream gradient gout (n, t - drop),
  grad = d sum(loss * gout) / d logits by autograd.  `act` None: no logpi term;
  `adv` / `weight` None: 1; weight is (n, t) or (n, t - drop)."""
  x = torch.from_numpy(np.ascontiguousarray(logits)).to(dtype).requires_grad_()
  dist = _dist(x, unimix)
  ent = _entropy(dist, dims)
  logpi = torch.zeros_like(ent) if act is None else _logp(dist, torch.from_numpy(np.ascontiguousarray(act)), dims)
  kept = x.shape[1] - drop
  logpi, ent = logpi[:, :kept], ent[:, :kept]
  one = torch.ones((), dtype=dtype)
  a = one if adv is None else torch.from_numpy(np.ascontiguousarray(adv)).to(dtype)
  w = one if weight is None else torch.from_numpy(np.ascontiguousarray(weight)).to(dtype)[:, :kept]
  loss = w * -(logpi * a + actent * ent)
  out = {'logpi': logpi.detach(), 'ent': ent.detach(), 'loss': loss.detach()}
  if gout is not None:
    (loss * torch.from_numpy(np.ascontiguousarray(gout)).to(dtype)).sum().backward()
    out['grad'] = x.grad
  return {k: v.numpy() for k, v in out.items()}


def reference64(logits, act, adv, weight, actent, unimix, dims, drop, gout=None):
  return restate(logits, act, adv, weight, actent, unimix, dims, drop, gout, torch.float64)


BF16_GRAD = 2.0 ** -8     # a gradient stored as bfloat16 is rounded once more: half an ulp of 8 significant bits


def row_scale(gout, weight, adv, actent):
  """s = |gout * weight| (|adv| + actent) per output row: the size of what multiplies a row's gradient."""
  return np.abs(np.asarray(gout, np.float64) * weight) * (np.abs(np.asarray(adv, np.float64)) + actent)


def grad_ratio(got, want, s, bf16=False):
  """Worst |got - want| / (1e-5 s (1 + |want| / s)) = / (1e-5 (s + |want|)) per
  element, `s` (rows...) the row's scale (`row_scale`) over the kept rows of
  `got`; a bfloat16 result gets BF16_GRAD |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all() and np.isfinite(got).all()
  s = np.asarray(s, np.float64)
  bar = 1e-5 * (s.reshape(s.shape + (1,) * (want.ndim - s.ndim)) + np.abs(want))
  if bf16:
    bar = bar + BF16_GRAD * np.abs(want)
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))
