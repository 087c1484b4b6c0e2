"""Seeded cases of `embodied_amd.optim.Adam`, the chain in torch on the CPU, and
the bars.

THE FLOAT64 RUN OF `restate` IS THE DEFINITION these tests hold the optimizer to.
The chain is the PPO learner's (ppo/agent.py:114-124): optax.clip_by_global_norm,
scale_by_adam, add_decayed_weights, scale_by_learning_rate.  optax is neither
installed where the fixtures of this project are made nor part of the reference
tree, so there is no fixture made by running the reference; instead the host test
(tests/test_adam_host.py) ties `restate` to an independent implementation,
`torch.optim.AdamW` in float64 over gradients scaled by a clip coefficient that
is computed by hand, to 1e-12 on every case and step.

The hyper-parameters (3 lr x 3 clip x 2 wd x 2 warmup x 2 gradient dtypes = 72)
are crossed in full with the list `clip`, whose gradients are scaled, step by
step, to a global norm of 0.1, 10 (1 + NEAR), 0.5 (1 - NEAR) and 30: below, above
and close to either bound.  NEAR = 4e-3: rounding the gradients to bfloat16 moves
the norm by at most 2^-9 of itself, which leaves the float64 norm 2e-3 away from
the bound, far enough for float32 and float64 to take the same branch whatever
the order of the sum.  The geometry lists of tests/optim_cases.py differ in what
the kernels index, not in what they compute per element, and run the COVER
combinations, in which every value of every factor occurs.
"""
import collections
import functools

import numpy as np
import torch

from tests.optim_cases import C, LISTS as _GEOMETRY, TINY, Spec, bf16_round, ratio, ratio_nu, sample_index  # noqa: F401

f32 = np.float32
STEPS = 4
EPS = 1e-7
BETA1, BETA2 = 0.9, 0.999
METRICS = ('grad_norm', 'grad_rms', 'update_rms', 'param_rms')

NEAR = 4e-3
NORMS = (0.1, 10.0 * (1 + NEAR), 0.5 * (1 - NEAR), 30.0)        # the global norm of `clip`'s gradients, per step
MARGIN = 1e-3                                                  # no case's float64 norm is closer to its bound

LISTS = {
    # 1-D and 2-D: a mixed decay mask; the tensors differ in scale, the norm is one for all three
    'clip': (Spec((4,), gscale=0.01), Spec((2, 2), gscale=10.0), Spec((3,), gscale=1.0)),
}
LISTS.update({name: _GEOMETRY[name] for name in ('one', 'two', 'sizes', 'seventy', 'wide', 'views')})

Hyper = collections.namedtuple('Hyper', 'lr clip wd warmup bf16')
LRS, CLIPS, WDS, WARMUPS = (3e-4, 1e-2, 1.0), (10.0, 0.5, 0.0), (0.0, 0.1), (0, 3)
FULL = tuple(Hyper(lr, clip, wd, warmup, bf16) for lr in LRS for clip in CLIPS for wd in WDS for warmup in WARMUPS
             for bf16 in (False, True))
COVER = (Hyper(3e-4, 10.0, 0.0, 0, False), Hyper(1e-2, 0.5, 0.1, 3, True), Hyper(1.0, 0.0, 0.1, 3, False),
         Hyper(1.0, 0.5, 0.0, 0, True))

Case = collections.namedtuple('Case', 'list hyper')
CASES = tuple(Case('clip', h) for h in FULL) + tuple(Case(name, h) for name in LISTS if name != 'clip' for h in COVER)


def tag(case):
  c = CASES[case]
  h = c.hyper
  return f'c{case}_{c.list}_lr{h.lr:g}_k{h.clip:g}_w{h.wd:g}_u{h.warmup}_{"bf16" if h.bf16 else "f32"}'


def mask_of(specs):
  """wd_mask=None: tensors with dim() >= 2 decay."""
  return tuple(len(s.shape) >= 2 for s in specs)


def global_norm(grads):
  """optax.global_norm in float64."""
  return float(np.sqrt(sum(np.square(g.astype(np.float64)).sum() for g in grads)))


@functools.lru_cache(maxsize=None)
def _inputs(name, bf16):
  specs = LISTS[name]
  rng = np.random.default_rng([7, sorted(LISTS).index(name), len(specs)])      # one draw per list: cases share it
  p = [(s.pscale * rng.standard_normal(s.shape)).astype(f32) for s in specs]
  g = [[s.gscale * rng.standard_normal(s.shape) for s in specs] for _ in range(STEPS)]
  if name == 'clip':
    g = [[x * (NORMS[step] / global_norm(grads)) for x in grads] for step, grads in enumerate(g)]
  g = [[x.astype(f32) for x in grads] for grads in g]
  if bf16:
    g = [[bf16_round(x).reshape(x.shape) for x in grads] for grads in g]
  for x in p + [x for grads in g for x in grads]:
    x.setflags(write=False)                              # shared among the cases: left unchanged
  return {'p': p, 'g': g}


def inputs(case):
  """{'p': [array per tensor], 'g': [[array per tensor] per step]}, float32 and
  read-only; the gradients of a bfloat16 case are bfloat16 values."""
  c = CASES[case]
  return _inputs(c.list, c.hyper.bf16)


def schedule(lr, warmup, count):
  """optax.linear_schedule(0, lr, warmup) (ppo/agent.py:118): lr * min(count / warmup, 1)."""
  return lr * min(count / warmup, 1.0) if warmup else lr


def regime(grads, clip):
  """'off', 'below' or 'above', and how far the float64 norm is from the bound, relative to it."""
  if not clip:
    return 'off', float('inf')
  norm = global_norm(grads)
  return ('below' if norm < clip else 'above'), abs(norm - clip) / clip


def restate(inp, hyper, specs, dtype=torch.float64):
  """The chain on torch CPU in `dtype` over the float32 inputs; in float64 it is
  the definition.  A list over the steps of {'p', 'nu', 'mu', 'amu': [array per
  tensor], 'metrics': (4,) array}; `amu` is mu's moving average taken over |g1|,
  the condition of that signed sum (the bar of mu)."""
  lr0, clip, wd, warmup, _ = hyper
  mask = mask_of(specs)
  p = [torch.from_numpy(x.copy()).to(dtype) for x in inp['p']]
  nu = [torch.zeros_like(x) for x in p]
  mu = [torch.zeros_like(x) for x in p]
  amu = [torch.zeros_like(x) for x in p]
  count = float(sum(x.numel() for x in p))
  out = []
  for step in range(len(inp['g'])):
    t = step + 1                                                          # count = t - 1
    lr = schedule(lr0, warmup, step)
    gs = [torch.from_numpy(raw.copy()).to(dtype) for raw in inp['g'][step]]
    gsq = torch.stack([torch.square(g).sum() for g in gs]).sum()
    if clip:                                                              # optax.clip_by_global_norm
      gnorm = torch.sqrt(gsq)                                             # optax.global_norm
      trigger = gnorm < clip
      gs = [torch.where(trigger, g, (g / gnorm) * clip) for g in gs]
    usq, psq = [], []
    for i, g in enumerate(gs):
      mu[i] = BETA1 * mu[i] + (1 - BETA1) * g                             # optax.scale_by_adam: update_moment
      amu[i] = BETA1 * amu[i] + (1 - BETA1) * g.abs()
      nu[i] = BETA2 * nu[i] + (1 - BETA2) * (g * g)                       #   update_moment_per_elem_norm
      u = (mu[i] / (1 - BETA1 ** t)) / (torch.sqrt(nu[i] / (1 - BETA2 ** t)) + EPS)     #   bias_correction
      if wd and mask[i]:
        u = u + wd * p[i]                                                 # optax.add_decayed_weights
      upd = u * -lr                                                       # optax.scale_by_learning_rate
      p[i] = p[i] + upd                                                   # optax.apply_updates
      usq.append(torch.square(upd).sum())
      psq.append(torch.square(p[i]).sum())
    usq, psq = torch.stack(usq).sum(), torch.stack(psq).sum()
    n = torch.tensor(count, dtype=dtype)
    metrics = torch.stack([torch.sqrt(gsq), torch.sqrt(gsq / n), torch.sqrt(usq / n), torch.sqrt(psq / n)])
    out.append({'p': [x.numpy().copy() for x in p], 'nu': [x.numpy().copy() for x in nu],
                'mu': [x.numpy().copy() for x in mu], 'amu': [x.numpy().copy() for x in amu],
                'metrics': metrics.numpy().copy()})
  return out


@functools.lru_cache(maxsize=None)
def reference64(case):
  """The definition of a case: computed once, shared, left unchanged."""
  c = CASES[case]
  return restate(inputs(case), c.hyper, LISTS[c.list], torch.float64)


# ---- the bars, against float64 over the same float32 inputs: p and the metrics
# `ratio`, nu `ratio_nu` (tests/optim_cases.py), mu `ratio_mu`.

def ratio_mu(got, want, amu):
  """mu: worst |got - want| / (1e-5 (|want| + A)).  mu is a signed moving sum of
  gradients of any scale, so an absolute 1e-5 would hide everything at small
  gradients; A, the same moving average over |g1| from the float64 run, is the
  condition of that sum.  A is floored at the smallest normal float32."""
  got, want, amu = (np.asarray(x, np.float64) for x in (got, want, amu))
  assert got.shape == want.shape == amu.shape, (got.shape, want.shape, amu.shape)
  assert np.isfinite(want).all() and np.isfinite(amu).all()
  assert np.isfinite(got).all(), int((~np.isfinite(got)).sum())
  return float(np.max(np.abs(got - want) / (1e-5 * (np.abs(want) + np.maximum(amu, TINY))), initial=0.0))


def worst_ratios(got_steps, want_steps):
  """{'p', 'nu', 'mu', 'metrics': the worst ratio to its bar} of a run's per-step
  dicts against the float64 run's, every element."""
  worst = dict.fromkeys(('p', 'nu', 'mu', 'metrics'), 0.0)
  assert len(got_steps) == len(want_steps)
  for got, want in zip(got_steps, want_steps):
    for i in range(len(want['p'])):
      worst['p'] = max(worst['p'], ratio(got['p'][i], want['p'][i]))
      worst['nu'] = max(worst['nu'], ratio_nu(got['nu'][i], want['nu'][i]))
      worst['mu'] = max(worst['mu'], ratio_mu(got['mu'][i], want['mu'][i], want['amu'][i]))
    worst['metrics'] = max(worst['metrics'], ratio(got['metrics'], want['metrics']))
  return worst


# The (list, quantity) pairs at which the float32 DEFINITION itself misses a bar
# (the host test measures it), each with its reason: none.
EXEMPT = ()
