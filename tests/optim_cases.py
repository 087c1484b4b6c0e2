"""Seeded cases of the optimizer fixture (tests/golden/optim.npz), a restatement
of the chain in torch on the CPU, and the bars.

Shared by `tools/gen_optim_golden.py` (which feeds the inputs to the reference's
own `clip_by_agc`, `scale_by_rms` and `scale_by_momentum`), by the host test and
by the GPU tests.  `reference64` is this project's own torch-CPU code in float64;
the host test holds it against the fixture's float64 run to 1e-12 on every case,
and only then do the GPU tests use it for the elements the fixture does not hold.

A committed file is small, a tensor of 70 chunks is not: the fixture holds, per
case and per step, the four metrics (sums over EVERY element of the gradients,
the updates and the new parameters) and p, nu and mu at `sample_index(n)` of every
tensor -- all elements of a tensor of up to 8, else the two ends, the elements on
both sides of the first chunk boundary and of the first aligned vector, and the
middle.  The GPU tests compare those against the fixture and every element against
`reference64`.

The hyper-parameters (3 lr x 2 agc x 2 wd x 2 nesterov x 2 warmup x 2 gradient
dtypes = 96) are crossed in full with the list `agc` -- the tensors where the
arithmetic differs: unorm / upper below 1, above 1, pnorm below pmin.  The
geometry lists differ in what the kernels index, not in what they compute per
element, and run the five COVER combinations, in which every value of every
factor occurs, every pair of (agc, wd), (nesterov, warmup) and (dtype, lr = 1)
included; the full cross over 70-chunk tensors would take minutes, not seconds.
"""
import collections

import numpy as np
import torch

from embodied_amd.optim import CHUNK as C          # the kernels' chunk size: csrc/optim.h holds it
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round

f32 = np.float32
STEPS = 4
PMIN = 1e-3
EPS = 1e-20
BETA1, BETA2 = 0.9, 0.999
METRICS = ('grad_norm', 'grad_rms', 'update_rms', 'param_rms')

# One tensor: its shape, the element offsets of the parameter and of the gradient
# in their flat buffers (None: a tensor of its own), and the scales of p and g.
Spec = collections.namedtuple('Spec', 'shape poff goff pscale gscale', defaults=(None, None, 1.0, 1.0))

LISTS = {
    # unorm / upper < 1 (no clipping), > 1 (clipped), pnorm < pmin; 1-D and 2-D: a mixed decay mask
    'agc': (Spec((4,), gscale=0.01), Spec((2, 2), gscale=10.0), Spec((3,), pscale=1e-5, gscale=1e-6)),
    'one': (Spec((5,)),),
    'two': (Spec((C + 1,)), Spec((1, 3))),
    # 1, 3, C - 1, C, C + 1, 2C + 5 elements and a tensor of none
    'sizes': (Spec((1,)), Spec((3, 1)), Spec((C - 1,)), Spec((C // 2, 2)), Spec((C + 1,)), Spec((0,)),
              Spec((2 * C + 5,), gscale=3.0), Spec((0, 7))),
    # more descriptors than one wave is wide
    'seventy': tuple(Spec((1 + i % 4,) if i % 3 else (1, 1 + i % 4), gscale=(0.01, 1.0, 30.0)[i % 3]) for i in range(70)),
    # more partial sums than one wave holds, a ragged last chunk
    'wide': (Spec((69 * C + 7,), gscale=0.5),),
    # views into flat buffers: the same offset for p and g (vectors behind 3, 2, 1 scalar elements), different
    # ones (every access scalar), a tensor shorter than its head
    'views': (Spec((C + 2,), 1, 1), Spec((2 * C + 1,), 2, 2), Spec((7,), 3, 0), Spec((C + 3,), 3, 3), Spec((9,), 0, 2),
              Spec((2,), 1, 1), Spec((3, 2), 2, 6)),
}

Hyper = collections.namedtuple('Hyper', 'lr agc wd nesterov warmup bf16')
LRS, AGCS, WDS, WARMUPS = (4e-5, 1e-2, 1.0), (0.3, 0.0), (0.0, 0.1), (0, 3)
FULL = tuple(Hyper(lr, agc, wd, nesterov, warmup, bf16) for lr in LRS for agc in AGCS for wd in WDS
             for nesterov in (False, True) for warmup in WARMUPS for bf16 in (False, True))
COVER = (Hyper(4e-5, 0.3, 0.0, False, 0, False), Hyper(1e-2, 0.0, 0.1, True, 3, True),
         Hyper(1.0, 0.3, 0.1, False, 3, False), Hyper(1.0, 0.0, 0.0, True, 0, True),
         Hyper(1.0, 0.3, 0.0, True, 3, True))

Case = collections.namedtuple('Case', 'list hyper')
CASES = tuple(Case('agc', h) for h in FULL) + tuple(Case(name, h) for name in LISTS if name != 'agc' for h in COVER)


def tag(case):
  c = CASES[case]
  h = c.hyper
  return (f'c{case}_{c.list}_lr{h.lr:g}_a{h.agc:g}_w{h.wd:g}_n{int(h.nesterov)}_u{h.warmup}_'
          f'{"bf16" if h.bf16 else "f32"}')


def mask_of(specs):
  """wd_mask=None: tensors with dim() >= 2 decay."""
  return tuple(len(s.shape) >= 2 for s in specs)


def inputs(case):
  """{'p': [array per tensor], 'g': [[array per tensor] per step]}, float32; the
  gradients of a bfloat16 case are bfloat16 values."""
  c = CASES[case]
  specs = LISTS[c.list]
  rng = np.random.default_rng([sorted(LISTS).index(c.list), len(specs)])       # one draw per list: cases share it
  p = [(s.pscale * rng.standard_normal(s.shape)).astype(f32) for s in specs]
  g = [[(s.gscale * rng.standard_normal(s.shape)).astype(f32) for s in specs] for _ in range(STEPS)]
  if c.hyper.bf16:
    g = [[bf16_round(x).reshape(x.shape) for x in step] for step in g]
  return {'p': p, 'g': g}


def flat_digest(inp):
  arrays = {f'p{i}': x for i, x in enumerate(inp['p'])}
  arrays.update({f'g{s}_{i}': x for s, step in enumerate(inp['g']) for i, x in enumerate(step)})
  return digest(arrays)


def schedule(lr, warmup, count):
  """The reference's default: lr * min(count / warmup, 1) (agent.py:367-378)."""
  return lr * min(count / warmup, 1.0) if warmup else lr


def restate(inp, hyper, specs, dtype=torch.float64):
  """The chain on torch CPU in `dtype` over the float32 inputs: a list over the
  steps (as many as `inp['g']` holds, STEPS in every case of the fixture) of
  {'p', 'nu', 'mu': [array per tensor], 'metrics': (4,) array}."""
  lr0, agc, wd, nesterov, warmup, _ = hyper
  mask = mask_of(specs)
  p = [torch.from_numpy(x).to(dtype) for x in inp['p']]
  nu = [torch.zeros_like(x) for x in p]
  mu = [torch.zeros_like(x) for x in p]
  count = float(sum(x.numel() for x in p))
  out = []
  for step in range(len(inp['g'])):
    t = step + 1
    lr = schedule(lr0, warmup, step)
    gsq, usq, psq = [], [], []
    for i, raw in enumerate(inp['g'][step]):
      g = torch.from_numpy(raw).to(dtype)
      gsq.append(torch.square(g).sum())
      if agc:
        unorm = torch.sqrt(gsq[-1])                                         # opt.py:116, as jnp.linalg.norm does it:
        pnorm = torch.sqrt(torch.square(p[i]).sum())                        # opt.py:117  sqrt(sum(x * x))
        upper = agc * torch.maximum(torch.full_like(pnorm, PMIN), pnorm)    # opt.py:118
        g = g * (1 / torch.maximum(torch.ones_like(unorm), unorm / upper))  # opt.py:119
      nu[i] = BETA2 * nu[i] + (1 - BETA2) * (g * g)                         # opt.py:136-137
      u = g / (torch.sqrt(nu[i] / (1 - BETA2 ** t)) + EPS)                  # opt.py:138-140
      mu[i] = (1 - BETA1) * u + BETA1 * mu[i]                               # opt.py:156
      m = (1 - BETA1) * u + BETA1 * mu[i] if nesterov else mu[i]            # opt.py:157-161
      m = m / (1 - BETA1 ** t)
      if wd and mask[i]:
        m = m + wd * p[i]                                                   # agent.py:365
      upd = m * -lr                                                         # agent.py:378
      p[i] = p[i] + upd                                                     # opt.py:62
      usq.append(torch.square(upd).sum())
      psq.append(torch.square(p[i]).sum())
    gsq, usq, psq = (torch.stack(x).sum() for x in (gsq, usq, psq))
    n = torch.tensor(count, dtype=dtype)
    metrics = torch.stack([torch.sqrt(gsq), torch.sqrt(gsq / n), torch.sqrt(usq / n), torch.sqrt(psq / n)])
    out.append({'p': [x.numpy().copy() for x in p], 'nu': [x.numpy().copy() for x in nu],
                'mu': [x.numpy().copy() for x in mu], 'metrics': metrics.numpy().copy()})
  return out


def reference64(inp, hyper, specs):
  return restate(inp, hyper, specs, torch.float64)


def sample_index(n):
  """The elements of a tensor of n that the fixture holds."""
  if n <= 8:
    return np.arange(n)
  picks = {0, 1, 3, 4, n // 2, n - 2, n - 1, C - 1, C}
  return np.array(sorted(i for i in picks if 0 <= i < n))


def sampled(arrays):
  """One flat array: every tensor's sampled elements, in the order of the tensors."""
  parts = [np.asarray(a).reshape(-1)[sample_index(np.asarray(a).size)] for a in arrays]
  return np.concatenate(parts) if parts else np.zeros(0)


def unpack(packed):
  """A case's (steps, 3 S + 4) array of the fixture: p, nu, mu (steps, S) and the metrics (steps, 4)."""
  size = (packed.shape[1] - len(METRICS)) // 3
  assert packed.shape == (STEPS, 3 * size + len(METRICS)), packed.shape
  return {'p': packed[:, :size], 'nu': packed[:, size:2 * size], 'mu': packed[:, 2 * size:3 * size],
          'metrics': packed[:, 3 * size:]}


def packed_of(steps):
  """The same layout from `restate`'s (or an optimizer's) per-step dicts."""
  return np.stack([np.concatenate([*(sampled(step[k]) for k in ('p', 'nu', 'mu')), step['metrics']]) for step in steps])


# ---- the bars, against float64 over the same float32 inputs

TINY = float(np.finfo(f32).tiny)         # the smallest normal float32


def ratio(got, want):
  """p, mu and the metrics: worst |got - want| / (1e-5 + 1e-5 |want|).  mu is a
  mean of normalised updates of order 1, so the absolute term means something."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all()
  assert np.isfinite(got).all(), int((~np.isfinite(got)).sum())
  return float(np.max(np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want)), initial=0.0))


def ratio_nu(got, want):
  """nu: purely relative, 1e-5 |want|, with a floor at the smallest normal
  float32 -- a sum of non-negative terms that spans many decades."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all()
  assert np.isfinite(got).all(), int((~np.isfinite(got)).sum())
  return float(np.max(np.abs(got - want) / np.maximum(1e-5 * np.abs(want), TINY), initial=0.0))


# The families whose float32 DEFINITION misses a bar (the host test measures it):
# none is exempt unless listed here, as (list, quantity), with its reason.
EXEMPT = ()
