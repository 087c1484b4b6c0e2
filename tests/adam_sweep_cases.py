"""Tensor lists that take `embodied_amd.optim.Adam`'s two kernels (csrc/optim.hip:
`optim_norms_kernel<false>`, `optim_adam_update_kernel`) past the first iteration
of their loops, sized by the kernels' own constants read out of the source:

  * `k += kThreads` in the update kernel, EVERY workgroup's sum of ALL chunks'
    partials for the one global norm, needs more than kThreads chunks in all;
  * `chunk += gridDim.x` in both kernels needs more than kMaxBlocks chunks;
  * `k += kMetricThreads` in the metrics kernel needs more than kMetricThreads.

The shapes are those of tests/optim_sweep_cases.py.  `many` is 2 kMaxBlocks + 3
tensors of 1 to 5 elements, one chunk each: a workgroup handles chunks i,
i + kMaxBlocks and, for i < 3, i + 2 kMaxBlocks.  `deep` is a tensor of
kThreads + 2 chunks with a ragged last one, a tensor of 3 elements and a second
large one as a view at element offset 1 of both p and g (head = 3).

What differs from LaProp's lists is where the gradients' norm sits, because
Adam's clip is one decision for all tensors.  The gradients are rescaled per
step, in float64 before the cast to float32, so that the part of the norm a
kernel would see that stopped after the first pass is on the OTHER side of the
bound from the whole:

  many  steps 0 and 2: global norm 30, above both bounds (10 and 0.5); the
        tensors in chunks < kMaxBlocks carry 0.2 of it, below both.
        steps 1 and 3: global norm 0.1, below both.
  deep  step 0: global norm 20; the first kThreads C elements of tensor 0
        (chunks 0 .. kThreads - 1, all a one-round sum sees) carry 5; clip = 10.
        step 1: global norm 5.

In the bfloat16 cases of `many` the list is MIXED: tensor i has a bfloat16
gradient iff i % 3 == 0, the others float32, and only those tensors' values are
bf16-rounded.  kMaxBlocks % 3 != 0, so a workgroup's first and second chunk
differ in dtype in most workgroups.  In `deep`'s every gradient is bfloat16.

The oracle is `adam_cases.restate(..., torch.float64)`, which the host test ties
to `torch.optim.AdamW`; the bars are `adam_cases`'.  Plain numpy and torch-CPU.
"""
import numpy as np
import torch

from tests import adam_cases as cases
from tests.adam_cases import Hyper, worst_ratios  # noqa: F401
from tests.optim_sweep_cases import _small, kernel_constants
from tests.optim_cases import C, Spec, bf16_round

f32 = np.float32
K = kernel_constants()
BLOCKS = K['kMaxBlocks']
THREADS = K['kThreads']
DEEP = (THREADS + 1) * C + 7                # kThreads + 2 chunks, the last one of 7 elements

LISTS = {
    'many': tuple(_small(i) for i in range(2 * BLOCKS + 3)),
    'deep': (Spec((DEEP,)), Spec((3,)), Spec((DEEP,), 1, 1)),
}
STEPS = {'many': 4, 'deep': 2}
HYPERS = {'many': cases.COVER,
          'deep': (Hyper(1e-2, 10.0, 0.1, 0, False), Hyper(1e-2, 10.0, 0.1, 0, True))}
CASES = tuple((name, i) for name in LISTS for i in range(len(HYPERS[name])))

# (the whole norm, the norm of the first-pass part or None: every element at one scale), per step
NORMS = {'many': ((30.0, 0.2), (0.1, None), (30.0, 0.2), (0.1, None)),
         'deep': ((20.0, 5.0), (5.0, None))}

EXEMPT = ()


def tag(case):
  name, i = case
  h = HYPERS[name][i]
  return f'{name}_lr{h.lr:g}_k{h.clip:g}_w{h.wd:g}_u{h.warmup}_{"bf16" if h.bf16 else "f32"}'


def chunks(specs):
  return sum(-(-int(np.prod(s.shape)) // C) for s in specs)


def grad_dtypes(name, bf16):
  """Per tensor: is its gradient bfloat16?"""
  count = len(LISTS[name])
  if not bf16:
    return (False,) * count
  return tuple(i % 3 == 0 for i in range(count)) if name == 'many' else (True,) * count


def first_pass(name, grads):
  """The parts of a step's gradients in the chunks a kernel reads that never
  takes the second iteration of its loop: the chunks < kMaxBlocks of `many`
  (`chunk += gridDim.x`), the chunks < kThreads of `deep` (`k += kThreads`)."""
  if name == 'many':
    return list(grads[:BLOCKS])
  return [grads[0].reshape(-1)[:THREADS * C]]


def _rescaled(name, grads, whole, part):
  """The float64 draw `grads`, scaled to the global norm `whole` with the first-pass part at `part`."""
  if part is None:
    scale = whole / cases.global_norm(grads)
    return [g * scale for g in grads]
  out = [g.copy() for g in grads]
  head = first_pass(name, out)                        # views into `out`
  rest = np.sqrt(cases.global_norm(out) ** 2 - cases.global_norm(head) ** 2)
  head_scale = part / cases.global_norm(head)
  rest_scale = np.sqrt(whole ** 2 - part ** 2) / rest
  for g in out:
    g *= rest_scale
  for g in head:
    g *= head_scale / rest_scale
  return out


_INPUTS = {}


def inputs(name, bf16):
  """{'p': [array per tensor], 'g': [[array per tensor] per step], 'bf16': (bool
  per tensor)}, float32, made once and read-only; the gradients of the tensors
  flagged in 'bf16' hold bfloat16 values, the others do not."""
  key = (name, bool(bf16))
  if key not in _INPUTS:
    specs = LISTS[name]
    flags = grad_dtypes(name, bf16)
    rng = np.random.default_rng([29, sorted(LISTS).index(name), len(specs)])      # one draw per list: cases share it
    p = [(s.pscale * rng.standard_normal(s.shape)).astype(f32) for s in specs]
    g = []
    for step in range(STEPS[name]):
      raw = [rng.standard_normal(s.shape) for s in specs]
      whole, part = NORMS[name][step]
      g.append([x.astype(f32) for x in _rescaled(name, raw, whole, part)])
    g = [[bf16_round(x).reshape(x.shape) if flag else x for x, flag in zip(grads, flags)] for grads in g]
    for x in p + [x for grads in g for x in grads]:
      x.setflags(write=False)
    _INPUTS[key] = {'p': p, 'g': g, 'bf16': flags}
  return _INPUTS[key]


_REF = {}


def reference(case):
  """`adam_cases.restate` in float64 of a case: the definition, computed once."""
  if case not in _REF:
    name, i = case
    h = HYPERS[name][i]
    _REF[case] = cases.restate(inputs(name, h.bf16), h, LISTS[name], torch.float64)
  return _REF[case]
