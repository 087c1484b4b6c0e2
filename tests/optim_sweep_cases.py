"""Tensor lists that take the optimizer kernels (csrc/optim.hip) past the first
iteration of three loops no list of `tests.optim_cases.LISTS` reaches, sized by
the kernels' own constants read out of the source:

  * `chunk += gridDim.x` in the norms and the update kernel needs more than
    kMaxBlocks chunks; in the update kernel it is also the only way a workgroup
    meets a second tensor and has to replace its cached AGC scale;
  * `k += kThreads`, a workgroup's sum of its tensor's partials, needs a tensor of
    more than kThreads chunks;
  * `k += kMetricThreads` in the metrics kernel needs more than kMetricThreads
    chunks in all.

`many` is 2 kMaxBlocks + 3 tensors of 1 to 5 elements, one chunk each: chunk i and
chunk i + kMaxBlocks land in the same workgroup, and the tensors behind them
differ in AGC regime (clipped, then not clipped; the last three have pnorm below
pmin).  `deep` is a tensor of kThreads + 2 chunks with a ragged last one, a small
tensor behind it (first_chunk != 0) and a second large one as a view at element
offset 1 of both p and g (head = 3: vectors behind scalars across many chunks).

The lists are not in `optim_cases.LISTS`: the fixture is indexed by case number.
The oracle is `optim_cases.reference64`, which the host test holds against the
reference's own float64 run.  Plain numpy.
"""
import pathlib
import re

import numpy as np

from tests import optim_cases as cases
from tests.optim_cases import C, Spec

f32 = np.float32
SOURCE = pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc' / 'optim.hip'


def kernel_constants():
  text = SOURCE.read_text()
  return {name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))
          for name in ('kThreads', 'kMetricThreads', 'kMaxBlocks')}


K = kernel_constants()
BLOCKS = K['kMaxBlocks']
DEEP = (K['kThreads'] + 1) * C + 7          # kThreads + 2 chunks, the last one of 7 elements


def _small(i, **kw):
  return Spec((1 + i % 5,) if i % 2 else (1, 1 + i % 5), **kw)           # 1-D and 2-D: a mixed decay mask


LISTS = {
    'many': tuple(_small(i, gscale=10.0) for i in range(BLOCKS)) +
            tuple(_small(i, gscale=0.01) for i in range(BLOCKS, 2 * BLOCKS)) +
            tuple(_small(i, pscale=1e-5, gscale=1e-6) for i in range(2 * BLOCKS, 2 * BLOCKS + 3)),
    'deep': (Spec((DEEP,), gscale=0.5), Spec((3,)), Spec((DEEP,), 1, 1, gscale=0.5)),
}
STEPS = {'many': cases.STEPS, 'deep': 2}
HYPERS = {'many': cases.COVER, 'deep': (cases.COVER[0], cases.COVER[4])}      # deep: float32 and bfloat16 gradients, agc on
CASES = tuple((name, i) for name in LISTS for i in range(len(HYPERS[name])))


def tag(case):
  name, i = case
  h = HYPERS[name][i]
  return f'{name}_lr{h.lr:g}_a{h.agc:g}_w{h.wd:g}_n{int(h.nesterov)}_u{h.warmup}_{"bf16" if h.bf16 else "f32"}'


def chunks(specs):
  return sum(-(-int(np.prod(s.shape)) // C) for s in specs)


_INPUTS = {}


def inputs(name, bf16):
  """{'p': [array per tensor], 'g': [[array per tensor] per step]}, float32, made
  once and left unchanged; the gradients of a bfloat16 case are bfloat16 values.
  Every element is scale * (z + sign(z) / 2), z ~ N(0, 1): no element is so small
  that a tensor of one element leaves the AGC regime its scales put it in."""
  key = (name, bool(bf16))
  if key not in _INPUTS:
    specs = LISTS[name]
    rng = np.random.default_rng([23, sorted(LISTS).index(name), len(specs)])

    def draw(shape, scale):
      z = rng.standard_normal(shape)
      return (scale * (z + 0.5 * np.sign(z))).astype(f32)

    p = [draw(s.shape, s.pscale) for s in specs]
    g = [[draw(s.shape, s.gscale) for s in specs] for _ in range(STEPS[name])]
    if bf16:
      g = [[cases.bf16_round(x).reshape(x.shape) for x in step] for step in g]
    for x in p + [x for step in g for x in step]:
      x.setflags(write=False)
    _INPUTS[key] = {'p': p, 'g': g}
  return _INPUTS[key]


_REF = {}


def reference(case):
  """`optim_cases.reference64` of a case, computed once."""
  if case not in _REF:
    name, i = case
    h = HYPERS[name][i]
    _REF[case] = cases.reference64(inputs(name, h.bf16), h, LISTS[name])
  return _REF[case]


def worst_ratios(got_all, want_all):
  """Per quantity, the worst share of its bar over every step and every element."""
  worst = {}
  for got, want in zip(got_all, want_all):
    for key in ('p', 'nu', 'mu'):
      bar = cases.ratio_nu if key == 'nu' else cases.ratio
      flat = lambda arrays: np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
      worst[key] = max(worst.get(key, 0.0), bar(flat(got[key]), flat(want[key])))
    worst['metrics'] = max(worst.get('metrics', 0.0), cases.ratio(got['metrics'], want['metrics']))
  return worst
