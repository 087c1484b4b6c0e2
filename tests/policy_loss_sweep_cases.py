"""Shapes and seeded inputs of the sweep over every instantiation of the policy
loss kernels (csrc/policy_loss.hip): `policy_loss_kernel<T, W, NPER>` and
`policy_loss_grad_kernel<T, W, NPER>`.

Shared by tests/test_gpu_policy_loss_sweep.py (which runs the kernels at them)
and tests/test_policy_loss_sweep_host.py (which shows, without a GPU, that the
float32 definition stays inside both bars at every one of them).  Plain numpy.
The oracle is `tests.policy_loss_cases.reference64`.

Where the lists come from -- the kernels' own constants, read out of the source:

  * a wave of kWave = 64 lanes works on a row of logits; a workgroup has
    kWaves = 4 waves.  GEOMETRIES (N, T, drop) are chosen around that: (1, 2, 1)
    one kept row and one dropped row; (5, 2, 1) a second workgroup with one live
    wave in the forward (5 rows), 10 rows and 3 workgroups in the gradient;
    (2, 4, 1) kept = 3, so the forward's `row / kept` and the gradient's
    `row / steps` differ; (5, 1, 0) nothing dropped.
  * a group of `classes` logits occupies a segment of W lanes with NPER values
    per lane, chosen from `classes` alone (`width` below, the ladder of
    EMB_POLICY_BY_WIDTH); per rung the first class count (most padding lanes),
    the last (none), and the counts at which a slot j of NPER starts (lane 0
    alone), fills, and the one before.
  * a wave holds k = kSegs = kWave / W groups per iteration of the g0 loop, so
    per class count groups 1, k (one full iteration), k + 1 (a second iteration
    with one live segment) and 2 k + 1; k = 1 collapses that to 1, 2, 3.  The
    first class count of every rung also runs with no group axis (groups 0,
    dims=0).
  * a launch has at most kMaxBlocks workgroups: SWEEP = kMaxBlocks * kWaves rows
    are one pass of the grid-stride loop, PAST_* are the shapes that need a
    second one.
"""
import pathlib
import re

import numpy as np

from tests import policy_loss_cases as cases

f32 = np.float32
CSRC = pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc'
SOURCE = CSRC / 'policy_loss.hip'


def kernel_constants():
  text = SOURCE.read_text()
  return {name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1)) for name in ('kWave', 'kWaves', 'kMaxBlocks')}


def max_classes():
  return int(re.search(r'constexpr int kPolicyMaxClasses = (\d+);', (CSRC / 'policy_loss.h').read_text()).group(1))


def source_ladder():
  """EMB_POLICY_BY_WIDTH as the source spells it: [(last class count, W, NPER), ...],
  the closing `else` ending at kPolicyMaxClasses."""
  text = SOURCE.read_text()
  macro = text[text.index('#define EMB_POLICY_BY_WIDTH'):]
  macro = macro[:macro.index('while (0)')]
  rungs = [tuple(map(int, m)) for m in re.findall(r'if \(\(c\) <= (\d+)\) \{ CALL\((\d+), (\d+)\); \}', macro)]
  last = re.search(r'else \{ CALL\((\d+), (\d+)\); \}', macro)
  return rungs + [(max_classes(), int(last.group(1)), int(last.group(2)))]


K = kernel_constants()
WAVE = K['kWave']
MAX_CLASSES = 256
SWEEP = K['kMaxBlocks'] * K['kWaves']       # rows of one pass of either kernel's grid-stride loop


def width(classes):
  """(W, NPER) of the instantiation that runs `classes`."""
  assert 1 <= classes <= MAX_CLASSES, classes
  for W in (2, 4, 8, 16, 32, 64):
    if classes <= W:
      return W, 1
  return (64, 2) if classes <= 128 else (64, 4)


RUNGS = ((2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
CLASSES = {
    (2, 1): (1, 2),
    (4, 1): (3, 4),
    (8, 1): (5, 7, 8),
    (16, 1): (9, 15, 16),
    (32, 1): (17, 18, 31, 32),
    (64, 1): (33, 63, 64),
    (64, 2): (65, 96, 127, 128),
    (64, 4): (129, 191, 192, 193, 255, 256),
}
GEOMETRIES = ((1, 2, 1), (5, 2, 1), (2, 4, 1), (5, 1, 0))      # (N, T, drop)
ALONE = (5, 2, 1)                                               # where a row is run alone and the canaries stand
# (unimix, logit scale).  tests/test_policy_loss_sweep_host.py holds the float32
# definition inside both bars at every input under each of them.
SETTINGS = ((0.01, 1.0), (0.01, 30.0), (0.0, 1.0), (0.0, 5.0))
KINDS = ('f32', 'bf16')
ACTENT = cases.ACTENT
SEED = 11

# past one pass of the capped grid: T = 4 with one step dropped, so N (T - 1) kept
# rows and N T rows of logits both pass SWEEP
PAST_T, PAST_DROP = 4, 1
PAST_N = SWEEP // (PAST_T - PAST_DROP) + 2
PAST_SHAPES = ((3, 5), (1, 96))
PAST_SETTING = (0.01, 1.0)


def segments(rung):
  """kSegs: the groups a wave holds per iteration of the g0 loop."""
  return WAVE // rung[0]


def control_groups(classes):
  """The one group count per class count at which the composed path, the
  facade identities, the hit lanes and the output canaries run: k + 1, a last
  iteration with dead segments."""
  return segments(width(classes)) + 1


def groups_of(classes):
  rung = width(classes)
  k = segments(rung)
  some = {1, k, k + 1, 2 * k + 1}
  if classes == CLASSES[rung][0]:
    some.add(0)                               # no group axis
  return tuple(sorted(some))


def shapes(rung):
  """(groups, classes) of one rung; groups 0: dims=0."""
  return [(groups, classes) for classes in CLASSES[rung] for groups in groups_of(classes)]


def all_shapes():
  return [shape for rung in RUNGS for shape in shapes(rung)]


def cut_weight(n, t, drop, unimix, scale):
  """Whether a sweep input hands weight over as (N, T - drop) instead of (N, T):
  both layouts occur in every rung, for every geometry and for every setting."""
  return bool((GEOMETRIES.index((n, t, drop)) + SETTINGS.index((unimix, scale))) % 2) if (n, t, drop) in GEOMETRIES else False


def _frozen(d):
  for a in d.values():
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return d


def _rest(rng, n, t, drop):
  """adv, weight and gout as tests/test_gpu_policy_loss.py draws them: every
  fourth sequence ends early (weight 0 from the middle step on)."""
  adv = (2 * rng.standard_normal((n, t - drop))).astype(f32)
  weight = np.cumprod(np.where((np.arange(n)[:, None] % 4 == 1) & (np.arange(t) >= t // 2), 0, 0.997), 1)
  gout = rng.standard_normal((n, t - drop)).astype(f32)
  return adv, weight.astype(f32), gout


_DATA = {}


def data(groups, classes, n, t, drop, scale, kind='f32'):
  """Seeded inputs (bfloat16-rounded logits for kind 'bf16'), made once and left
  unchanged: logits (n, t, [groups,] classes), act (n, t[, groups]) from
  `policy_loss_cases.actions_of`, adv and gout (n, t - drop), weight (n, t)."""
  key = (groups, classes, n, t, drop, scale, kind)
  if key not in _DATA:
    rng = np.random.default_rng([SEED, groups, classes, n, t, int(scale * 10), drop])
    logits = cases.logits_of(n, t, groups, classes, scale, rng)
    if kind == 'bf16':
      logits = cases.bf16_round(logits)
    act = cases.actions_of(n, t, groups, classes, rng)
    adv, weight, gout = _rest(rng, n, t, drop)
    _DATA[key] = _frozen(dict(logits=logits, act=act, adv=adv, weight=weight, gout=gout, drop=drop,
                              dims=1 if groups else 0, ref={}))
  return _DATA[key]


def hit_data(classes, scale):
  """Every lane as the hit lane: N = classes + 2 rows of one step, nothing
  dropped, groups k + 1, row r's action in every group r - 1 (-1 .. classes: the
  first and the last row match no lane).  Every weight is 0.997, so that every
  row's gradient is live."""
  key = ('hit', classes, scale)
  if key not in _DATA:
    groups, n = control_groups(classes), classes + 2
    rng = np.random.default_rng([SEED, 1, groups, classes, int(scale * 10)])
    logits = cases.logits_of(n, 1, groups, classes, scale, rng)
    act = np.broadcast_to((np.arange(n, dtype=np.int32) - 1)[:, None, None], (n, 1, groups)).copy()
    adv, _, gout = _rest(rng, n, 1, 0)
    weight = np.full((n, 1), 0.997, f32)
    _DATA[key] = _frozen(dict(logits=logits, act=act, adv=adv, weight=weight, gout=gout, drop=0, dims=1, ref={}))
  return _DATA[key]


def reference(d, unimix, act=True):
  """`reference64` of an input, computed once per unimix (act False: no action
  term, the entropy's alone)."""
  key = (unimix, act)
  if key not in d['ref']:
    d['ref'][key] = cases.reference64(d['logits'], d['act'] if act else None, d['adv'], d['weight'], ACTENT, unimix,
                                      d['dims'], d['drop'], d['gout'])
  return d['ref'][key]


def ratios(d, out, grad, ref, bf16=False):
  """(forward, gradient) of a run as shares of the bars of
  tests/test_gpu_policy_loss.py; a dropped step's gradient must be zeros."""
  kept = d['logits'].shape[1] - d['drop']
  forward = max(cases.forward_ratio(out[key], ref[key]) for key in ('loss', 'logpi', 'ent'))
  grad = np.asarray(grad)
  assert not grad[:, kept:].any()
  s = cases.row_scale(d['gout'], d['weight'][:, :kept], d['adv'], ACTENT)
  return forward, cases.grad_ratio(grad[:, :kept], ref['grad'][:, :kept], s, bf16)
