"""Shapes and seeded inputs of the sweep over every instantiation of the OneHot
KL kernels (csrc/onehot_kl.hip): `onehot_kl_kernel<T, W, NPER>` and
`onehot_kl_grad_kernel<T, W, NPER>`.

Shared by tests/test_gpu_rssm_kl_sweep.py (which runs the kernels at them),
tests/test_rssm_kl_sweep_host.py (which shows, without a GPU, that the float32
definition stays inside both bars at every one of them and that no row's kl
sits at free_nats) and tools/bench_rssm_kl.py (the accuracy record).  Plain
numpy.

Where the lists come from -- the kernels' own constants, read out of the source:

  * a wave of kWave = 64 lanes works on a row; a workgroup has kWaves = 4 waves,
    so ROWS = (1, kWaves + 1): one row, and a second workgroup with one live
    wave.  Row 0 is the `logits_of` "near" row whose kl is below free_nats = 1.
  * a group of `classes` logits occupies a segment of W lanes with NPER values
    per lane, chosen from `classes` alone (`width` below, the ladder of
    EMB_ONEHOT_BY_WIDTH); per rung the first class count (most padding lanes),
    the last (none), the counts at which a slot j of NPER starts (lane 0 alone),
    fills, and the one before, and every size the reference ships
    (dreamerv3/configs.yaml: 4, 16, 24, 32, 48, 64, 96 classes, stoch 32).
  * a wave holds k = kSegs = kWave / W groups per iteration of the g0 loop, so
    per rung stoch 1, k (one full iteration), k + 1 (a second iteration with one
    live segment) and 2 k + 1; k = 1 collapses that to 1, 2, 3.  The shipped
    class counts also run at the shipped stoch, 32.
"""
import pathlib
import re

import numpy as np

from tests import rssm_kl_cases as cases

f32 = np.float32
SOURCE = pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc' / 'onehot_kl.hip'


def kernel_constants():
  text = SOURCE.read_text()
  return {name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1)) for name in ('kWave', 'kWaves', 'kMaxBlocks')}


def source_ladder():
  """EMB_ONEHOT_BY_WIDTH as the source spells it: [(last class count, W, NPER), ...],
  the closing `else` ending at kOneHotMaxClasses."""
  text = SOURCE.read_text()
  macro = text[text.index('#define EMB_ONEHOT_BY_WIDTH'):]
  macro = macro[:macro.index('while (0)')]
  rungs = [tuple(map(int, m)) for m in re.findall(r'if \(\(c\) <= (\d+)\) \{ CALL\((\d+), (\d+)\); \}', macro)]
  last = re.search(r'else \{ CALL\((\d+), (\d+)\); \}', macro)
  header = (SOURCE.parent / 'onehot_kl.h').read_text()
  most = int(re.search(r'constexpr int kOneHotMaxClasses = (\d+);', header).group(1))
  return rungs + [(most, int(last.group(1)), int(last.group(2)))]


K = kernel_constants()
WAVE = K['kWave']
MAX_CLASSES = 256


def width(classes):
  """(W, NPER) of the instantiation that runs `classes`."""
  assert 1 <= classes <= MAX_CLASSES, classes
  for W in (2, 4, 8, 16, 32, 64):
    if classes <= W:
      return W, 1
  return (64, 2) if classes <= 128 else (64, 4)


RUNGS = ((2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
SHIPPED_CLASSES = (4, 16, 24, 32, 48, 64, 96)
SHIPPED_STOCH = 32
# 5, 24, 32, 64, 96 and 256 also run (at one stoch each) in rssm_kl_cases.FUSED_SHAPES;
# the shipped ones of them are here once more for stoch = k + 1
CLASSES = {
    (2, 1): (1, 2),
    (4, 1): (3, 4),
    (8, 1): (7, 8),
    (16, 1): (9, 15, 16),
    (32, 1): (17, 24, 31, 32),
    (64, 1): (33, 48, 63, 64),
    (64, 2): (65, 96, 127, 128),
    (64, 4): (129, 191, 192, 193, 255),
}
ROWS = (1, K['kWaves'] + 1)
FREE_NATS = cases.FREE_NATS
# (unimix, logit scale): with unimix = 0 the scales at which the float32
# definition holds the gradient bar (rssm_kl_cases.GRAD_SCALES_NO_UNIMIX)
SETTINGS = ((0.01, 1.0), (0.01, 5.0)) + tuple((0.0, s) for s in cases.GRAD_SCALES_NO_UNIMIX)
KINDS = ('f32', 'bf16')
FREE_MARGIN = 1e-4          # no row's float64 kl is this close to free_nats = 1
SEED = 7


def segments(rung):
  """kSegs: the groups a wave holds per iteration of the g0 loop."""
  return WAVE // rung[0]


def stochs(classes):
  k = segments(width(classes))
  some = {1, k, k + 1, 2 * k + 1}
  if classes in SHIPPED_CLASSES:
    some.add(SHIPPED_STOCH)
  return tuple(sorted(some))


def shapes(rung):
  """(stoch, classes) of one rung."""
  return [(stoch, classes) for classes in CLASSES[rung] for stoch in stochs(classes)]


def all_shapes():
  return [shape for rung in RUNGS for shape in shapes(rung)]


def control_stoch(classes):
  """The one stoch per class count at which the composed path, the self-KL and
  the output canaries run: k + 1, a last iteration with dead segments."""
  return segments(width(classes)) + 1


_DATA = {}


def data(stoch, classes, rows, scale, kind='f32'):
  """Seeded logits (bfloat16-rounded for kind 'bf16') and upstream gradients,
  made once and left unchanged: dict of post, prior (rows, stoch, classes) and
  g_dyn, g_rep (rows,), float32."""
  key = (stoch, classes, rows, scale, kind)
  if key not in _DATA:
    rng = np.random.default_rng([SEED, stoch, classes, rows, int(scale * 10)])
    post, prior = cases.logits_of(rows, stoch, classes, scale, rng)
    if kind == 'bf16':
      post, prior = cases.bf16_round(post), cases.bf16_round(prior)
    g_dyn, g_rep = rng.standard_normal((2, rows)).astype(f32)
    for a in (post, prior, g_dyn, g_rep):
      a.setflags(write=False)
    _DATA[key] = dict(post=post, prior=prior, g_dyn=g_dyn, g_rep=g_rep)
  return _DATA[key]
