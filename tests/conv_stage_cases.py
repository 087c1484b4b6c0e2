"""Shapes and seeded inputs of the conv-stage tests (`nets.pool_norm_act`,
`nets.norm_act_upsample`), the fixture's cases (tests/golden/conv_stage.npz) and a
numpy restatement of both stages with closed-form gradients, the equal split
among tied maxima included.

Built on `tests.norm_act_cases.evaluate`: a stage is a pool or a repeat around
that module's row, and its bars -- `out_ratio`, `grad_ratio`, `sum_ratio`, each
<= 1.0 against the float64 run, with the same bfloat16 allowance -- are the bars
here.  Shared by `tools/gen_conv_stage_golden.py` and the tests; the host test
holds `reference` against the fixture, central differences and a hand-written
tie example before the GPU tests rely on it.
"""
import collections

import numpy as np

from tests import norm_act_cases as norms
from tests.norm_act_cases import ACTS, EPS, IMPLS, SCALES, SUM_ROWS, bf16_round, digest, present  # noqa: F401

f32 = np.float32

STAGES = ('pool', 'upsample')
MAX_UNITS = 1024
# the builder's lanes-per-pixel ladder (csrc/conv_stage.h): 8, 16, 32, 64 lanes up
# to these widths, then 16 values per lane instead of 8 up to MAX_UNITS
LADDER = (64, 128, 256, 512)
# the vector widths (1 .. 3, 7 .. 9), every step of the ladder and the steps either side
UNITS = tuple(sorted({1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 1024}
                     | {u + d for u in LADDER for d in (-1, 0, 1)}))
SHAPES = ((1, 2, 2), (3, 4, 6))                  # (images, H, W) of x
# What a launch covers in one pass and the rows of partial sums a gradient launch
# leaves (csrc/conv_stage.h): 2048 and 1024 workgroups of 256 / lanes pixels.
MAX_BLOCKS, MAX_PARTIALS = 2048, 1024

Case = collections.namedtuple('Case', 'stage height width units impl act affine eps scale')
# the fixture: 3 images, four widths x three image sizes, the stage, impl,
# activation and the other options in turn (the larger sizes mostly pool: the
# repeated output is 16 times the pooled one)
GOLDEN_IMAGES, GOLDEN_UNITS, GOLDEN_SIZES = 3, (1, 3, 65, 257), ((2, 2), (2, 6), (4, 4))
_STAGE_OF = ('pup', 'upu', 'puu', 'upp')
_TURNS = tuple((affine, eps, scale) for affine in (True, False) for eps in EPS for scale in SCALES)
CASES = tuple(Case({'p': 'pool', 'u': 'upsample'}[_STAGE_OF[i][j]], h, w, units, IMPLS[(i + j) % 2],
                   ACTS[(3 * i + j) % 4], *_TURNS[(5 * i + 3 * j) % len(_TURNS)])
              for i, units in enumerate(GOLDEN_UNITS) for j, (h, w) in enumerate(GOLDEN_SIZES))


def tag(case):
  c = CASES[case]
  return (f'c{case}_{c.stage}_{c.height}x{c.width}x{c.units}_{c.impl}_{c.act}_{"affine" if c.affine else "plain"}'
          f'_e{c.eps:g}_s{c.scale:g}')


def lanes(units):
  return 8 if units <= 64 else 16 if units <= 128 else 32 if units <= 256 else 64


def out_shape(stage, shape):
  n, h, w, c = shape
  return (n, h // 2, w // 2, c) if stage == 'pool' else (n, 2 * h, 2 * w, c)


def windows(big):
  """(N, 2h, 2w, C) -> (N h w, 4, C): the 2x2 window of every pixel of the smaller
  tensor, positions in the order (0,0), (0,1), (1,0), (1,1)."""
  n, h, w, c = big.shape
  return big.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4, c)


def unwindows(win, shape):
  n, h, w, c = shape
  return win.reshape(n, h // 2, w // 2, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(shape)


def inputs_of(stage, images, height, width, units, impl, affine, scale, rng, ties=False):
  """x (images, H, W, C), gout in the shape of the result, scale / shift as
  `norms.inputs_of`; all float32.  The Norm rows are drawn by `norms.inputs_of`
  (what its bars were worked out for): for the upsample they are x; for the pool
  they are the window maxima, at a random position of each window and channel,
  and the other three positions are lower by scale * (0.1 + |N(0, 1)|), so no
  window has a tie.  `ties`: every value is -scale / 2, 0 or scale / 2
  instead, so windows tie two, three and four ways."""
  shape = (images, height, width, units)
  small = out_shape('pool', shape) if stage == 'pool' else shape
  rows = small[0] * small[1] * small[2]
  base = norms.inputs_of(rows, units, impl, affine, scale, rng)
  out = {'scale': base['scale'], 'shift': base['shift']}
  if stage == 'pool':
    drop = (0.1 + np.abs(rng.standard_normal((rows, 4, units)))) * scale
    winner = rng.integers(0, 4, (rows, units))
    drop[np.arange(4)[None, :, None] == winner[:, None, :]] = 0
    win = base['x'][:, None, :].astype(np.float64) - drop
    if ties:
      win = scale * rng.integers(-1, 2, (rows, 4, units)) / 2
    out['x'] = unwindows(win.astype(f32), shape)
    out['gout'] = base['gout'].reshape(small)
  else:
    out['x'] = base['x'].reshape(shape)
    out['gout'] = rng.standard_normal(out_shape(stage, shape)).astype(f32)
  return out


def inputs(case):
  c = CASES[case]
  return inputs_of(c.stage, GOLDEN_IMAGES, c.height, c.width, c.units, c.impl, c.affine, c.scale,
                   np.random.default_rng([case, c.units, c.height]))


def reference(stage, x, scale, shift, impl, act, eps, gout=None, dtype=np.float64):
  """The stage in `dtype` over float32 (or bfloat16-rounded) inputs.
    pool      rssm.py:239-240, x.reshape((B, H // 2, 2, W // 2, 2, C)).max((2, 4)),
              then `norms.evaluate`; the gradient g of a pooled value goes to the
              positions of its window that equal it, g / count each (torch.amax,
              jax's reduce_max), 0 to the others
    upsample  `norms.evaluate`, then rssm.py:336, x.repeat(2, -2).repeat(2, -3);
              the gradient of a row is the sum of its four copies'
  Returns a dict: out, and with gout dx, dscale, dshift, dscale_abs, dshift_abs,
  and `s` (Norm rows,): `norms.row_scale` of the gradient that reaches the row
  (for the upsample the float64 sum of the four gout rows)."""
  x = np.asarray(x, dtype)
  n, h, w, c = x.shape
  if stage == 'pool':
    rows = x.reshape((n, h // 2, 2, w // 2, 2, c)).max((2, 4)).reshape(-1, c)
    reach = None if gout is None else np.asarray(gout, dtype).reshape(-1, c)
  else:
    rows = x.reshape(-1, c)
    reach = None if gout is None else windows(np.asarray(gout, dtype)).sum(1)
  res = norms.evaluate(rows, scale, shift, impl, act, eps, reach, dtype)
  small = res['out'].reshape(out_shape('pool', x.shape) if stage == 'pool' else x.shape)
  result = {'out': small if stage == 'pool' else small.repeat(2, -2).repeat(2, -3)}
  if gout is None:
    return result
  if stage == 'pool':
    win = windows(x)
    hit = win == rows[:, None, :]
    count = hit.sum(1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
      dx = unwindows(np.where(hit, res['dx'][:, None, :] / count, 0), x.shape)
  else:
    dx = res['dx'].reshape(x.shape)
  result.update({k: res[k] for k in ('dscale', 'dshift', 'dscale_abs', 'dshift_abs')})
  result.update(dx=dx, s=norms.row_scale(np.asarray(reach, np.float64), scale, res['rstd']))
  return result


def ratios(stage, want, out, dx=None, dscale=None, dshift=None, bf16=False, sums=False):
  """The worst share of each bar: `out` and `dx` against `norms.out_ratio` and
  `norms.grad_ratio` (a window of dx belongs to one Norm row and takes its `s`),
  the column sums against `norms.sum_ratio` where `sums` (SUM_ROWS rows or more)."""
  found = {'out': norms.out_ratio(out, want['out'], bf16)}
  units = want['out'].shape[-1]
  as_rows = (lambda a: windows(np.asarray(a)).reshape(-1, 4 * units)) if stage == 'pool' else (
      lambda a: np.asarray(a).reshape(-1, units))
  if dx is not None:
    found['dx'] = norms.grad_ratio(as_rows(dx), as_rows(want['dx']), want['s'], bf16)
  if sums and dscale is not None:
    found['dscale'] = norms.sum_ratio(dscale, want['dscale'], want['dscale_abs'])
  if sums and dshift is not None:
    found['dshift'] = norms.sum_ratio(dshift, want['dshift'], want['dshift_abs'])
  return found
