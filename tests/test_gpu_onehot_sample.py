"""`embodied_amd.outs.OneHot.sample` / `pred` and `Categorical.sample`: the draw of
dreamerv3/rssm.py:87, 100 and dreamerv3/agent.py:18, 126, 192 on the kernels of
csrc/onehot_sample.hip and as composed torch ops, against the restatements of
tests/onehot_sample_cases.py (which the host test holds against the reference's
own run, tests/golden/onehot_sample.npz, and the Random123 known answers).  Need
a GPU.

The acceptance rule of an index k drawn with the uniform u: C64[k - 1] - tol <=
u < C64[k] + tol with C64 the float64 CDF of the same (possibly bfloat16-rounded)
logits and tol = (classes + 8) 2^-23 -- at most `classes` float32 additions of
terms that sum to 1, plus a few ulps for the softmax; p[k] > 0 always.  A draw
within tol of a boundary may take either neighbour; the share of such draws is
asserted below 5 %, so the rule cannot hide a wrong kernel.  The gradient's bar:
each element within 1e-5 s (1 + |want| / s) of the float64 autograd, s =
(1 - unimix) max |g| over the group (a bfloat16 gradient: plus 2^-8 |want|).
tools/onehot_sample_accuracy.py records the worst ratios in
profiles/onehot_sample_accuracy.txt."""
import pathlib

import numpy as np
import pytest
import torch

from embodied_amd.outs import Categorical, OneHot, onehot_sample_launches, philox_uniform   # fails without the feature
from tests import onehot_sample_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'onehot_sample.npz'
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
# every shape on both paths, 257 classes on the composed path alone
SHAPE_PATHS = [pytest.param(shape, fused, id=f'{shape[0]}x{shape[1]}-{"fused" if fused else "composed"}')
               for shape in cases.SHAPES for fused in (True, False) if not (fused and shape[1] > 256)]
SEED, OFFSET = 0x9e3779b97f4a7c15, 2 ** 33 + 5                      # both above 2^32


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def _tensor(values, kind='f32'):
  t = torch.from_numpy(np.ascontiguousarray(values)).cuda()
  return t if kind == 'f32' or not t.dtype.is_floating_point else t.to(torch.bfloat16)


def _host(t):
  return t.detach().float().cpu().numpy()


_DATA = {}


def _data(groups, classes, rows, scale, kind='f32'):
  """Seeded logits (bfloat16-rounded for kind 'bf16'), uniforms and upstream
  gradient, made once and left unchanged.  Uniforms: the stream's grid, with 0,
  1 - 2^-24 and values exactly on a boundary of the float32 CDF planted in the
  first groups (`planted` marks them)."""
  key = (groups, classes, rows, scale, kind)
  if key not in _DATA:
    rng = np.random.default_rng([groups, classes, rows, int(scale * 10), kind == 'bf16'])
    x = cases.logits_of(rows, groups, classes, scale, rng)
    if kind == 'bf16':
      x = cases.bf16_round(x)
    lead = x.shape[:-1]
    count = int(np.prod(lead))
    u = (rng.integers(0, 2 ** 24, count).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    planted = np.zeros(count, bool)
    cdf = cases.define32(x, 0.0)['cdf'].reshape(count, classes)
    special = [0.0, 1 - 2.0 ** -24] + [float(cdf[i, (i * 7) % classes] / cdf[i, -1]) for i in range(2, min(count, 6))]
    for i, value in enumerate(special[:count]):
      if 0 <= value < 1:
        u[i], planted[i] = value, True
    g = cases.gout_of(x.shape, rng)
    if kind == 'bf16':
      g = cases.bf16_round(g)
    d = dict(logits=x, u=u.reshape(lead), planted=planted.reshape(lead), gout=g, dims=1 if groups else 0, p64={})
    for a in d.values():
      if isinstance(a, np.ndarray):
        a.setflags(write=False)
    _DATA[key] = d
  return _DATA[key]


def _p64(d, unimix):
  if unimix not in d['p64']:
    d['p64'][unimix] = cases.probs64(d['logits'], unimix)
  return d['p64'][unimix]


def _onehot_index(onehot):
  """The index a one-hot row encodes, after checking it holds exactly one 1 and zeros."""
  assert ((onehot == 0) | (onehot == 1)).all()
  assert (onehot.sum(-1) == 1).all()
  return onehot.argmax(-1)


def _sample(d, unimix, fused, kind='f32', **how):
  """OneHot.sample over `d` -> (index, onehot) as numpy, the one-hot checked bit for bit."""
  x = _tensor(d['logits'], kind)
  out = OneHot(x, unimix, fused=fused).sample(**how)
  assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
  onehot = _host(out)
  return _onehot_index(onehot), onehot


def _check_draws(d, unimix, index, u, tol):
  """The acceptance rule over every group; returns (near, counted) of the draws that were not planted."""
  ok, near = cases.accepted(_p64(d, unimix), u, index, tol)
  assert ok.all(), (np.argwhere(~ok)[:4], index[~ok][:4], u[~ok][:4])
  free = ~d['planted']
  return int(near[free].sum()), int(free.sum())


def test_stream_is_the_numpy_philox_bit_for_bit():
  for seed in (SEED, 2 ** 32 + 1):
    for offset in (0, OFFSET):
      for first in (0, 1, 2 ** 32 - 1, 2 ** 32):
        for count in (1, 1000):
          got = philox_uniform(seed, offset, first, count, 'cuda')
          assert got.dtype == torch.float32 and got.shape == (count,)
          assert np.array_equal(_host(got), cases.uniforms(seed, offset, first, count)), (seed, offset, first, count)
  assert philox_uniform(SEED, 0, 0, 0, 'cuda').shape == (0,)


@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_seeded_draw_is_the_draw_of_its_uniforms(shape, fused):
  """`sample(seed, offset)` equals `sample(uniform=the stream's values)` exactly,
  and `Categorical.sample` returns `OneHot.sample`'s index."""
  groups, classes = shape
  for rows, kind, unimix in ((1, 'f32', 0.0), (3, 'bf16', 0.01), (37, 'f32', 0.01)):
    d = _data(groups, classes, rows, 1.0, kind)
    count = d['u'].size
    u = cases.uniforms(SEED, OFFSET, 0, count).reshape(d['u'].shape)
    seeded, onehot = _sample(d, unimix, fused, kind, seed=SEED, offset=OFFSET)
    given, again = _sample(d, unimix, fused, kind, uniform=_tensor(u))
    assert np.array_equal(onehot, again) and np.array_equal(seeded, given)
    ok, _ = cases.accepted(_p64(d, unimix), u, seeded, cases.tol_of(classes))
    assert ok.all()
    act = Categorical(_tensor(d['logits'], kind), unimix, dims=d['dims'], fused=fused).sample(SEED, OFFSET)
    assert act.dtype == torch.int32 and act.shape == d['u'].shape and not act.requires_grad
    assert np.array_equal(act.cpu().numpy(), seeded)


@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_index_is_inside_the_acceptance_rule(shape, fused):
  """Rows 1, 3 and 37, every logit scale, unimix 0 and 0.01, float32 and
  bfloat16-rounded logits, supplied uniforms with 0, 1 - 2^-24 and exact float32
  CDF boundaries among them: every index is accepted, the one-hot holds one 1 at
  it, and few of the draws lie near a boundary."""
  groups, classes = shape
  tol = cases.tol_of(classes)
  near = counted = 0
  for rows in cases.ROWS:
    for scale in cases.SCALES:
      for unimix in cases.UNIMIX:
        for kind in ('f32', 'bf16'):
          d = _data(groups, classes, rows, scale, kind)
          index, _ = _sample(d, unimix, fused, kind, uniform=_tensor(d['u']))
          a, b = _check_draws(d, unimix, index, d['u'], tol)
          near, counted = near + a, counted + b
  print(f'{shape} fused={fused}: {near} of {counted} draws within tol of a boundary')
  if classes > 1:
    assert counted > 0 and near < 0.05 * counted


@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_pred_is_the_fixtures_argmax(golden, shape, fused):
  """Every case of the fixture at this shape: the one-hot of the reference's own
  `Categorical.pred()`, the planted tie broken towards the first class."""
  seen = 0
  for case, c in enumerate(cases.CASES):
    if (c.groups, c.classes) != shape:
      continue
    name = cases.tag(case)
    inp = cases.inputs(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(inp))
    for kind in ('f32', 'bf16'):
      if kind == 'bf16' and not np.array_equal(cases.bf16_round(inp['logits']).argmax(-1), golden[f'argmax_{name}']):
        continue                                                   # rounding made a new tie: another question
      out = OneHot(_tensor(inp['logits'], kind), c.unimix, fused=fused).pred()
      assert out.dtype == (torch.float32 if kind == 'f32' else torch.bfloat16)
      assert np.array_equal(_onehot_index(_host(out)), golden[f'argmax_{name}']), (name, kind)
      seen += 1
  assert seen >= 10


@PATHS
def test_the_rows_that_follow_do_not_change_a_draw(fused):
  for groups, classes, kind in ((3, 18, 'f32'), (33, 2, 'bf16'), (3, 96, 'f32'), (0, 64, 'bf16')):
    d = _data(groups, classes, 37, 1.0, kind)
    x = _tensor(d['logits'], kind)
    whole = OneHot(x, 0.01, fused=fused).sample(SEED, OFFSET)
    for n in (1, 18):
      part = OneHot(x[:n].contiguous(), 0.01, fused=fused).sample(SEED, OFFSET)
      assert torch.equal(part, whole[:n])                          # (no group axis: the rows are the groups)


def test_dtype_and_path_do_not_change_a_draw():
  """float32 and bfloat16 views of bfloat16-representable logits, and the fused
  and the composed path, give the same indices apart from draws within tol of a
  boundary; two runs give identical bits."""
  different = counted = 0
  for groups, classes in cases.FUSED_SHAPES:
    tol = cases.tol_of(classes)
    for scale, unimix in ((1.0, 0.0), (5.0, 0.01), (1e4, 0.0)):
      d = _data(groups, classes, 37, scale, 'bf16')
      u = cases.uniforms(SEED, OFFSET, 0, d['u'].size).reshape(d['u'].shape)
      _, near = cases.accepted(_p64(d, unimix), u, np.zeros(u.shape, np.int64), tol)
      runs = {(kind, fused): _sample(d, unimix, fused, kind, seed=SEED, offset=OFFSET)[0]
              for kind in ('f32', 'bf16') for fused in (True, False)}
      base = runs['f32', True]
      for key, index in runs.items():
        assert np.array_equal(index[~near], base[~near]), (groups, classes, scale, key)
        different += int((index != base).sum())
      counted += u.size
      again = _sample(d, unimix, True, 'f32', seed=SEED, offset=OFFSET)[0]
      assert np.array_equal(again, base)
  print(f'{different} differences between the four (dtype, path) runs over {counted} groups')
  assert different < 0.05 * counted


@PATHS
def test_seed_and_offset_change_the_draws(fused):
  x = torch.zeros(1024, 32, device='cuda')
  draw = lambda seed, offset: _onehot_index(_host(OneHot(x, 0.0, fused=fused).sample(seed, offset)))
  base = draw(SEED, OFFSET)
  assert np.array_equal(base, draw(SEED, OFFSET))
  for seed, offset in ((SEED, OFFSET + 1), (SEED + 1, OFFSET), (SEED, OFFSET + 2 ** 32), (SEED + 2 ** 32, OFFSET)):
    assert (draw(seed, offset) != base).sum() > 512, (seed, offset)
  assert np.bincount(base, minlength=32).min() > 0


@PATHS
@pytest.mark.parametrize('classes', cases.STAT_CLASSES)
@pytest.mark.parametrize('unimix', cases.UNIMIX)
def test_statistics(classes, unimix, fused):
  """One row of probabilities over 65 536 groups: Pearson's chi-square below the
  1 - 10^-6 quantile (the host test shows the seeds pass under the restatement)."""
  row = cases.stat_logits(classes)
  x = _tensor(row).expand(cases.STAT_GROUPS, classes).contiguous()
  index = Categorical(x, unimix, fused=fused).sample(cases.STAT_SEEDS[classes], cases.STAT_OFFSET).cpu().numpy()
  assert index.min() >= 0 and index.max() < classes
  stat, dof = cases.chi_square(np.bincount(index, minlength=classes), cases.probs64(row, unimix))
  bound = cases.chi_square_bound(dof)
  print(f'{classes} classes, unimix {unimix}, fused={fused}: chi-square {stat:.1f} on {dof} dof, bound {bound:.1f}')
  assert stat < bound


def _gradient(d, unimix, fused, kind, seed=SEED, pred=False):
  x = _tensor(d['logits'], kind).requires_grad_()
  dist = OneHot(x, unimix, fused=fused)
  out = dist.pred() if pred else dist.sample(seed, OFFSET)
  assert out.requires_grad
  (out * _tensor(d['gout'], kind)).sum().backward()
  assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
  return _host(x.grad)


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_gradient(shape, fused, kind):
  """The straight-through gradient against the float64 autograd of the reference
  expression, zero rows of g included; it does not depend on the seed nor on
  sample / pred."""
  groups, classes = shape
  worst = 0.0
  for i, rows in enumerate(cases.ROWS):
    for j, unimix in enumerate(cases.UNIMIX):
      for scale in (cases.SCALES[(i + j) % 5], cases.SCALES[(i + j + 2) % 5], 1e4):
        d = _data(groups, classes, rows, scale, kind)
        assert not d['gout'].reshape(-1, classes)[0].any()
        grad = _gradient(d, unimix, fused, kind)
        want = cases.restate(d['logits'], unimix, np.zeros(d['u'].shape, np.int64), d['gout'])['grad']
        ratio = cases.grad_ratio(grad, want, cases.group_scale(d['gout'], unimix), kind == 'bf16')
        assert ratio <= 1.0, (rows, unimix, scale, ratio)
        assert not grad.reshape(-1, classes)[0].any()              # a zero row of g: exactly zero
        worst = max(worst, ratio)
        if rows == 3:
          assert np.array_equal(grad, _gradient(d, unimix, fused, kind, seed=SEED + 1))
          assert np.array_equal(grad, _gradient(d, unimix, fused, kind, pred=True))
  print(f'{shape} {kind} fused={fused}: gradient {worst:.3g} of its bar')


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_fused_gradient_against_the_composed_autograd(kind):
  """Under the same bar.  The composed side runs on the float32 view of the same
  (bfloat16-representable) values, so the one rounding the bar allows a bfloat16
  gradient is the fused side's own."""
  for groups, classes in cases.FUSED_SHAPES:
    d = _data(groups, classes, 37, 5.0, kind)
    fused, composed = _gradient(d, 0.01, True, kind), _gradient(d, 0.01, False, 'f32')
    s = cases.group_scale(d['gout'], 0.01)
    assert cases.grad_ratio(fused, composed, s, kind == 'bf16') <= 1.0, (groups, classes)


@PATHS
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_poisoned_groups(fused, kind):
  """One group each with a NaN, a +inf and nothing but -inf among valid ones:
  index -1, a NaN one-hot and a NaN gradient there, every other group bit-identical
  to the run without them."""
  for groups, classes in ((3, 5), (3, 18), (3, 96)):
    d = _data(groups, classes, 37, 1.0, kind)
    dirty = d['logits'].copy()
    dirty[2, 1, 3], dirty[5, 0, 0], dirty[36, 2, :] = np.nan, np.inf, -np.inf
    dirty[7, 1, 2] = -np.inf                                       # a single -inf: a class of probability 0 (or unimix / classes)
    bad = np.zeros(dirty.shape[:-1], bool)
    bad[2, 1] = bad[5, 0] = bad[36, 2] = True
    for unimix in cases.UNIMIX:
      results = {}
      for name, logits in (('clean', d['logits']), ('dirty', dirty)):
        x = _tensor(logits, kind).requires_grad_()
        dist = OneHot(x, unimix, fused=fused)
        out = dist.sample(SEED, OFFSET)
        (out * _tensor(d['gout'], kind)).sum().backward()
        act = Categorical(x.detach(), unimix, dims=1, fused=fused).sample(SEED, OFFSET).cpu().numpy()
        pred = _host(dist.pred())
        results[name] = (_host(out), _host(x.grad), act, pred)
      clean, got = results['clean'], results['dirty']
      assert (got[2][bad] == -1).all() and (got[2][~bad] >= 0).all()
      for k in (0, 1, 3):
        assert np.isnan(got[k][bad]).all(), k
      same = ~bad
      same[7, 1] = False
      for k in range(4):
        assert np.array_equal(got[k][same], clean[k][same]), k
      assert np.isfinite(got[0][7, 1]).all() and np.isfinite(got[1][7, 1]).all()
      assert got[2][7, 1] != 2 or unimix                           # probability exactly 0: never drawn
      assert _onehot_index(got[0][same]).shape == (same.sum(),)


def test_launch_counts():
  d = _data(3, 18, 37, 1.0)
  torch.cuda.synchronize()
  before = onehot_sample_launches()
  x = _tensor(d['logits']).requires_grad_()
  dist = OneHot(x, 0.01)                                             # fused=None
  out = dist.sample(SEED)
  assert onehot_sample_launches() == before + 1
  out.sum().backward()
  assert onehot_sample_launches() == before + 2                      # one forward, one backward
  dist.pred().sum().backward()
  assert onehot_sample_launches() == before + 4
  dist.sample(uniform=_tensor(d['u']))
  Categorical(x, 0.01, dims=1).sample(SEED, 4)
  assert onehot_sample_launches() == before + 6
  with torch.no_grad():
    OneHot(x, 0.01, fused=False).sample(uniform=_tensor(d['u']))
    assert onehot_sample_launches() == before + 6                    # the caller's uniforms: the composed path launches none
    OneHot(x, 0.01, fused=False).sample(SEED)
    assert onehot_sample_launches() == before + 7                    # the stream alone
    OneHot(x, 0.01, fused=False).pred()
  assert onehot_sample_launches() == before + 7
  wide = torch.zeros(3, 2, 257, device='cuda', requires_grad=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    OneHot(wide, fused=True).sample(SEED)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes'):
    Categorical(wide, dims=1, fused=True).sample(SEED)
  out = OneHot(wide).sample(SEED)
  out.sum().backward()
  assert out.shape == wide.shape and wide.grad.shape == wide.shape
  # no groups: nothing launched
  for fused in (True, None, False):
    empty = torch.zeros(0, 3, 8, device='cuda', requires_grad=True)
    assert OneHot(empty, fused=fused).sample(SEED).shape == (0, 3, 8)
    assert OneHot(empty, fused=fused).pred().shape == (0, 3, 8)
    assert Categorical(empty, dims=1, fused=fused).sample(SEED).shape == (0, 3)
  assert onehot_sample_launches() == before + 7 + 1                  # (the composed 257-class draw: the stream)


def test_refusals():
  x = torch.zeros(3, 4, 8, device='cuda')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    OneHot(x.cpu()).sample(0)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    Categorical(x.cpu()).sample(0)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    philox_uniform(0, 0, 0, 4, 'cpu')
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    OneHot(x.half())
  with pytest.raises(ValueError, match='unimix'):
    OneHot(x, unimix=1.0)
  with pytest.raises(ValueError, match='unimix'):
    Categorical(x, unimix=-0.1)
  strided = torch.zeros(3, 4, 16, device='cuda')[..., ::2]
  for fused in (True, False):
    with pytest.raises(ValueError, match='not contiguous'):
      OneHot(strided, fused=fused).sample(0)
    with pytest.raises(ValueError, match='not contiguous'):
      OneHot(strided, fused=fused).pred()
    with pytest.raises(ValueError, match='not contiguous'):
      Categorical(strided, dims=1, fused=fused).sample(0)
  for bad in (-1, 2 ** 64):
    with pytest.raises(ValueError, match='seed'):
      OneHot(x).sample(bad)
    with pytest.raises(ValueError, match='offset'):
      OneHot(x).sample(0, bad)
  with pytest.raises(TypeError, match='seed'):
    OneHot(x).sample()
  with pytest.raises(TypeError, match='seed'):
    OneHot(x).sample(0.5)
  with pytest.raises(TypeError, match='uniform'):
    OneHot(x).sample(uniform=torch.zeros(3, 4, dtype=torch.float64, device='cuda'))
  with pytest.raises(TypeError, match='uniform'):
    OneHot(x).sample(uniform=torch.zeros(3, 4))
  with pytest.raises(ValueError, match='uniform of shape'):
    OneHot(x).sample(uniform=torch.zeros(3, 5, device='cuda'))
  assert OneHot(x).sample(2 ** 64 - 1, 2 ** 64 - 1).shape == x.shape
