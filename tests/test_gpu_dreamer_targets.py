"""`scans.dreamer_targets`: the top of imag_loss (dreamerv3/agent.py:397-419) as
one HIP launch (emb_dreamer_targets, csrc/dreamer_targets.hip) and as the
composition of the library's separate pieces; `scans.lambda_return_cont`, the
lambda-return over float continuation probabilities.  Against the fixture made
by executing the reference's `imag_loss` with its own `lambda_return` and
`Normalize` (tests/golden/dreamer_targets.npz), and the two paths against each
other.  Need a GPU."""
import pathlib

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from embodied_amd import DeviceNormalize
from embodied_amd import normalize as normlib
from embodied_amd import scans
from embodied_amd.scans import dreamer_targets, lambda_return_cont      # every test here fails without the feature
from tests import dreamer_target_cases as cases
# dreamerv3/agent.py:401-405,482-490 in float64, for inputs that are not in the fixture
from tests.target_reference import lambda_cont64 as _reference_lambda_cont

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'dreamer_targets.npz'
# the project's stated float tolerance, as tests/test_gpu_device_normalize.py
RTOL = ATOL = 1e-5
FIELDS = ('ret', 'weight', 'adv', 'adv_normed', 'tar_padded')
GOLDEN_KEYS = dict(ret='ret', adv='adv', adv_normed='advnormed', tar_padded='tarpadded')
ALL3 = (('perc', {}), ('meanstd', {}), ('meanstd', {}))
SHIPPED = (('perc', {}), ('none', {}), ('none', {}))


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def _cuda(array):
  return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def _norms(specs=ALL3):
  return [DeviceNormalize(impl, **{**cases.NORM, **fields}) for impl, fields in specs]


def _state(norm):
  """All five state words as host uint32 (bit patterns); 'none' has none."""
  if norm.impl == 'none':
    return np.zeros(5, np.uint32)
  return norm._state().cpu().numpy().view(np.uint32).copy()


def _pair(norm):
  return [0.0, 1.0] if norm.impl == 'none' else [float(v) for v in norm._stats]


def _worst(got, want):
  return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))) if want.size else 0.0


def _host(result):
  return {k: getattr(result, k).cpu().numpy() for k in FIELDS}


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
@pytest.mark.parametrize('case', range(len(cases.CASES)))
def test_golden_parity(golden, case, fused):
  """Four consecutive train steps with carried state against the reference's."""
  c = cases.CASES[case]
  name = cases.tag(case)
  retnorm, valnorm, advnorm = _norms((c.retnorm, c.valnorm, c.advnorm))
  worst = {}
  for step in range(cases.STEPS):
    inp = cases.inputs(case, step)
    assert np.array_equal(cases.digest(inp), golden[f'in_{name}'][step])
    got = dreamer_targets(_cuda(inp['rew']), _cuda(inp['con']), _cuda(cases.target_pred(case, inp)),
                          retnorm, valnorm, advnorm, contdisc=c.contdisc, fused=fused, **cases.PARAMS)
    host = _host(got)
    stats = np.array(_pair(retnorm) + _pair(advnorm) + _pair(valnorm), np.float64)
    pairs = {**{k: (host[k], golden[f'{g}_{name}'][step]) for k, g in GOLDEN_KEYS.items()},
             'stats': (stats, golden[f'stats_{name}'][step])}
    for key, (have, want) in pairs.items():
      assert have.shape == want.shape, (key, have.shape, want.shape)
      worst[key] = max(worst.get(key, 0.0), _worst(have, want))
    want = golden[f'weight_{name}'][step]
    assert host['weight'].shape == want.shape
    differ = _bits(host['weight']) != _bits(want)
    assert not differ.any(), (name, step, int(differ.sum()), np.argwhere(differ)[:4].tolist())
  print(f'{name} {"fused" if fused else "composed"}: worst |got - want| / (atol + rtol |want|) = '
        + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()) + '; weight bit for bit')
  assert max(worst.values()) <= 1.0, worst


def _golden_inputs(case, step=0):
  inp = cases.inputs(case, step)
  return inp['rew'], inp['con'], cases.target_pred(case, inp)


# (3, 5), (5, 257) and (1, 1030) run without a valnorm: boot is the prediction
# itself.  (7, 2) has a 'meanstd' valnorm: at step 0 its statistics are fresh,
# (voffset, vscale) = (0, limit), so boot = pred * limit + 0.
@pytest.mark.parametrize('case', [2, 3, 4, 7])
def test_lambda_return_cont_against_the_fixture(golden, case):
  c = cases.CASES[case]
  assert c.shape == {2: (3, 5), 3: (7, 2), 4: (5, 257), 7: (1, 1030)}[case]
  fresh_valnorm = case not in cases.NONE_VALNORM_CASES
  disc = 1 if c.contdisc else 1 - 1 / cases.PARAMS['horizon']
  for step in range(1 if fresh_valnorm else cases.STEPS):
    inp = cases.inputs(case, step)
    boot = cases.target_pred(case, inp)
    if fresh_valnorm:
      boot = boot * np.float32(cases.NORM['limit']) + np.float32(0)
    ret = lambda_return_cont(_cuda(inp['rew']), _cuda(inp['con']), _cuda(boot), disc, cases.PARAMS['lam'])
    np.testing.assert_allclose(ret.cpu().numpy(), golden[f'ret_{cases.tag(case)}'][step], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('shape', [(3, 5), (7, 2), (5, 257), (1, 1030)])
def test_lambda_return_cont_every_row_length(shape):
  """Rows of <= 16, <= 256 and > 256 steps take three different kernels."""
  rew, con, pred = (x.cpu().numpy() for x in _fresh(*shape, 5))
  for disc in (1.0, float(np.float32(1 - 1 / 333))):
    ret = lambda_return_cont(_cuda(rew), _cuda(con), _cuda(pred), disc, 0.95)
    assert ret.shape == (shape[0], shape[1] - 1)
    want = _reference_lambda_cont(rew, con, pred, disc, float(np.float32(0.95)))
    np.testing.assert_allclose(ret.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    out = torch.empty(shape[0], shape[1] - 1, device='cuda')
    assert lambda_return_cont(_cuda(rew), _cuda(con), _cuda(pred), disc, 0.95, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ret.cpu().numpy()))
  with pytest.raises(ValueError, match='out='):
    lambda_return_cont(_cuda(rew), _cuda(con), _cuda(pred), 1.0, 0.95, out=torch.empty(shape, device='cuda'))


def test_lambda_return_with_flags_is_not_this_scan(golden):
  """Why the new scan exists: `lambda_return` reads `term` as flags, so
  term = 1 - con makes every con < 1 terminal and the returns differ."""
  case = 0
  rew, con, pred = (_cuda(x) for x in _golden_inputs(case))
  want = golden[f'ret_{cases.tag(case)}'][0]
  flags = scans.lambda_return(torch.zeros_like(con), 1 - con, rew, pred, pred, 1.0, cases.PARAMS['lam'])
  assert not np.allclose(flags.cpu().numpy(), want, rtol=1e-2, atol=1e-2)
  cont = lambda_return_cont(rew, con, pred, 1.0, cases.PARAMS['lam'])
  np.testing.assert_allclose(cont.cpu().numpy(), want, rtol=RTOL, atol=ATOL)


def _fresh(N, T, seed, misalign=False):
  """Random inputs that are not in the fixture; with `misalign` every tensor
  starts one element past a 16-byte boundary."""
  gen = np.random.default_rng([seed, N, T])
  rew = gen.standard_normal((N, T)).astype(np.float32)
  con = (0.9 + 0.1 * gen.random((N, T))).astype(np.float32)
  pick = gen.random((N, T))
  con[pick < 0.03] = 0.0
  con[pick > 0.97] = 1.0
  pred = gen.standard_normal((N, T)).astype(np.float32)
  out = []
  for array in (rew, con, pred):
    t = _cuda(array)
    if misalign:
      padded = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
      padded[1:].copy_(t.reshape(-1))
      t = padded[1:].view(N, T)
      assert t.is_contiguous() and t.data_ptr() % 16 == 4
    out.append(t)
  return out


def _shapes(N, T):
  return ((N, T - 1), (N, T), (N, T - 1), (N, T - 1), (N, T))


def _outs(N, T, misalign=False):
  if not misalign:
    return None
  outs = []
  for rows, cols in _shapes(N, T):
    padded = torch.empty(rows * cols + 1, dtype=torch.float32, device='cuda')
    outs.append(padded[1:].view(rows, cols))
    assert outs[-1].data_ptr() % 16 == 4
  return tuple(outs)


# the shipped shape, exactly kNormLdsMax values, one value, and the PPO file's shapes
@pytest.mark.parametrize('misalign', [False, True], ids=['aligned', 'off16'])
@pytest.mark.parametrize('shape', [(1024, 16), (1024, 17), (1, 2), (3, 5), (7, 2), (64, 16), (5, 257), (1, 1030)])
def test_fused_against_composed(shape, misalign):
  N, T = shape
  specs = ALL3 if (N + T) % 2 else SHIPPED          # both sets of normalisers over the shapes
  contdisc = shape != (64, 16) and shape != (1, 1030)
  runs = {}
  for path in ('fused', 'composed', 'again'):
    norms = _norms(specs)
    results = []
    for step in range(3):
      inp = _fresh(N, T, step, misalign)
      results.append(_host(dreamer_targets(*inp, *norms, contdisc=contdisc, out=_outs(N, T, misalign),
                                           fused=path != 'composed')))
    runs[path] = (results, [_state(norm) for norm in norms])
  # One value (1, 2): rscale = limit, so adv and everything after it is rounding
  # noise divided by 1e-8: ret, weight and retnorm's statistics only.
  n_values, worst = N * (T - 1), 0.0
  for a, b in zip(runs['fused'][0], runs['composed'][0]):
    for key in FIELDS if n_values > 1 else ('ret', 'weight'):
      worst = max(worst, _worst(a[key], b[key]))
      np.testing.assert_allclose(a[key], b[key], rtol=RTOL, atol=ATOL, err_msg=key)
    assert np.array_equal(_bits(a['weight']), _bits(b['weight']))
  for norm, fused_state, composed_state in zip(_norms(specs), runs['fused'][1], runs['composed'][1]):
    if n_values > 1 or norm.impl == 'perc':
      np.testing.assert_allclose(fused_state.view(np.float32), composed_state.view(np.float32), rtol=RTOL, atol=ATOL)
  print(f'{shape} fused against composed: worst ratio {worst:.4f}')
  # two fused runs from equal state: the same bits
  for a, b in zip(runs['fused'][0], runs['again'][0]):
    for key in FIELDS:
      assert np.array_equal(_bits(a[key]), _bits(b[key])), key
  for a, b in zip(runs['fused'][1], runs['again'][1]):
    assert np.array_equal(a, b)


def test_beyond_one_workgroup_composes():
  N, T = 1024, 18                              # 17 408 returns: more keys than one workgroup holds
  inp = _fresh(N, T, 60)
  with pytest.raises(ValueError, match='fused=True.*17408 returns'):
    dreamer_targets(*inp, *_norms(SHIPPED), fused=True)
  ours = scans.dreamer_targets_launches()
  got = dreamer_targets(*inp, *_norms(SHIPPED))
  assert scans.dreamer_targets_launches() == ours
  assert got.ret.shape == (N, T - 1) and bool(torch.isfinite(got.adv_normed).all())


@pytest.mark.parametrize('shape', [(64, 16), (5, 257)])
def test_state_coherence(shape):
  """The kernel and emb_normalize form (offset, scale) with one device function:
  stats() after fused steps returns the bits the fused launch left."""
  norms = _norms(ALL3)
  for step in range(3):
    dreamer_targets(*_fresh(*shape, 10 + step), *norms, fused=True)
  for norm in norms:
    left = _state(norm)
    offset, scale = norm.stats()
    after = _state(norm)
    assert np.array_equal(left, after), (norm.impl, left, after)
    assert offset.cpu().numpy().view(np.uint32) == left[3] and scale.cpu().numpy().view(np.uint32) == left[4]


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_update_false(fused):
  norms = _norms(ALL3)
  for step in range(2):
    dreamer_targets(*_fresh(64, 16, 20 + step), *norms, fused=fused)
  before = [_state(norm) for norm in norms]
  (roffset, rscale), (voffset, vscale), (aoffset, ascale) = ([v.clone() for v in norm.stats()] for norm in norms)
  rew, con, pred = _fresh(64, 16, 29)
  got = dreamer_targets(rew, con, pred, *norms, update=False, fused=fused)
  for b, norm in zip(before, norms):
    a = _state(norm)
    assert np.array_equal(b[:3], a[:3]), (b, a)
    assert np.array_equal(b, a)                     # words 3-4 rewritten with the same values
  tarval = pred * vscale + voffset
  torch.testing.assert_close(got.adv, (got.ret - tarval[:, :-1]) / rscale, rtol=1e-6, atol=0)
  torch.testing.assert_close(got.adv_normed, (got.adv - aoffset) / ascale, rtol=1e-6, atol=0)
  torch.testing.assert_close(got.tar_padded[:, :-1], (got.ret - voffset) / vscale, rtol=1e-6, atol=0)
  want = lambda_return_cont(rew, con, tarval, 1.0, 0.95)
  torch.testing.assert_close(got.ret, want, rtol=RTOL, atol=ATOL)


class _Ops(TorchDispatchMode):
  """Every operator torch dispatches while the mode is on."""

  def __init__(self):
    super().__init__()
    self.seen = []

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    self.seen.append(str(func))
    return func(*args, **(kwargs or {}))


@pytest.mark.parametrize('specs', [SHIPPED, ALL3], ids=['shipped', 'all3'])
def test_one_launch(specs):
  N, T = 64, 16
  inp = _fresh(N, T, 40)
  norms = _norms(specs)
  out = tuple(torch.empty(shape, device='cuda') for shape in _shapes(N, T))
  dreamer_targets(*inp, *norms, out=out, fused=True)
  torch.cuda.synchronize()
  ours, theirs = scans.dreamer_targets_launches(), normlib.launches()
  with _Ops() as ops:
    got = dreamer_targets(*inp, *norms, out=out, fused=True)
  assert ops.seen == [], ops.seen
  assert scans.dreamer_targets_launches() - ours == 1
  assert normlib.launches() == theirs
  assert all(a is b for a, b in zip(got, out))
  # the composed path: one normalising launch per normaliser that is not 'none'
  ours, theirs = scans.dreamer_targets_launches(), normlib.launches()
  dreamer_targets(*inp, *norms, out=out, fused=False)
  assert normlib.launches() - theirs == sum(norm.impl != 'none' for norm in norms)
  assert scans.dreamer_targets_launches() == ours
  # fused=None: the kernel up to the crossover, the composition for other impls
  ours = scans.dreamer_targets_launches()
  dreamer_targets(*inp, *norms, out=out)
  assert scans.dreamer_targets_launches() - ours == int(N * (T - 1) <= scans.DREAMER_TARGETS_FUSED_MAX)
  ours = scans.dreamer_targets_launches()
  dreamer_targets(*inp, DeviceNormalize('meanstd'), *norms[1:])
  assert scans.dreamer_targets_launches() == ours


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_pad_and_degenerate_shapes(fused):
  got = dreamer_targets(*_fresh(5, 257, 70), *_norms(ALL3), fused=fused)
  assert np.array_equal(_bits(got.tar_padded[:, -1].cpu().numpy()), np.zeros(5, np.uint32))      # +0.0 bitwise
  assert bool((got.tar_padded[:, :-1] != 0).any())
  ours, theirs = scans.dreamer_targets_launches(), normlib.launches()
  empty = dreamer_targets(*(torch.empty(0, 4, device='cuda') for _ in range(3)), *_norms(SHIPPED), fused=fused)
  assert [tuple(t.shape) for t in empty] == list(_shapes(0, 4))
  rew, con, pred = _fresh(3, 1, 71)
  single = dreamer_targets(rew, con, pred, *_norms(SHIPPED), fused=fused)
  assert [tuple(t.shape) for t in single] == list(_shapes(3, 1))
  assert np.array_equal(_bits(single.weight.cpu().numpy()), _bits(con.cpu().numpy()))
  assert not single.tar_padded.any()
  assert (scans.dreamer_targets_launches(), normlib.launches()) == (ours, theirs)


def test_out_validation_and_reuse():
  N, T = 3, 5
  inp = _fresh(N, T, 50)
  good = [torch.empty(shape, device='cuda') for shape in _shapes(N, T)]
  bad = {
      'shape': torch.empty((N, T - 1), device='cuda'),              # in tar_padded's place
      'dtype': torch.empty((N, T), dtype=torch.float64, device='cuda'),
      'device': torch.empty((N, T)),
      'strides': torch.empty((T, N), device='cuda').t(),
  }
  for fused in (True, False):
    for why, tensor in bad.items():
      with pytest.raises(ValueError, match='out='):
        dreamer_targets(*inp, *_norms(), out=(*good[:4], tensor), fused=fused)
    with pytest.raises(ValueError, match='out='):
      dreamer_targets(*inp, *_norms(), out=good[:4], fused=fused)
    norms = _norms()
    first = _host(dreamer_targets(*inp, *norms, out=good, fused=fused))
    second = dreamer_targets(*_fresh(N, T, 51), *norms, out=good, fused=fused)
    assert all(a is b for a, b in zip(second, good))
    assert not np.array_equal(first['ret'], good[0].cpu().numpy())
    fresh = dreamer_targets(*inp, *_norms(), fused=fused)                # one allocation, same values
    assert all(t.data_ptr() % 16 == 0 for t in fresh)
    for key, values in _host(fresh).items():
      assert np.array_equal(first[key], values), key
