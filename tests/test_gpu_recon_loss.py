"""`embodied_amd.outs.MSE`, `ImageMSE` and `Binary`: the reconstruction terms of
dreamerv3/agent.py:170-182 on the kernels of csrc/recon_loss.hip and as composed
torch ops, against the restatements of tests/recon_loss_cases.py (which the host
test holds against the reference's own run, tests/golden/recon_loss.npz).  Need a
GPU.

The bars.  Loss: |got - want64| <= 1e-5 sum_j |term_j| of the float64 restatement
on the same (for bfloat16: rounded) inputs.  Gradient: each element within
1e-5 s (1 + |want| / s) of the float64 autograd, s = max |want| over the row (a
bfloat16 gradient: plus 2^-8 |want|).  The fused path is held to the restatement
that rounds nothing.  The composed path is held to `cases.restate_rounded`:
float64 around the roundings the reference makes in the compute dtype -- the
sigmoid itself, taken as the device's `torch.sigmoid` gives it (and held to the
float64 sigmoid here), and the upstream gradient of its backward -- so every
case is asserted on both paths, none exempt.  tools/recon_loss_accuracy.py
records the worst ratios in profiles/recon_loss_accuracy.txt."""
import pathlib

import numpy as np
import pytest
import torch

from embodied_amd import _lib
from embodied_amd.outs import MSE, Binary, ImageMSE, recon_loss_launches   # fails without the feature
from tests import recon_loss_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'recon_loss.npz'
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
OPS = pytest.mark.parametrize('op', cases.OPS)
KINDS = pytest.mark.parametrize('kind', cases.KINDS)
CODES = {'mse': _lib.EMB_RECON_MSE, 'symlog': _lib.EMB_RECON_MSE_SYMLOG, 'sigmoid': _lib.EMB_RECON_SIGMOID_MSE,
         'binary': _lib.EMB_RECON_BINARY}


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


def _loss(op, x, target, fused, dims=1):
  """The row losses of `op` through the public classes."""
  if op == 'mse':
    return MSE(x, fused=fused).loss(target, dims)
  if op == 'symlog':
    return MSE(x, 'symlog', fused=fused).loss(target, dims)
  if op == 'sigmoid':
    return ImageMSE(x, fused=fused).loss(target, dims)
  return Binary(x, fused=fused).loss(target, dims)


_WANT = {}


def _device_sigmoid(x, kind):
  """`torch.sigmoid` of x in the compute dtype on the device, widened to float32,
  after holding it to the float64 sigmoid: 2^-21 of it in float32 (four ulps: it
  is not a correctly rounded function), its rounding, 2^-8, on top in bfloat16 -- the composed path's restatement is built
  around this value, so it is checked here on its own."""
  y = _host(torch.sigmoid(_tensor(x, kind)))
  x64 = np.asarray(x, np.float64)
  exact = np.where(x64 >= 0, 1 / (1 + np.exp(-np.abs(x64))), np.exp(-np.abs(x64)) / (1 + np.exp(-np.abs(x64))))
  near = 2.0 ** -21 + (2.0 ** -8 if kind == 'bf16' else 0.0)
  assert (np.abs(y - exact) <= near * exact + 2.0 ** -126).all()           # (below 2^-126 float32 has no 24 bits)
  return y


def _want(c, kind, rounded):
  """The case's data and float64 oracle, computed once and left unchanged."""
  rounded = rounded and c.op == 'sigmoid'                           # the only op that rounds anything
  key = (c, kind, rounded)
  if key not in _WANT:
    d = cases.data(c.op, c.units, c.rows, c.scale, kind)
    want = (cases.restate_rounded(c.op, d['x'], d['target'], d['gout'], kind, y=_device_sigmoid(d['x'], kind))
            if rounded else cases.restate(c.op, d['x'], d['target'], d['gout']))
    want.pop('terms')
    for a in list(d.values()) + list(want.values()):
      a.setflags(write=False)
    _WANT[key] = (d, want)
  return _WANT[key]


def _run(op, d, kind, fused):
  x = _tensor(d['x'], kind).requires_grad_()
  loss = _loss(op, x, _tensor(d['target']), fused)
  assert loss.dtype == torch.float32 and loss.shape == (d['x'].shape[0],)
  (loss * _tensor(d['gout'])).sum().backward()
  assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
  return _host(loss), _host(x.grad)


def _check(op, kind, fused):
  worst = [0.0, 0.0]
  for c in cases.GRID:
    if c.op != op:
      continue
    d, want = _want(c, kind, rounded=not fused)
    loss, grad = _run(op, d, kind, fused)
    print(c, kind, 'fused' if fused else 'composed', end=' ')
    ratio = (cases.loss_ratio(loss, want),
             cases.grad_ratio(grad, want['grad'], cases.row_scale(want['grad']), kind == 'bf16'))
    print(f'loss {ratio[0]:.3g} gradient {ratio[1]:.3g}')
    if cases.loss_held(c.op, c.units):
      assert ratio[0] <= 1.0, (c, kind, ratio)
    if cases.grad_held(c.op, c.units):
      assert ratio[1] <= 1.0, (c, kind, ratio)
    assert not grad[4::5].any()                                      # a zero upstream gradient: exactly zero
    worst = [max(a, b) for a, b in zip(worst, ratio)]
  print(f'{op} {kind} fused={fused}: loss {worst[0]:.3g} of its bar, gradient {worst[1]:.3g} of its bar')


@KINDS
@OPS
def test_fused_path_is_inside_both_bars(op, kind):
  _check(op, kind, True)


@KINDS
@OPS
def test_composed_path_is_inside_both_bars(op, kind):
  _check(op, kind, False)


@PATHS
def test_fixture_is_reproduced(golden, fused):
  for case, c in enumerate(cases.CASES):
    name = cases.tag(case)
    inp = cases.inputs(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(inp)), name
    want = {'loss': golden[f'loss_{name}'], 'abs': cases.restate(c.op, inp['x'], inp['target'])['abs']}
    with torch.no_grad():
      got = _host(_loss(c.op, _tensor(inp['x']), _tensor(inp['target']), fused))
      assert cases.loss_ratio(got, want) <= 1.0, name
      if c.units <= cases.ELEMENTWISE_MAX:
        # dims = 0 runs every element as a row of one unit.  Fused: each is held to its own bar,
        # 1e-5 |term|.  Composed: to the bar of the fixture's row it is a term of, 1e-5 sum_j |term_j| --
        # the fixture is the float64 run of the UNROUNDED sigmoid, and float32's sigmoid is 1 beyond
        # x = 17, so a composed term of 1e-16 is 0: an error of the whole term, and part of that row's error
        terms = golden[f'terms_{name}']
        got = _host(_loss(c.op, _tensor(inp['x']), _tensor(inp['target']), fused, dims=0))
        assert got.shape == terms.shape
        bar = np.abs(terms).reshape(-1) if fused else np.repeat(want['abs'], c.units)
        assert cases.loss_ratio(got.reshape(-1), {'loss': terms.reshape(-1), 'abs': bar}) <= 1.0, name


def _raw(op, x, target, loss=None, gout=None, grad=None):
  """The entry points on device tensors, views included."""
  rows, units = x.shape
  div = cases.div_of(op)
  kinds = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: _lib.U8}
  args = (x.data_ptr(), kinds[x.dtype], target.data_ptr(), kinds[target.dtype], div, rows, units, CODES[op])
  stream = _lib.raw_stream(x.device)
  if loss is not None:
    _lib.api.emb_recon_loss(*args, loss.data_ptr(), stream)
  if grad is not None:
    _lib.api.emb_recon_loss_grad(*args, gout.data_ptr(), grad.data_ptr(), stream)


def _shifted(t, by=1):
  """The same values in a view that starts `by` elements into a larger buffer."""
  buf = torch.empty(t.numel() + by + 3, dtype=t.dtype, device=t.device)
  view = buf[by:by + t.numel()].view(t.shape)
  view.copy_(t)
  assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + by * t.element_size()
  return view


@KINDS
@OPS
def test_odd_offsets_give_the_same_bits(op, kind):
  for units, rows in ((3, 37), (65, 3), (1025, 3), (2049, 3), (12288, 3), (12291, 3)):
    d = cases.data(op, units, rows, 1.0, kind)
    x, t, g = _tensor(d['x'], kind), _tensor(d['target']), _tensor(d['gout'])
    loss, grad = torch.empty(rows, device='cuda'), torch.empty_like(x)
    _raw(op, x, t, loss, g, grad)
    for shift_x, shift_t, shift_g in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)):
      xs = _shifted(x, shift_x) if shift_x else x
      ts = _shifted(t, shift_t) if shift_t else t
      loss2 = torch.empty(rows, device='cuda')
      grad2 = _shifted(torch.zeros_like(x), shift_g) if shift_g else torch.empty_like(x)
      _raw(op, xs, ts, loss2, g, grad2)
      assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), (units, shift_x, shift_t, shift_g)
      assert torch.equal(grad.view(torch.int16 if kind == 'bf16' else torch.int32),
                         grad2.view(torch.int16 if kind == 'bf16' else torch.int32)), (units, shift_x, shift_t, shift_g)
    if op in ('mse', 'symlog'):                                     # a bfloat16 target on an odd half-word
      tb = t.to(torch.bfloat16)
      _raw(op, x, tb, loss, g, grad)
      for shift_x, shift_t in ((0, 1), (1, 1), (0, 3)):
        loss2, grad2 = torch.empty(rows, device='cuda'), torch.empty_like(x)
        _raw(op, _shifted(x, shift_x) if shift_x else x, _shifted(tb, shift_t), loss2, g, grad2)
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), (units, shift_x, shift_t)
        assert torch.equal(grad.view(torch.int16 if kind == 'bf16' else torch.int32),
                           grad2.view(torch.int16 if kind == 'bf16' else torch.int32)), (units, shift_x, shift_t)
      _raw(op, x, t, loss, g, grad)
    # and through the public classes: a view one element in, x and the uint8 target
    xs = _shifted(x).requires_grad_()
    ts = _shifted(t)
    out = _loss(op, xs, ts, True)
    (out * g).sum().backward()
    assert torch.equal(out.detach(), loss) and torch.equal(xs.grad, grad), units


@KINDS
@OPS
def test_nothing_is_written_outside_loss_and_grad(op, kind):
  for units, rows in ((1, 37), (7, 3), (65, 3), (2047, 3), (4099, 3), (12291, 1)):
    d = cases.data(op, units, rows, 1.0, kind)
    x, t, g = _tensor(d['x'], kind), _tensor(d['target']), _tensor(d['gout'])
    loss = torch.full((rows + 16,), 7.0, device='cuda')
    grad = torch.full((rows * units + 32,), 7.0, device='cuda', dtype=x.dtype)
    _raw(op, x, t, loss[8:], g, grad[15:15 + rows * units].view(rows, units))
    assert (loss[:8] == 7).all() and (loss[8 + rows:] == 7).all() and (loss[8:8 + rows] != 7).all()
    assert (grad[:15] == 7).all() and (grad[15 + rows * units:] == 7).all()
    want = torch.empty_like(x)
    _raw(op, x, t, None, g, want)
    assert torch.equal(grad[15:15 + rows * units].view(rows, units), want)


@KINDS
@OPS
def test_a_nan_stays_in_its_row(op, kind):
  for units in (1, 3, 65, 2049, 4099):
    d = cases.data(op, units, 37, 1.0, kind)
    clean = _run(op, d, kind, True)
    dirty = d['x'].copy()
    dirty[2, units // 2] = np.nan
    dirty[5, units - 1] = np.inf
    got = _run(op, dict(d, x=dirty), kind, True)
    assert np.isnan(got[0][[2, 5]]).all()
    assert np.isnan(got[1][2, units // 2]) and np.isnan(got[1][5, units - 1])
    rest = np.ones(37, bool)
    rest[[2, 5]] = False
    assert np.array_equal(got[0][rest], clean[0][rest]) and np.array_equal(got[1][rest], clean[1][rest])
    same = np.ones(units, bool)
    same[units // 2] = False
    assert np.array_equal(got[1][2][same], clean[1][2][same])        # the row's other gradient elements: unchanged


@PATHS
@KINDS
def test_huge_logits_stay_finite(fused, kind):
  for units in (1, 65, 4099):
    for value in (1e4, -1e4):
      x = np.full((3, units), value, np.float32)
      for op in cases.OPS:
        target = np.zeros((3, units), np.uint8 if op in ('sigmoid', 'binary') else np.float32)
        target[1] = 255 if op == 'sigmoid' else 1
        loss, grad = _run(op, {'x': x, 'target': target, 'gout': np.ones(3, np.float32)}, kind, fused)
        assert np.isfinite(loss).all() and np.isfinite(grad).all(), (op, value)
        if op == 'binary':
          wrong = 0 if value > 0 else 1                              # the label the logit contradicts
          assert np.allclose(loss[wrong], units * abs(float(_host(_tensor(x, kind))[0, 0])), rtol=1e-6)
          assert np.abs(loss[1 - wrong]).max() == 0


@OPS
def test_two_runs_give_identical_bits(op):
  for units, rows in ((7, 37), (1024, 37), (27648, 3)):
    for kind in cases.KINDS:
      d = cases.data(op, units, rows, 5.0, kind)
      a, b = _run(op, d, kind, True), _run(op, d, kind, True)
      assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_launch_counts():
  d = cases.data('sigmoid', 255, 37, 1.0)
  x, image = _tensor(d['x']).requires_grad_(), _tensor(d['target'])
  torch.cuda.synchronize()
  before = recon_loss_launches()
  loss = ImageMSE(x).loss(image, dims=1)                             # fused=None
  assert recon_loss_launches() == before + 1
  loss.sum().backward()
  assert recon_loss_launches() == before + 2                         # one forward, one backward
  Binary(x).loss(image > 127, dims=1).sum().backward()
  MSE(x, 'symlog').loss(x.detach() * 2).sum().backward()
  assert recon_loss_launches() == before + 6
  frozen = ImageMSE(x.detach()).loss(image, dims=1)
  assert not frozen.requires_grad
  assert recon_loss_launches() == before + 7                         # x needs no gradient: no backward to launch
  (frozen.sum() + x.sum()).backward()
  assert recon_loss_launches() == before + 7
  ImageMSE(x, fused=False).loss(image, dims=1).sum().backward()
  Binary(x, fused=False).loss(image > 127).sum().backward()
  MSE(x, fused=False).loss(x.detach()).sum().backward()
  assert recon_loss_launches() == before + 7                         # the composed path launches none
  for fused in (True, None, False):
    empty = torch.zeros(0, 8, 8, 3, device='cuda', requires_grad=True)
    out = ImageMSE(empty, fused=fused).loss(torch.zeros(0, 8, 8, 3, dtype=torch.uint8, device='cuda'))
    assert out.shape == (0,)
    out.sum().backward()
    assert Binary(empty, fused=fused).loss(torch.zeros(0, 8, 8, 3, device='cuda')).shape == (0, 8, 8, 3)
    assert MSE(empty, fused=fused).loss(torch.zeros(0, 8, 8, 3, device='cuda'), dims=2).shape == (0, 8)
  assert recon_loss_launches() == before + 7                         # no rows: nothing launched


def test_shapes_and_forcing():
  rng = np.random.default_rng(9)
  x = _tensor(rng.standard_normal((2, 3, 8, 8, 3)).astype(np.float32))
  image = _tensor(rng.integers(0, 256, (2, 3, 8, 8, 3)).astype(np.uint8))
  want = MSE(torch.sigmoid(x), fused=False).loss(image.float() / 255, dims=3)
  for fused in (True, False):
    got = ImageMSE(x, fused=fused).loss(image)
    assert got.shape == (2, 3) and got.dtype == torch.float32
    assert torch.allclose(got, want, rtol=5e-6, atol=0), fused       # sigmoid off by 2^-23 at most: 2.4e-7 / rms(d) of the sum
    assert torch.equal(ImageMSE(x, fused=fused).pred(), torch.sigmoid(x))
  plain = MSE(x, fused=False).loss(image.float() / 255, dims=3)
  for fused in (True, False):
    assert torch.allclose(ImageMSE(x, sigmoid=False, fused=fused).loss(image), plain, rtol=5e-6, atol=0)
  # a bfloat16 target is widened as a float32 one of the same values
  t = _tensor(rng.standard_normal((5, 70)).astype(np.float32), 'bf16')
  y = _tensor(rng.standard_normal((5, 70)).astype(np.float32))
  for squash in (None, 'symlog'):
    assert torch.equal(MSE(y, squash, fused=True).loss(t, 1), MSE(y, squash, fused=True).loss(t.float(), 1))
    assert torch.equal(MSE(y, squash, fused=True).pred(), y)
  # Binary: bool, uint8 and float labels are one loss
  logit = _tensor(3 * rng.standard_normal((4, 9)).astype(np.float32))
  label = _tensor(rng.integers(0, 2, (4, 9)).astype(np.uint8))
  for fused in (True, False):
    head = Binary(logit, fused=fused)
    base = head.loss(label.bool())
    assert base.shape == (4, 9)
    for other in (label, label.float(), label.to(torch.bfloat16), label.double()):
      assert torch.equal(head.loss(other), base)
    assert torch.equal(head.logp(label, dims=1), -head.loss(label, dims=1))
    assert torch.equal(head.pred(), logit > 0)
    u = torch.rand(4, 9, device='cuda')
    assert torch.equal(head.sample(uniform=u), u < torch.sigmoid(logit))
    drawn = head.sample(seed=3, offset=1)
    assert drawn.dtype == torch.bool and torch.equal(drawn, head.sample(seed=3, offset=1))
  # past 2^31 - 1 elements: fused=True says so (an expanded view: no memory behind it)
  wide = torch.zeros(1, device='cuda', dtype=torch.bfloat16).expand(2 ** 16, 2 ** 15)
  frames = torch.zeros(1, device='cuda', dtype=torch.uint8).expand(2 ** 16, 2 ** 15)
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    ImageMSE(wide, fused=True).loss(frames, dims=1)
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    Binary(wide, fused=True).loss(frames)
  with pytest.raises(ValueError, match='target of shape'):
    ImageMSE(x).loss(image[:1])
  with pytest.raises(TypeError, match='uint8'):
    ImageMSE(x).loss(image.float())
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    MSE(x.half())
  with pytest.raises(ValueError, match='dims'):
    MSE(x).loss(x, dims=6)
