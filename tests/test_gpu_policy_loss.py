"""`embodied_amd.outs.policy_loss` / `Categorical`: the actor's loss of imag_loss
(dreamerv3/agent.py:411-415) on the kernels of csrc/policy_loss.hip and as
composed torch ops, against the float64 run of the reference's own `imag_loss`
and output classes (tests/golden/policy_loss.npz) and, for other shapes,
bfloat16-rounded inputs and the gradients, against
`tests.policy_loss_cases.reference64` (which the host test holds against that
fixture).  Need a GPU.

Bars: loss, logpi and ent within 1e-5 + 1e-5 |want| of float64; a gradient
element within 1e-5 s (1 + |want| / s), s = |gout weight| (|adv| + actent) the
row's scale (a bfloat16 gradient: plus 2^-8 |want|, its own rounding).  The
float32 definition sits inside both at every logit scale, with and without
unimix (tests/test_policy_loss_host.py prints its ratios), so no case is exempt.
tools/policy_loss_accuracy.py records the kernels' worst ratios in
profiles/policy_loss_accuracy.txt."""
import pathlib

import numpy as np
import pytest
import torch

from embodied_amd.outs import Categorical, policy_loss, policy_loss_launches      # every test here fails without the feature
from tests import policy_loss_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'policy_loss.npz'
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
# every shape on both paths, 257 classes on the composed path alone
SHAPE_PATHS = [pytest.param(shape, fused, id=f'{shape[0]}x{shape[1]}-{"fused" if fused else "composed"}')
               for shape in cases.SHAPES for fused in (True, False) if not (fused and shape[1] > 256)]
OUTPUTS = ('loss', 'logpi', 'ent')
# output rows 1, 3, 4, 5, 37 and 75 with drop_last (2, 6, 6, 74, 80 rows of logits), as many without
GEOMETRIES = ((1, 2), (3, 2), (2, 3), (37, 2), (5, 16))


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


def _data(groups, classes, n, t, scale, kind='f32', drop=1):
  """Seeded inputs (bfloat16-rounded logits for kind 'bf16'), made once and left
  unchanged: every fourth sequence ends early (weight 0 from some step on)."""
  key = (groups, classes, n, t, scale, kind, drop)
  if key not in _DATA:
    rng = np.random.default_rng([groups, classes, n, t, int(scale * 10), drop])
    logits = cases.logits_of(n, t, groups, classes, scale, rng)
    if kind == 'bf16':
      logits = cases.bf16_round(logits)
    act = cases.actions_of(n, t, groups, classes, rng)
    adv = (2 * rng.standard_normal((n, t - drop))).astype(np.float32)
    weight = np.cumprod(np.where((np.arange(n)[:, None] % 4 == 1) & (np.arange(t) >= t // 2), 0, 0.997), 1)
    gout = rng.standard_normal((n, t - drop)).astype(np.float32)
    d = dict(logits=logits, act=act, adv=adv, weight=weight.astype(np.float32), gout=gout, drop=drop,
             dims=1 if groups else 0, ref={})
    for a in d.values():
      if isinstance(a, np.ndarray):
        a.setflags(write=False)
    _DATA[key] = d
  return _DATA[key]


def _ref(d, unimix, actent=cases.ACTENT):
  if (unimix, actent) not in d['ref']:
    d['ref'][unimix, actent] = cases.reference64(
        d['logits'], d['act'], d['adv'], d['weight'], actent, unimix, d['dims'], d['drop'], d['gout'])
  return d['ref'][unimix, actent]


def _run(d, unimix, fused, kind='f32', actent=cases.ACTENT, cut_weight=False, lead=None, logits=None):
  """policy_loss over `d` -> (outputs as numpy (n, t - drop), grad as numpy in the logits' shape)."""
  n, t = d['logits'].shape[:2]
  kept = t - d['drop']
  x = _tensor(d['logits'] if logits is None else logits, kind)
  act, adv, weight = _tensor(d['act']), _tensor(d['adv']), _tensor(d['weight'][:, :kept] if cut_weight else d['weight'])
  gout = _tensor(d['gout'])
  if lead == 'flat':            # (n, t) -> (n * t,), where no step is dropped
    x, act, adv, weight, gout = (v.reshape(-1, *v.shape[2:]) for v in (x, act, adv, weight, gout))
  elif lead is not None:        # (n,) -> lead in front of the time axis (drop_last), or of everything (not)
    x, act, adv, weight, gout = (v.view(*lead, *v.shape[1:]) for v in (x, act, adv, weight, gout))
  x.requires_grad_()
  out = policy_loss(x, act, adv, weight, actent=actent, unimix=unimix, dims=d['dims'], drop_last=bool(d['drop']),
                    fused=fused)
  assert sorted(out) == sorted(OUTPUTS)
  for key in OUTPUTS:
    assert out[key].dtype == torch.float32 and out[key].shape == gout.shape, key
  assert out['loss'].requires_grad and not out['logpi'].requires_grad and not out['ent'].requires_grad
  (out['loss'] * gout).sum().backward()
  assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
  return {k: _host(v).reshape(n, kept) for k, v in out.items()}, _host(x.grad).reshape(d['logits'].shape)


def _ratios(d, out, grad, ref, kind, actent=cases.ACTENT):
  kept = d['logits'].shape[1] - d['drop']
  forward = max(cases.forward_ratio(out[key], ref[key]) for key in OUTPUTS)
  assert not grad[:, kept:].any()                                   # a dropped step: zeros
  s = cases.row_scale(d['gout'], d['weight'][:, :kept], d['adv'], actent)
  return forward, cases.grad_ratio(grad[:, :kept], ref['grad'][:, :kept], s, kind == 'bf16')


@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_fixture_parity(golden, shape, fused):
  """Every case of the fixture at this shape (five logit scales, unimix 0 and
  0.01), both layouts of weight, against the reference's own float64 run of
  imag_loss; the out-of-range actions of the first row are in it."""
  worst = 0.0
  for case, c in enumerate(cases.CASES):
    if (c.groups, c.classes) != shape:
      continue
    name = cases.tag(case)
    inp = cases.inputs(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(inp))
    want = dict(zip(cases.FIELDS, golden[f'out64_{name}']))
    logits, act = _tensor(inp['logits']), _tensor(inp['act'])
    adv, weight = _tensor(golden[f'adv_{name}']), _tensor(golden[f'weight_{name}'])
    for w in (weight, weight[:, :-1]):
      out = policy_loss(logits, act, adv, w, actent=cases.ACTENT, unimix=c.unimix, dims=1 if c.groups else 0, fused=fused)
      ratio = max(cases.forward_ratio(_host(out[key]), want[key]) for key in OUTPUTS)
      assert ratio <= 1.0, (name, ratio)
      worst = max(worst, ratio)
  print(f'{shape} fused={fused}: {worst:.3g} of the forward bar')


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_parity_with_gradients(shape, fused, kind):
  """(N, T) of (1, 2), (3, 2), (2, 3), (37, 2) and (5, 16) with drop_last and
  without (1 .. 80 output rows: fewer than a workgroup's waves, no multiple of
  them, many workgroups), every logit scale, unimix 0 and 0.01, both dtypes,
  both layouts of weight, leading shapes (N, T), flattened and with one more axis in front:
  the three outputs and the gradient against float64."""
  groups, classes = shape
  worst = [0.0, 0.0]
  for i, (n, t) in enumerate(GEOMETRIES):
    for drop in (1, 0):
      for j, unimix in enumerate(cases.UNIMIX):
        scale = cases.SCALES[(i + j + drop) % len(cases.SCALES)]
        d = _data(groups, classes, n, t, scale, kind, drop)
        lead = (1, n) if (i + j) % 2 else None if drop else 'flat'
        out, grad = _run(d, unimix, fused, kind, cut_weight=bool((i + drop) % 2), lead=lead)
        ratios = _ratios(d, out, grad, _ref(d, unimix), kind)
        assert max(ratios) <= 1.0, (n, t, drop, unimix, scale, ratios)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
  print(f'{shape} {kind} fused={fused}: forward {worst[0]:.3g}, gradient {worst[1]:.3g} of their bars')


@PATHS
@pytest.mark.parametrize('unimix', cases.UNIMIX)
def test_every_scale_at_one_shape(unimix, fused):
  """(3, 18) and (33, 2) at all five logit scales, a large entropy coefficient too."""
  for groups, classes in ((3, 18), (33, 2)):
    for scale in cases.SCALES:
      d = _data(groups, classes, 5, 16, scale)
      for actent in (cases.ACTENT, 0.5):
        out, grad = _run(d, unimix, fused, actent=actent)
        ratios = _ratios(d, out, grad, _ref(d, unimix, actent), 'f32', actent)
        assert max(ratios) <= 1.0, (groups, classes, scale, actent, ratios)


@PATHS
def test_actions_at_the_edges_and_outside(fused):
  """Class 0, the last class, -1 and `classes`: the two outside add exactly 0 to
  logpi and leave the entropy's gradient alone; int64 actions, one beyond int32
  too, are the same as int32."""
  for groups, classes in ((0, 5), (3, 18), (1, 256)):
    d = _data(groups, classes, 3, 2, 1.0, drop=0)
    edge = d['act'].reshape(-1)[:4]
    assert list(edge) == [0, classes - 1, -1, classes]
    for unimix in cases.UNIMIX:
      ref = _ref(d, unimix)
      out, grad = _run(d, unimix, fused)
      assert max(_ratios(d, out, grad, ref, 'f32')) <= 1.0
      assert np.isfinite(out['logpi']).all() and np.isfinite(grad).all()
      if not groups:
        assert out['logpi'][0, 0] != 0 and out['logpi'][1, 0] == 0 and out['logpi'][1, 1] == 0
        # no action term: the gradient of those two rows is the entropy's alone
        none = cases.reference64(d['logits'], None, d['adv'], d['weight'], cases.ACTENT, unimix, 0, 0, d['gout'])
        s = cases.row_scale(d['gout'], d['weight'], d['adv'], cases.ACTENT)
        assert cases.grad_ratio(grad[1], none['grad'][1], s[1]) <= 1.0
    x = _tensor(d['logits'])
    act = _tensor(d['act']).to(torch.int64)
    far = act.clone()
    far.view(-1)[2] = 2 ** 32                       # wraps to class 0 if narrowed blindly
    kw = dict(actent=cases.ACTENT, unimix=0.01, dims=d['dims'], drop_last=False, fused=fused)
    base = policy_loss(x, _tensor(d['act']), _tensor(d['adv']), _tensor(d['weight']), **kw)
    for other in (act, far):
      again = policy_loss(x, other, _tensor(d['adv']), _tensor(d['weight']), **kw)
      assert all(torch.equal(base[key], again[key]) for key in OUTPUTS)


@PATHS
def test_zero_weight_rows(fused):
  """A continuation flag of 0 zeroes the weight from there on: loss and gradient
  of those rows are exactly zero, logpi and ent are what they are."""
  d = _data(3, 18, 5, 16, 1.0)
  out, grad = _run(d, 0.01, fused)
  dead = d['weight'][:, :-1] == 0
  assert dead.any() and not dead.all()
  assert not out['loss'][dead].any() and out['loss'][~dead].all()
  assert not grad[:, :-1][dead].any() and np.abs(grad[:, :-1][~dead]).max() > 0
  assert out['ent'][dead].all() and out['logpi'][dead].all()


@PATHS
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_categorical_logp_and_entropy(fused, kind):
  """`Categorical.logp` and `.entropy` alone, each with its gradient, dims 0 and 1."""
  for groups, classes, unimix in ((0, 5, 0.0), (3, 18, 0.01), (33, 2, 0.0), (3, 96, 0.01)):
    d = _data(groups, classes, 37, 2, 1.0, kind, drop=0)
    ones = np.ones_like(d['gout'])
    x = _tensor(d['logits'], kind).requires_grad_()
    dist = Categorical(x, unimix=unimix, dims=d['dims'], fused=fused)
    assert dist.fused is fused and dist.minent == 0 and dist.maxent == pytest.approx(np.log(classes) * max(groups, 1))
    # logp = -loss with adv = weight = 1, actent = 0; entropy = loss with no action and actent = -1
    want = cases.reference64(d['logits'], d['act'], None, None, 0.0, unimix, d['dims'], 0, -d['gout'])
    logp = dist.logp(_tensor(d['act']))
    assert logp.shape == (37, 2) and logp.dtype == torch.float32
    (logp * _tensor(d['gout'])).sum().backward()
    assert cases.forward_ratio(_host(logp), want['logpi']) <= 1.0
    s = cases.row_scale(d['gout'], ones, ones, 0.0)
    assert cases.grad_ratio(_host(x.grad), want['grad'], s, kind == 'bf16') <= 1.0
    x.grad = None
    want = cases.reference64(d['logits'], None, None, None, -1.0, unimix, d['dims'], 0, d['gout'])
    entropy = dist.entropy()
    assert entropy.shape == (37, 2) and entropy.requires_grad
    (entropy * _tensor(d['gout'])).sum().backward()
    assert cases.forward_ratio(_host(entropy), want['ent']) <= 1.0
    assert np.array_equal(want['ent'], want['loss'])
    assert cases.grad_ratio(_host(x.grad), want['grad'], s, kind == 'bf16') <= 1.0
    pred = dist.pred()
    assert pred.shape == x.shape[:-1] and pred.dtype == torch.int64
    if not unimix:              # (the mix and the log can round two neighbours onto each other)
      assert torch.equal(pred, x.detach().float().argmax(-1))


@PATHS
def test_two_action_keys_add_up(fused):
  """agent.py:411-414 sums logpi and the entropies over the action keys first;
  the loss is linear in both, so two calls add up to it within the forward bar."""
  a, b = _data(3, 18, 5, 16, 1.0), _data(0, 5, 5, 16, 5.0)
  ra = cases.reference64(a['logits'], a['act'], None, None, 0.0, 0.01, 1, 1)
  rb = cases.reference64(b['logits'], b['act'], None, None, 0.0, 0.01, 0, 1)
  want = a['weight'][:, :-1] * -((ra['logpi'] + rb['logpi']) * a['adv'] + cases.ACTENT * (ra['ent'] + rb['ent']))
  total = 0
  for d in (a, b):
    total = total + policy_loss(_tensor(d['logits']), _tensor(d['act']), _tensor(a['adv']), _tensor(a['weight']),
                                actent=cases.ACTENT, unimix=0.01, dims=d['dims'], fused=fused)['loss']
  assert cases.forward_ratio(_host(total), want) <= 1.0


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('groups,classes', [(3, 5), (3, 18)])
def test_padding_lanes_and_dropped_steps_do_not_see_their_neighbours(groups, classes, kind):
  """The logits inside one allocation whose every other element is NaN, at an
  odd offset, and NaN in every dropped step: a lane past `classes`, a segment
  past `groups` or a read of a dropped step would show."""
  d = _data(groups, classes, 5, 16, 1.0, kind)
  n = d['logits'].size
  dtype = torch.float32 if kind == 'f32' else torch.bfloat16
  room = torch.full((n + 64,), float('nan'), dtype=dtype, device='cuda')
  x = room[7:7 + n].view(d['logits'].shape)
  x.copy_(_tensor(d['logits'], kind))
  x[:, -1] = float('nan')
  assert x.is_contiguous() and x.storage_offset() == 7
  x.requires_grad_()
  out = policy_loss(x, _tensor(d['act']), _tensor(d['adv']), _tensor(d['weight']), actent=cases.ACTENT, unimix=0.01,
                    dims=1, fused=True)
  (out['loss'] * _tensor(d['gout'])).sum().backward()
  ratios = _ratios(d, {k: _host(v) for k, v in out.items()}, _host(x.grad), _ref(d, 0.01), kind)
  assert max(ratios) <= 1.0, ratios


@PATHS
def test_strided_logits(fused):
  d = _data(3, 18, 5, 16, 1.0)
  wide = torch.zeros(5, 16, 3, 24, device='cuda')
  wide[..., 3:21] = _tensor(d['logits'])
  x = wide[..., 3:21].detach().requires_grad_()               # classes 24 floats apart, offset 3
  assert not x.is_contiguous()
  out = policy_loss(x, _tensor(d['act']), _tensor(d['adv']), _tensor(d['weight']), actent=cases.ACTENT, unimix=0.01,
                    dims=1, fused=fused)
  (out['loss'] * _tensor(d['gout'])).sum().backward()
  assert max(_ratios(d, {k: _host(v) for k, v in out.items()}, _host(x.grad), _ref(d, 0.01), 'f32')) <= 1.0


def _poisoned(d, value, step, row=2, group=1):
  logits = d['logits'].copy()
  if value == 'group':
    logits[row, step, group, :] = -np.inf
  else:
    logits[row, step, group, 3] = value
  return logits


VALUES = pytest.mark.parametrize('value', [np.nan, np.inf, 'group'], ids=['nan', 'pinf', 'group_of_ninf'])


@PATHS
@VALUES
@pytest.mark.parametrize('unimix', cases.UNIMIX)
def test_a_poisoned_logit_makes_its_row_nan_and_no_other(value, unimix, fused):
  """A NaN or +inf logit, or a group of -inf, in a kept step: that output row's
  loss, logpi and ent are NaN, its gradient NaN in the poisoned group (on the
  kernels: over the whole row), and no other row changes by a bit."""
  d = _data(3, 5, 5, 3, 1.0)
  clean = _run(d, unimix, fused)
  dirty = _run(d, unimix, fused, logits=_poisoned(d, value, step=1))
  bad = np.zeros((5, 2), bool)
  bad[2, 1] = True
  for key in OUTPUTS:
    assert np.isnan(dirty[0][key][bad]).all() and np.array_equal(dirty[0][key][~bad], clean[0][key][~bad]), key
  assert np.isnan(dirty[1][2, 1, 1]).all()
  if fused:
    assert np.isnan(dirty[1][2, 1]).all()
  others = np.ones((5, 3), bool)
  others[2, 1] = False
  assert np.array_equal(dirty[1][others], clean[1][others]) and np.isfinite(dirty[1][others]).all()


@PATHS
@VALUES
def test_a_poisoned_dropped_step_touches_nothing(value, fused):
  """The same values in the step that drop_last drops: every output has the bits
  of the clean run and that step's gradient is zeros."""
  d = _data(3, 5, 5, 3, 1.0)
  clean = _run(d, 0.01, fused)
  dirty = _run(d, 0.01, fused, logits=_poisoned(d, value, step=2))
  for key in OUTPUTS:
    assert np.array_equal(dirty[0][key], clean[0][key]) and np.isfinite(dirty[0][key]).all(), key
  assert np.array_equal(dirty[1], clean[1]) and np.isfinite(dirty[1]).all() and not dirty[1][:, 2].any()


@PATHS
def test_a_single_ninf_logit(fused):
  """With unimix it is a class of probability unimix / classes: finite, equal to
  the definition.  Without, 0 * -inf in the definition: the row's outputs are NaN
  on both paths and no other row changes."""
  d = _data(3, 5, 5, 3, 1.0)
  logits = _poisoned(d, -np.inf, step=1)
  out, grad = _run(d, 0.01, fused, logits=logits)
  ref = cases.reference64(logits, d['act'], d['adv'], d['weight'], cases.ACTENT, 0.01, 1, 1, d['gout'])
  assert np.isfinite(ref['loss']).all() and np.isfinite(grad).all()
  assert max(_ratios(d, out, grad, ref, 'f32')) <= 1.0
  clean = _run(d, 0.0, fused)
  out, grad = _run(d, 0.0, fused, logits=logits)
  bad = np.zeros((5, 2), bool)
  bad[2, 1] = True
  for key in OUTPUTS:
    assert np.isnan(out[key][bad]).all() and np.array_equal(out[key][~bad], clean[0][key][~bad]), key


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_same_bits_run_to_run(kind):
  d = _data(3, 18, 37, 2, 5.0, kind)
  first = _run(d, 0.01, True, kind)
  again = _run(d, 0.01, True, kind)
  for key in OUTPUTS:
    assert np.array_equal(first[0][key], again[0][key]), key
  assert np.array_equal(first[1], again[1])


def test_launch_counts():
  d = _data(3, 18, 5, 16, 1.0)
  torch.cuda.synchronize()
  before = policy_loss_launches()
  x = _tensor(d['logits']).requires_grad_()
  args = (_tensor(d['act']), _tensor(d['adv']), _tensor(d['weight']))
  out = policy_loss(x, *args, dims=1)                          # fused=None takes the kernels where they fit
  assert policy_loss_launches() == before + 1
  out['loss'].sum().backward()
  assert policy_loss_launches() == before + 2                  # one forward, one backward
  x.grad = None
  policy_loss(x, *args, dims=1, fused=False)['loss'].sum().backward()
  assert policy_loss_launches() == before + 2                  # the composed path launches none of the kernels
  wide = torch.zeros(3, 2, 257, device='cuda', requires_grad=True)
  small = (torch.zeros(3, 2, dtype=torch.int32, device='cuda'), torch.ones(3, 1, device='cuda'), torch.ones(3, 2, device='cuda'))
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    policy_loss(wide, *small, fused=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes'):
    Categorical(wide, fused=True)
  policy_loss(wide, *small)['loss'].sum().backward()
  assert Categorical(wide).fused is False
  # no output rows: T = 1 with drop_last, or N = 0 -- nothing launched, the gradient is zeros
  for fused in (True, None, False):
    single = torch.randn(4, 1, 8, device='cuda', requires_grad=True)
    out = policy_loss(single, torch.zeros(4, 1, dtype=torch.int32, device='cuda'), torch.zeros(4, 0, device='cuda'),
                      torch.ones(4, 1, device='cuda'), fused=fused)
    assert all(out[key].shape == (4, 0) and out[key].dtype == torch.float32 for key in OUTPUTS)
    out['loss'].sum().backward()
    assert single.grad.shape == (4, 1, 8) and not single.grad.any()
    empty = torch.zeros(0, 3, 8, device='cuda', requires_grad=True)
    out = policy_loss(empty, torch.zeros(0, 3, dtype=torch.int32, device='cuda'), torch.zeros(0, 2, device='cuda'),
                      torch.zeros(0, 3, device='cuda'), fused=fused)
    out['loss'].sum().backward()
    assert out['loss'].shape == (0, 2) and empty.grad.shape == (0, 3, 8)
    assert Categorical(torch.zeros(2, 0, 8, device='cuda'), fused=fused).entropy().shape == (2, 0)
  assert policy_loss_launches() == before + 2
  # Categorical: logp forward + backward two launches, entropy forward one
  dist = Categorical(x, 0.01, dims=1, fused=True)
  dist.logp(args[0]).sum().backward()
  assert policy_loss_launches() == before + 4
  dist.entropy()
  assert policy_loss_launches() == before + 5


def test_refusals():
  x = torch.zeros(3, 4, 8, device='cuda')
  act, adv, weight = torch.zeros(3, 4, dtype=torch.int32, device='cuda'), x[..., :3, 0], x[..., 0]
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    policy_loss(x.cpu(), act, adv, weight)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    Categorical(x.cpu())
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    policy_loss(x.half(), act, adv, weight)
  with pytest.raises(TypeError, match='must be integers'):
    policy_loss(x, act.float(), adv, weight)
  with pytest.raises(ValueError, match='actions of shape'):
    policy_loss(x, act[:, :3], adv, weight)
  with pytest.raises(ValueError, match='adv of shape'):
    policy_loss(x, act, weight, weight)
  with pytest.raises(ValueError, match='weight of shape'):
    policy_loss(x, act, adv, weight[:, :2])
  with pytest.raises(ValueError, match='unimix'):
    policy_loss(x, act, adv, weight, unimix=1.0)
  with pytest.raises(ValueError, match='dims'):
    Categorical(x, dims=2)
