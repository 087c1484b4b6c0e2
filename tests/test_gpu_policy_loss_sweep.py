"""Every instantiation of `policy_loss_kernel<T, W, NPER>` and
`policy_loss_grad_kernel<T, W, NPER>` (csrc/policy_loss.hip): the eight rungs of
EMB_POLICY_BY_WIDTH, float32 and bfloat16, forward and gradient, at the shapes
tests/policy_loss_sweep_cases.py derives from the kernels' constants -- per rung
its first and last class count and the boundaries of the NPER slots, groups 1,
kSegs, kSegs + 1 (a second iteration of the g0 loop with one live segment) and
2 kSegs + 1, no group axis, and (N, T, drop) of (1, 2, 1), (5, 2, 1), (2, 4, 1)
and (5, 1, 0).

Per rung: (a) parity with `tests.policy_loss_cases.reference64` at the bars of
tests/test_gpu_policy_loss.py (forward 1e-5 + 1e-5 |want|; gradient
1e-5 (s + |want|), s the row's scale, bfloat16 plus 2^-8 |want|), the composed
path as the control; (b) a sequence run alone has the bits it has among its
neighbours; (c) the bfloat16 instantiation has the bits of the float32 one on the
same values; (d) `Categorical.logp` / `.entropy` have the bits of logpi and ent,
and one class is exactly 0; (e) every lane as the hit lane, and the actions
outside; (f) through the C ABI, with every output inside a sentinel-filled
allocation at an odd offset, nothing outside the outputs is written.  Once, not
per rung: (g) more rows than one pass of the capped grid.
tests/test_policy_loss_sweep_host.py shows without a GPU that the float32
definition sits inside both bars at every input used here.  Need a GPU."""
import numpy as np
import pytest
import torch

from embodied_amd.outs import Categorical, policy_loss
from embodied_amd import _lib
from tests import policy_loss_cases as cases
from tests import policy_loss_sweep_cases as sweep

pytestmark = pytest.mark.gpu
RUNGS = pytest.mark.parametrize('rung', sweep.RUNGS, ids=[f'W{W}x{nper}' for W, nper in sweep.RUNGS])
OUTPUTS = ('loss', 'logpi', 'ent')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
SENTINEL = -1234.5          # exact in bfloat16
GAP = 321                   # elements of sentinel around an output: more than the kWave * 4 = 256 a wave spans per iteration


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)
  assert GAP > sweep.WAVE * 4


def _host(t):
  return t.detach().float().cpu().numpy()


def _bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_DEVICE = {}


def _upload(d, key, kind, held=None):
  """An input on the device, uploaded once: logits in the dtype of `kind` (or
  `held`: bfloat16-rounded values in float32 tensors), act int32, the rest float32."""
  key = (key, kind, held)
  if key not in _DEVICE:
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('logits', 'act', 'adv', 'weight', 'gout')}
    t['logits'] = t['logits'].to(DTYPES[held or kind])      # exact: the values of kind 'bf16' are bfloat16 numbers
    assert np.array_equal(_host(t['logits']), d['logits'])
    _DEVICE[key] = t
  return _DEVICE[key]


def _device(groups, classes, n, t, drop, scale, kind, held=None):
  return _upload(sweep.data(groups, classes, n, t, drop, scale, kind), (groups, classes, n, t, drop, scale), kind, held)


def _run(t, d, unimix, fused, cut=False, n=None):
  """`policy_loss` with backward over the device inputs `t` of `d` (or over a
  copy of their sequence `n` alone): the three outputs (N, T - drop) and the
  gradient, on the device."""
  pick = (lambda x: x) if n is None else (lambda x: x[n:n + 1].clone())
  kept = d['logits'].shape[1] - d['drop']
  x = pick(t['logits']).detach().requires_grad_()
  weight = pick(t['weight'][:, :kept] if cut else t['weight'])
  out = policy_loss(x, pick(t['act']), pick(t['adv']), weight, actent=sweep.ACTENT, unimix=unimix, dims=d['dims'],
                    drop_last=bool(d['drop']), fused=fused)
  gout = pick(t['gout'])
  (out['loss'] * gout).sum().backward()
  got = {k: out[k].detach() for k in OUTPUTS}
  assert all(v.dtype == torch.float32 and v.shape == gout.shape for v in got.values())
  assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
  got['grad'] = x.grad
  return got


_FUSED = {}


def _fused(groups, classes, n, t, drop, scale, kind, unimix):
  """The kernels' run of one sweep input through the facade, made once: what
  (a) holds against float64 and (b), (c), (d) and (f) compare bits with."""
  key = (groups, classes, n, t, drop, scale, kind, unimix)
  if key not in _FUSED:
    d = sweep.data(groups, classes, n, t, drop, scale, kind)
    _FUSED[key] = _run(_device(groups, classes, n, t, drop, scale, kind), d, unimix, True,
                       sweep.cut_weight(n, t, drop, unimix, scale))
  return _FUSED[key]


def _ratios(d, got, ref, kind):
  return sweep.ratios(d, {k: _host(got[k]) for k in OUTPUTS}, _host(got['grad']), ref, kind == 'bf16')


def _title(rung):
  return f'W = {rung[0]}, NPER = {rung[1]} (kSegs {sweep.segments(rung)})'


@RUNGS
def test_parity_at_every_shape_of_the_rung(rung):
  """(a) Every shape of the rung, every geometry, both dtypes, every setting,
  weight as (N, T) and as (N, T - drop): the three outputs and the gradient of
  the kernels against float64, a dropped step's gradient exactly zero; the other
  layout of weight and the composed path at groups kSegs + 1 of every class
  count as the controls."""
  worst, control, controls = [0.0, 0.0], [0.0, 0.0], []
  for groups, classes in sweep.shapes(rung):
    assert sweep.width(classes) == rung
    composed = groups == sweep.control_groups(classes)
    controls += [f'{groups}x{classes}'] if composed else []
    for n, t, drop in sweep.GEOMETRIES:
      for kind in sweep.KINDS:
        for unimix, scale in sweep.SETTINGS:
          where = (groups, classes, n, t, drop, kind, unimix, scale)
          d = sweep.data(groups, classes, n, t, drop, scale, kind)
          ref = sweep.reference(d, unimix)
          got = _fused(groups, classes, n, t, drop, scale, kind, unimix)
          ratios = _ratios(d, got, ref, kind)            # asserts the zeros of a dropped step
          assert max(ratios) <= 1.0, ('fused', *where, ratios)
          worst = [max(a, b) for a, b in zip(worst, ratios)]
          if composed:
            dev = _device(groups, classes, n, t, drop, scale, kind)
            other = _run(dev, d, unimix, True, not sweep.cut_weight(n, t, drop, unimix, scale))
            assert all(_same_bits(other[k], got[k]) for k in OUTPUTS + ('grad',)), ('weight layout', *where)
            ratios = _ratios(d, _run(dev, d, unimix, False), ref, kind)
            assert max(ratios) <= 1.0, ('composed', *where, ratios)
            control = [max(a, b) for a, b in zip(control, ratios)]
  print(f'{_title(rung)}: ' + ' '.join(f'{g}x{c}' for g, c in sweep.shapes(rung)) + f': fused forward '
        f'{worst[0]:.3g}, gradient {worst[1]:.3g} of their bars; composed at ' + ' '.join(controls) +
        f': forward {control[0]:.3g}, gradient {control[1]:.3g}')


@RUNGS
def test_a_sequence_alone_has_the_bits_it_has_among_its_neighbours(rung):
  """(b) Every shape of the rung at (N, T, drop) = (5, 2, 1), every dtype and
  setting: each n run alone (its own allocation, one kept row and one dropped)
  gives the bits of that n in all three outputs and in the gradient -- what
  another row or another segment leaked into a row would change, inside the
  tolerance or not."""
  n, t, drop = sweep.ALONE
  for groups, classes in sweep.shapes(rung):
    for kind in sweep.KINDS:
      for unimix, scale in sweep.SETTINGS:
        together = _fused(groups, classes, n, t, drop, scale, kind, unimix)
        d = sweep.data(groups, classes, n, t, drop, scale, kind)
        dev = _device(groups, classes, n, t, drop, scale, kind)
        alone = [_run(dev, d, unimix, True, n=i) for i in range(n)]
        for key in OUTPUTS + ('grad',):
          assert _same_bits(torch.cat([a[key] for a in alone]), together[key]), (key, groups, classes, kind, unimix, scale)


@RUNGS
def test_bfloat16_instantiation_has_the_bits_of_the_float32_one(rung):
  """(c) The two instantiations differ in `load` and `store` alone: the float32
  kernels over the bfloat16 inputs' values held in float32 tensors give the
  forward outputs of the bfloat16 run bit for bit, and a gradient whose rounding
  to bfloat16 has the bits of the bfloat16 gradient.  Finite inputs."""
  for groups, classes in sweep.shapes(rung):
    for n, t, drop in sweep.GEOMETRIES:
      for unimix, scale in sweep.SETTINGS:
        where = (groups, classes, n, t, drop, unimix, scale)
        narrow = _fused(groups, classes, n, t, drop, scale, 'bf16', unimix)
        d = sweep.data(groups, classes, n, t, drop, scale, 'bf16')
        wide = _run(_device(groups, classes, n, t, drop, scale, 'bf16', held='f32'), d, unimix, True)
        for key in OUTPUTS:
          assert _same_bits(wide[key], narrow[key]), (key, *where)
        assert wide['grad'].dtype == torch.float32 and narrow['grad'].dtype == torch.bfloat16
        assert torch.isfinite(wide['grad']).all(), where
        assert _same_bits(wide['grad'].to(torch.bfloat16), narrow['grad']), ('grad', *where)


@RUNGS
def test_facade_identities(rung):
  """(d) At groups kSegs + 1 of every class count, geometry (5, 1, 0), both
  dtypes: `Categorical.logp(act)` has the bits of the logpi output and
  `Categorical.entropy()` those of ent; with adv = weight = 1 and actent = 0 the
  loss has the bits of -logpi; one class: logpi, ent and the gradient are
  exactly 0."""
  n, t, drop = sweep.GEOMETRIES[-1]
  assert drop == 0
  for classes in sweep.CLASSES[rung]:
    groups = sweep.control_groups(classes)
    for kind in sweep.KINDS:
      for unimix, scale in sweep.SETTINGS:
        where = (groups, classes, kind, unimix, scale)
        dev = _device(groups, classes, n, t, drop, scale, kind)
        want = _fused(groups, classes, n, t, drop, scale, kind, unimix)
        dist = Categorical(dev['logits'], unimix, dims=1, fused=True)
        assert dist.fused is True
        assert _same_bits(dist.logp(dev['act']), want['logpi']), ('logp', *where)
        assert _same_bits(dist.entropy(), want['ent']), ('entropy', *where)
        ones = torch.ones_like(dev['adv'])
        plain = policy_loss(dev['logits'], dev['act'], ones, ones, actent=0.0, unimix=unimix, dims=1, drop_last=False,
                            fused=True)
        assert _same_bits(plain['loss'], -want['logpi']) and _same_bits(plain['logpi'], want['logpi']), ('loss', *where)
        if classes == 1:
          assert (want['logpi'] == 0).all() and (want['ent'] == 0).all() and (want['grad'] == 0).all(), where
          assert (want['loss'] == 0).all(), where


@RUNGS
def test_every_lane_as_the_hit_lane(rung):
  """(e) N = classes + 2 rows, T = 1, nothing dropped, groups kSegs + 1: row r's
  action in every group is r - 1, so the actions run over -1 .. classes and
  every lane and every slot of NPER is the hit once.  float32, unimix 0.01 and 0:
  logpi and the gradient against float64; the first and the last row match no
  lane, so their logpi is exactly 0 and their gradient is the entropy's alone."""
  worst = [0.0, 0.0]
  for classes in sweep.CLASSES[rung]:
    d = sweep.hit_data(classes, 1.0)
    dev = _upload(d, ('hit', classes), 'f32')
    n = classes + 2
    s = cases.row_scale(d['gout'], d['weight'], d['adv'], sweep.ACTENT)
    for unimix in (0.01, 0.0):
      got = _run(dev, d, unimix, True)
      ref = sweep.reference(d, unimix)
      ratios = _ratios(d, got, ref, 'f32')
      assert max(ratios) <= 1.0, (classes, unimix, ratios)
      worst = [max(a, b) for a, b in zip(worst, ratios)]
      logpi, grad = _host(got['logpi']), _host(got['grad'])
      assert logpi[0, 0] == 0 and logpi[n - 1, 0] == 0, (classes, unimix)
      assert classes == 1 or (logpi[1:n - 1, 0] < 0).all(), (classes, unimix)
      none = sweep.reference(d, unimix, act=False)
      for row in (0, n - 1):
        assert cases.grad_ratio(grad[row], none['grad'][row], s[row]) <= 1.0, (classes, unimix, row)
  print(f'{_title(rung)}, every lane the hit lane: forward {worst[0]:.3g}, gradient {worst[1]:.3g} of their bars')


def _odd(at):
  return at | 1


@RUNGS
def test_nothing_is_written_outside_the_outputs(rung):
  """(f) `emb_policy_loss` and `emb_policy_loss_grad` through the C ABI at groups
  kSegs + 1 and (N, T, drop) = (5, 2, 1) -- the last iteration of every row has
  dead segments, there are padding lanes wherever classes < W NPER, and every
  second row of the gradient is a dropped step's zero fill -- with loss, logpi
  and ent and the gradient each at an odd element offset inside an allocation
  filled with a sentinel, weight with a row stride of T: afterwards everything
  outside the outputs is the sentinel, no output element is, and the outputs
  have the bits of the facade's run."""
  n, t, drop = sweep.ALONE
  rows = n * (t - drop)
  for classes in sweep.CLASSES[rung]:
    groups = sweep.control_groups(classes)
    count = n * t * groups * classes
    for kind in sweep.KINDS:
      for unimix, scale in sweep.SETTINGS:
        where = (groups, classes, kind, unimix, scale)
        dev = _device(groups, classes, n, t, drop, scale, kind)
        want = _fused(groups, classes, n, t, drop, scale, kind, unimix)
        small = torch.full((3 * rows + 4 * GAP + 1,), SENTINEL, device='cuda')
        starts = [_odd(GAP + i * (rows + GAP)) for i in range(3)]
        loss, logpi, ent = (small[at:at + rows] for at in starts)
        large = torch.full((count + 2 * GAP + 1,), SENTINEL, dtype=DTYPES[kind], device='cuda')
        spot = _odd(GAP)
        grad = large[spot:spot + count]
        for view in (loss, logpi, ent, grad):
          assert (view.data_ptr() // view.element_size()) % 2 == 1 and (view == SENTINEL).all()
        assert dev['weight'].shape == (n, t) and dev['weight'].is_contiguous()
        dtype = _lib.F32 if kind == 'f32' else _lib.BF16
        stream = _lib.raw_stream(small.device)
        _lib.api.emb_policy_loss(dev['logits'].data_ptr(), dev['act'].data_ptr(), dtype, n, t, drop, groups, classes, unimix,
                                 sweep.ACTENT, dev['adv'].data_ptr(), dev['weight'].data_ptr(), t, loss.data_ptr(),
                                 logpi.data_ptr(), ent.data_ptr(), stream)
        _lib.api.emb_policy_loss_grad(dev['logits'].data_ptr(), dev['act'].data_ptr(), dtype, n, t, drop, groups, classes,
                                      unimix, sweep.ACTENT, dev['adv'].data_ptr(), dev['weight'].data_ptr(), t,
                                      dev['gout'].data_ptr(), grad.data_ptr(), stream)
        inside = torch.zeros_like(small, dtype=torch.bool)
        for at in starts:
          inside[at:at + rows] = True
        assert (small[~inside] == SENTINEL).all() and int((~inside).sum()) == small.numel() - 3 * rows, where
        assert not (small[inside] == SENTINEL).any(), where
        inside = torch.zeros_like(large, dtype=torch.bool)
        inside[spot:spot + count] = True
        assert (large[~inside] == SENTINEL).all() and int((~inside).sum()) == large.numel() - count, where
        assert not (grad == SENTINEL).any(), where                   # the dropped rows too: zeros
        assert not grad.view(n, t, groups, classes)[:, t - drop:].any(), where
        for got, key in ((loss, 'loss'), (logpi, 'logpi'), (ent, 'ent')):
          assert _same_bits(got.view(n, t - drop), want[key]), (key, *where)
        assert _same_bits(grad.view(n, t, groups, classes), want['grad']), ('grad', *where)


@pytest.mark.parametrize('kind', sweep.KINDS)
@pytest.mark.parametrize('groups,classes', sweep.PAST_SHAPES, ids=[f'{g}x{c}' for g, c in sweep.PAST_SHAPES])
def test_rows_beyond_one_sweep_of_the_capped_grid(groups, classes, kind):
  """(g) T = 4 with the last step dropped and N = SWEEP / 3 + 2: the forward's
  N (T - 1) kept rows and the gradient's N T rows both pass the kMaxBlocks *
  kWaves rows one pass of the grid covers, so both kernels' loops run a second
  time -- the forward maps a row by `row / kept`, the gradient by `row / steps`,
  and the dropped step's zero fill is inside the same loop.  Every row against
  float64; the sequences that hold the rows SWEEP - 1, SWEEP and the last row of
  either kernel, run alone, have the same bits."""
  n, t, drop = sweep.PAST_N, sweep.PAST_T, sweep.PAST_DROP
  kept = t - drop
  assert n * kept > sweep.SWEEP and n * t > sweep.SWEEP            # a change of the constants fails here
  assert sweep.SWEEP == sweep.K['kMaxBlocks'] * sweep.K['kWaves']
  unimix, scale = sweep.PAST_SETTING
  d = sweep.data(groups, classes, n, t, drop, scale, kind)
  dev = _device(groups, classes, n, t, drop, scale, kind)
  got = _run(dev, d, unimix, True)
  ratios = _ratios(d, got, sweep.reference(d, unimix), kind)
  print(f'{groups}x{classes} {kind}, {n * kept} kept rows and {n * t} rows of logits against {sweep.SWEEP} per pass: '
        f'forward {ratios[0]:.3g}, gradient {ratios[1]:.3g} of their bars')
  assert max(ratios) <= 1.0, ratios
  rows = (sweep.SWEEP - 1, sweep.SWEEP)
  alone = sorted({row // kept for row in rows + (n * kept - 1,)} | {row // t for row in rows + (n * t - 1,)})
  assert len(alone) >= 4 and alone[-1] == n - 1 and alone[0] < sweep.SWEEP // t + 1 < alone[-2]
  for i in alone:
    one = _run(dev, d, unimix, True, n=i)
    for key in OUTPUTS + ('grad',):
      assert _same_bits(one[key], got[key][i:i + 1]), (key, i)
