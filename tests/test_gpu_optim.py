"""`embodied_amd.optim.LaProp` on the kernels of csrc/optim.hip and as composed
torch ops, after every one of 4 steps, against the float64 run of the reference's
own `clip_by_agc`, `scale_by_rms` and `scale_by_momentum` (tests/golden/optim.npz:
the metrics and the sampled elements) and, for every element, against
`tests.optim_cases.reference64` (which the host test holds against that fixture
to 1e-12).  Need a GPU.

Bars, against float64 over the same float32 inputs: p, mu and the metrics within
1e-5 + 1e-5 |want|, nu within 1e-5 |want| (floor: the smallest normal float32).
The float32 definition sits inside all of them on every list
(tests/test_optim_host.py prints its ratios), so no case is exempt.
tools/optim_accuracy.py records the worst ratios in profiles/optim_accuracy.txt.

The last tests run the lists of tests/optim_sweep_cases.py, which take each
kernel's loops past their first iteration (more chunks than workgroups, than a
workgroup's threads, than the metrics kernel's threads), against `reference64`
at the same bars."""
import pathlib

import numpy as np
import pytest
import torch

from embodied_amd.optim import LaProp, optimizer_launches        # every test here fails without the feature
from tests import optim_cases as cases
from tests import optim_sweep_cases as sweep

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'optim.npz'
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
CASE_PATHS = [pytest.param(case, fused, id=f'{cases.tag(case)}-{"fused" if fused else "composed"}')
              for case in range(len(cases.CASES)) for fused in (True, False)]


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


_REF = {}


def _reference(case):
  """`reference64` of a case, computed once and shared by both paths."""
  if case not in _REF:
    c = cases.CASES[case]
    _REF[case] = cases.reference64(cases.inputs(case), c.hyper, cases.LISTS[c.list])
  return _REF[case]


def _place(values, offset, dtype=torch.float32):
  """`values` on the device: a tensor of its own, or (offset given) a view at
  that element offset into a flat buffer."""
  t = torch.from_numpy(np.ascontiguousarray(values)).cuda().to(dtype)
  if offset is None:
    return t
  flat = torch.zeros(t.numel() + offset + 5, dtype=dtype, device='cuda')
  view = flat[offset:offset + t.numel()].view(t.shape)
  view.copy_(t)
  return view


def _params(inp, specs):
  return [_place(x, s.poff) for x, s in zip(inp['p'], specs)]


def _set_grads(params, grads, specs, bf16):
  for param, g, s in zip(params, grads, specs):
    param.grad_dtype = None                        # a float32 parameter may carry a bfloat16 gradient
    param.grad = _place(g, s.goff, torch.bfloat16 if bf16 else torch.float32)


def _make_from(specs, inp, h, fused, **kw):
  """An optimizer over `specs` with the parameters of `inp` and the hyper-parameters `h`."""
  params = _params(inp, specs)
  opt = LaProp(params, lr=h.lr, agc=h.agc, wd=h.wd, nesterov=h.nesterov, warmup=h.warmup, fused=fused, **kw)
  assert opt.fused is fused
  return opt, params, inp, specs, h


def _make(case, fused, **kw):
  c = cases.CASES[case]
  return _make_from(cases.LISTS[c.list], cases.inputs(case), c.hyper, fused, **kw)


def _host(t):
  return t.detach().float().cpu().numpy()


def _gathered(tensors):
  """Every tensor on the host, in one copy however many there are."""
  tensors = [t.detach() for t in tensors]
  flat = _host(torch.cat([t.reshape(-1) for t in tensors]))
  ends = np.cumsum([t.numel() for t in tensors])
  return [part.reshape(tuple(t.shape)) for part, t in zip(np.split(flat, ends[:-1]), tensors)]


def _state(opt, params):
  return {'p': _gathered(params), 'nu': _gathered([opt.state[p]['nu'] for p in params]),
          'mu': _gathered([opt.state[p]['mu'] for p in params])}


def _run_from(made, steps):
  """The per-step states (and metrics) of the optimizer `made` (`_make_from`'s) over `steps` steps."""
  opt, params, inp, specs, h = made
  out = []
  for step in range(steps):
    _set_grads(params, inp['g'][step], specs, h.bf16)
    opt.step()
    state = _state(opt, params)
    m = opt.metrics()
    state['metrics'] = np.array([float(m[key]) for key in cases.METRICS])
    assert all(m[key].is_cuda and m[key].dtype == torch.float32 and m[key].dim() == 0 for key in cases.METRICS)
    assert m['updates'] == step + 1 and m['param_count'] == sum(x.size for x in inp['p'])
    out.append(state)
  return out


def _run(case, fused, steps=cases.STEPS):
  """The per-step states (and metrics) of a case on one path."""
  return _run_from(_make(case, fused), steps)


def _same_bits(a, b):
  return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for key in ('p', 'nu', 'mu') for x, y in zip(a[key], b[key]))


@pytest.mark.parametrize('case,fused', CASE_PATHS)
def test_against_float64(golden, case, fused):
  want_all = _reference(case)
  fixture = cases.unpack(golden[f'out64_{cases.tag(case)}'])
  got_all = _run(case, fused)
  for step, (got, want) in enumerate(zip(got_all, want_all)):
    worst = {}
    for key in ('p', 'nu', 'mu'):
      bar = cases.ratio_nu if key == 'nu' else cases.ratio
      worst[key] = max([bar(g, w) for g, w in zip(got[key], want[key])], default=0.0)           # every element
      worst[key + ' (fixture)'] = bar(cases.sampled(got[key]), fixture[key][step])              # the reference's own run
    worst['metrics'] = cases.ratio(got['metrics'], fixture['metrics'][step])
    print(f'{cases.tag(case)} {"fused" if fused else "composed"} step {step}: ' +
          ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (step, worst)


@pytest.mark.parametrize('name', ['one', 'seventy'])
def test_two_launches_per_step_and_one_for_the_metrics(name):
  case = next(i for i, c in enumerate(cases.CASES) if c.list == name)
  opt, params, inp, specs, h = _make(case, True)
  for step in range(3):
    _set_grads(params, inp['g'][step], specs, h.bf16)
    before = optimizer_launches()
    opt.step()
    assert optimizer_launches() == before + 2, len(params)
  opt.metrics()
  assert optimizer_launches() == before + 3
  composed, cparams, _, _, _ = _make(case, False)
  _set_grads(cparams, inp['g'][0], specs, h.bf16)
  before = optimizer_launches()
  composed.step()
  composed.metrics()
  assert optimizer_launches() == before


@pytest.mark.parametrize('name', ['sizes', 'views', 'wide'])
def test_identical_state_gives_identical_bits(name):
  """No floating-point atomics on any sum: two optimizers from the same state
  hold the same bits after 4 steps, metrics included."""
  case = next(i for i, c in enumerate(cases.CASES) if c.list == name and c.hyper.agc)
  a, b = _run(case, True), _run(case, True)
  for x, y in zip(a, b):
    assert _same_bits(x, y) and np.array_equal(x['metrics'], y['metrics'])


@pytest.mark.parametrize('name', ['sizes', 'seventy'])
def test_reallocated_gradients_refresh_the_table(name):
  """Gradient tensors that come back at other addresses every step give the
  bits of gradients written in place; the table is uploaded once in place and
  once per step otherwise."""
  case = next(i for i, c in enumerate(cases.CASES) if c.list == name and c.hyper.agc)
  moving = _make(case, True)
  still = _make(case, True)
  inp, specs, h = moving[2], moving[3], moving[4]
  _set_grads(still[1], inp['g'][0], specs, h.bf16)
  keep = []                                          # the old gradients stay allocated: the new ones are elsewhere
  for step in range(cases.STEPS):
    keep.append([p.grad for p in moving[1]])
    _set_grads(moving[1], inp['g'][step], specs, h.bf16)
    for param, g in zip(still[1], inp['g'][step]):
      param.grad.copy_(torch.from_numpy(g).cuda())
    moving[0].step()
    still[0].step()
    assert _same_bits(_state(moving[0], moving[1]), _state(still[0], still[1])), step
  assert still[0].table_uploads == 1 and moving[0].table_uploads == cases.STEPS


@PATHS
def test_state_dict_round_trip_continues_bit_identically(fused):
  case = next(i for i, c in enumerate(cases.CASES) if c.list == 'sizes' and c.hyper.warmup and c.hyper.wd)
  whole = _run(case, fused)
  opt, params, inp, specs, h = _make(case, fused)
  for step in range(2):
    _set_grads(params, inp['g'][step], specs, h.bf16)
    opt.step()
  saved = opt.state_dict()
  fresh_params = [p.clone() for p in params]
  fresh = LaProp(fresh_params, lr=h.lr, agc=h.agc, wd=h.wd, nesterov=h.nesterov, warmup=h.warmup, fused=fused)
  fresh.load_state_dict(saved)
  assert fresh.param_groups[0]['updates'] == 2
  for step in range(2, cases.STEPS):
    _set_grads(fresh_params, inp['g'][step], specs, h.bf16)
    fresh.step()
    assert _same_bits(_state(fresh, fresh_params), whole[step]), step


def test_non_finite_gradients_stay_in_their_tensor():
  """One NaN in one tensor, one +inf in another, at the second step: the NaN
  tensor's p, nu and mu are NaN throughout; the inf tensor's scale is 0, so its
  finite elements go on with g1 = 0 and the infinite one becomes NaN; both paths
  agree on the NaN mask, and every other tensor has the bits of the clean run."""
  case = next(i for i, c in enumerate(cases.CASES) if c.list == 'sizes' and c.hyper.agc and not c.hyper.bf16)
  specs = cases.LISTS['sizes']
  nan_at, inf_at = 2, 6                              # C - 1 elements; 2C + 5 elements, three chunks
  runs = {}
  for fused in (True, False):
    clean = _run(case, fused, steps=2)[-1]
    opt, params, inp, _, h = _make(case, fused)
    for step in range(2):
      grads = [g.copy() for g in inp['g'][step]]
      if step == 1:
        grads[nan_at].reshape(-1)[cases.C // 2] = np.nan
        grads[inf_at].reshape(-1)[cases.C + 3] = np.inf
      _set_grads(params, grads, specs, h.bf16)
      opt.step()
    got = _state(opt, params)
    for key in ('p', 'nu', 'mu'):
      assert np.isnan(got[key][nan_at]).all(), key
      mask = np.isnan(got[key][inf_at]).reshape(-1)
      assert mask[cases.C + 3] and mask.sum() == 1, (key, int(mask.sum()))
      for i in range(len(specs)):
        if i not in (nan_at, inf_at):
          assert np.array_equal(got[key][i].view(np.uint32), clean[key][i].view(np.uint32)), (key, i)
    # the finite elements of the inf tensor: g1 = 0, so nu = beta2 * nu and mu = beta1 * mu of the step before
    runs[fused] = got
  for key in ('p', 'nu', 'mu'):
    for a, b in zip(runs[True][key], runs[False][key]):
      assert np.array_equal(np.isnan(a), np.isnan(b)), key
  finite = np.ones(specs[inf_at].shape[0], bool)
  finite[cases.C + 3] = False
  for key in ('nu', 'mu'):
    a, b = runs[True][key][inf_at][finite], runs[False][key][inf_at][finite]
    assert cases.ratio(a, b.astype(np.float64)) <= 1.0


def test_a_non_contiguous_parameter_takes_the_composed_path():
  case = next(i for i, c in enumerate(cases.CASES) if c.list == 'two')
  c = cases.CASES[case]
  inp, specs, h = cases.inputs(case), cases.LISTS['two'], c.hyper
  params = _params(inp, specs)
  wide = torch.zeros(3, 2, device='cuda')
  params[1] = wide.t()                               # (1, 3) would be contiguous either way: a (2, 3) transpose
  with pytest.raises(ValueError, match=r'fused=True.*parameter 1 of shape \(2, 3\) is not contiguous'):
    LaProp(params, fused=True)
  opt = LaProp(params, lr=1e-2, fused=None)
  assert opt.fused is False
  before = optimizer_launches()
  params[0].grad = torch.from_numpy(inp['g'][0][0]).cuda()
  params[1].grad = torch.ones(2, 3, device='cuda')
  opt.step()
  assert optimizer_launches() == before
  # LaProp's first update of a lone tensor: -lr * sign(g) up to the clipping, here below 1 in size
  assert torch.isfinite(params[1]).all() and (params[1] < 0).all() and float(params[1].abs().max()) <= 1e-2 * 1.001


# ---- past the first iteration of the kernels' loops: the lists of tests/optim_sweep_cases.py.  `many` has more
# chunks than kMaxBlocks workgroups (a workgroup meets a second tensor, in another AGC regime) and than the
# metrics kernel has threads; `deep` has a tensor of more chunks than a workgroup has threads to sum them with.

SWEEP_PATHS = [pytest.param(case, fused, id=f'{sweep.tag(case)}-{"fused" if fused else "composed"}')
               for case in sweep.CASES for fused in (True, False)]


def _make_sweep(case, fused):
  name, i = case
  h = sweep.HYPERS[name][i]
  return _make_from(sweep.LISTS[name], sweep.inputs(name, h.bf16), h, fused)


def _first(name, agc=True):
  return next(case for case in sweep.CASES if case[0] == name and bool(sweep.HYPERS[name][case[1]].agc) == agc)


@pytest.mark.parametrize('case,fused', SWEEP_PATHS)
def test_sweep_lists_against_float64(case, fused):
  """Every element of p, nu and mu and the four metrics after every step."""
  name = case[0]
  specs = sweep.LISTS[name]
  assert sweep.chunks(sweep.LISTS['many']) > max(sweep.K['kMaxBlocks'], sweep.K['kMetricThreads'])
  assert max(-(-int(np.prod(s.shape)) // cases.C) for s in sweep.LISTS['deep']) > sweep.K['kThreads']
  got_all = _run_from(_make_sweep(case, fused), sweep.STEPS[name])
  want_all = sweep.reference(case)
  assert len(got_all) == len(want_all) == sweep.STEPS[name] and len(got_all[0]['p']) == len(specs)
  worst = sweep.worst_ratios(got_all, want_all)
  print(f'{sweep.tag(case)} {"fused" if fused else "composed"}, {sweep.chunks(specs)} chunks: ' +
        ', '.join(f'{k} {v:.3g}' for k, v in worst.items()) + ' of its bar')
  assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('name', ['many', 'deep'])
def test_sweep_lists_take_two_launches_per_step_and_one_for_the_metrics(name):
  opt, params, inp, specs, h = _make_sweep(_first(name), True)
  for step in range(2):
    _set_grads(params, inp['g'][step], specs, h.bf16)
    before = optimizer_launches()
    opt.step()
    assert optimizer_launches() == before + 2, len(params)
  opt.metrics()
  assert optimizer_launches() == before + 3
  composed, cparams, _, _, _ = _make_sweep(_first(name), False)
  _set_grads(cparams, inp['g'][0], specs, h.bf16)
  before = optimizer_launches()
  composed.step()
  composed.metrics()
  assert optimizer_launches() == before


@pytest.mark.parametrize('name', ['many', 'deep'])
def test_sweep_lists_identical_state_gives_identical_bits(name):
  case = _first(name)
  a, b = (_run_from(_make_sweep(case, True), sweep.STEPS[name]) for _ in range(2))
  for x, y in zip(a, b):
    assert _same_bits(x, y) and np.array_equal(x['metrics'], y['metrics'])


@PATHS
def test_a_nan_gradient_stays_out_of_the_tensor_that_shares_its_workgroup(fused):
  """`many`: tensor 0 and tensor kMaxBlocks are chunk 0 and chunk kMaxBlocks, the
  same workgroup's first and second on the kernels.  A NaN in tensor 0's gradient
  makes its scale NaN; tensor kMaxBlocks, and every other tensor, keeps the bits
  of the clean run."""
  case = _first('many')
  blocks = sweep.BLOCKS
  clean = _run_from(_make_sweep(case, fused), 1)[-1]
  opt, params, inp, specs, h = _make_sweep(case, fused)
  assert h.agc and len(params) > blocks
  grads = [g.copy() for g in inp['g'][0]]
  grads[0].reshape(-1)[0] = np.nan
  _set_grads(params, grads, specs, h.bf16)
  opt.step()
  got = _state(opt, params)
  for key in ('p', 'nu', 'mu'):
    assert np.isnan(got[key][0]).all(), key
    for i in range(1, len(specs)):
      assert np.array_equal(got[key][i].view(np.uint32), clean[key][i].view(np.uint32)), (key, i)
    assert np.isfinite(got[key][blocks]).all()
