"""`embodied_amd.optim.Adam` on the kernels of csrc/optim.hip and as composed
torch ops, after every one of 4 steps, against the float64 run of
`tests.adam_cases.restate`, which is the definition (the host test ties it to
`torch.optim.AdamW` in float64 to 1e-12).  Need a GPU.

Bars, against float64 over the same float32 inputs, every element: p and the
metrics within 1e-5 + 1e-5 |want|, nu within 1e-5 |want| (floor: the smallest
normal float32), mu within 1e-5 (|want| + A) with A the same moving average over
|g1|.  The float32 definition sits inside all of them on every list
(tests/test_adam_host.py prints its ratios), so no case is exempt.
tools/adam_accuracy.py records the worst ratios in profiles/adam_accuracy.txt.

The last tests run the lists of tests/adam_sweep_cases.py, which take the global-
norm sum, the grid stride of both kernels and the metrics sum past their first
iteration, with the clip regime placed on the chunks only a later iteration
reads and, in the bfloat16 cases of `many`, both gradient dtypes in one list."""
import numpy as np
import pytest
import torch

from embodied_amd.optim import Adam, optimizer_launches        # every test here fails without the feature
from tests import adam_cases as cases
from tests import adam_sweep_cases as sweep

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
CASE_PATHS = [pytest.param(case, fused, id=f'{cases.tag(case)}-{"fused" if fused else "composed"}')
              for case in range(len(cases.CASES)) for fused in (True, False)]


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _place(values, offset, dtype=torch.float32):
  """`values` on the device: a tensor of its own, or (offset given) a view at
  that element offset into a flat buffer."""
  t = torch.from_numpy(np.array(values)).cuda().to(dtype)
  if offset is None:
    return t
  flat = torch.zeros(t.numel() + offset + 5, dtype=dtype, device='cuda')
  view = flat[offset:offset + t.numel()].view(t.shape)
  view.copy_(t)
  return view


def _params(inp, specs):
  return [_place(x, s.poff) for x, s in zip(inp['p'], specs)]


def _set_grads(params, grads, specs, bf16):
  """`bf16`: one flag for every gradient, or a sequence of one per tensor."""
  flags = [bool(bf16)] * len(params) if isinstance(bf16, (bool, np.bool_)) else [bool(flag) for flag in bf16]
  assert len(flags) == len(params) == len(grads) == len(specs)
  for param, g, s, flag in zip(params, grads, specs, flags):
    param.grad_dtype = None                        # a float32 parameter may carry a bfloat16 gradient
    param.grad = _place(g, s.goff, torch.bfloat16 if flag else torch.float32)


def _make_from(specs, inp, h, fused, **kw):
  """An optimizer over `specs` with the parameters of `inp` and the hyper-parameters `h`."""
  params = _params(inp, specs)
  opt = Adam(params, lr=h.lr, clip=h.clip, wd=h.wd, warmup=h.warmup, fused=fused, **kw)
  assert opt.fused is fused
  return opt, params, inp, specs, h


def _make(case, fused, **kw):
  c = cases.CASES[case]
  return _make_from(cases.LISTS[c.list], cases.inputs(case), c.hyper, fused, **kw)


def _first(name, **want):
  """The first case of the list `name` whose hyper-parameters satisfy `want` (truthiness)."""
  return next(i for i, c in enumerate(cases.CASES)
              if c.list == name and all(bool(getattr(c.hyper, k)) == v for k, v in want.items()))


def _gathered(tensors):
  """Every tensor on the host, in one copy however many there are."""
  tensors = [t.detach() for t in tensors]
  flat = torch.cat([t.reshape(-1) for t in tensors]).float().cpu().numpy()
  ends = np.cumsum([t.numel() for t in tensors])
  return [part.reshape(tuple(t.shape)) for part, t in zip(np.split(flat, ends[:-1]), tensors)]


def _state(opt, params):
  return {'p': _gathered(params), 'nu': _gathered([opt.state[p]['nu'] for p in params]),
          'mu': _gathered([opt.state[p]['mu'] for p in params])}


def _run_from(made, steps, grads_of=None):
  """The per-step states (and metrics) of the optimizer `made` (`_make_from`'s) over `steps` steps."""
  opt, params, inp, specs, h = made
  out = []
  for step in range(steps):
    _set_grads(params, inp['g'][step] if grads_of is None else grads_of(step), specs, inp.get('bf16', h.bf16))
    opt.step()
    state = _state(opt, params)
    m = opt.metrics()
    state['metrics'] = np.array([float(m[key]) for key in cases.METRICS])
    assert all(m[key].is_cuda and m[key].dtype == torch.float32 and m[key].dim() == 0 for key in cases.METRICS)
    assert m['updates'] == step + 1 and m['param_count'] == sum(x.size for x in inp['p'])
    assert sorted(m) == sorted(cases.METRICS + ('updates', 'param_count'))
    out.append(state)
  return out


def _run(case, fused, steps=cases.STEPS):
  """The per-step states (and metrics) of a case on one path."""
  return _run_from(_make(case, fused), steps)


def _same_bits(a, b):
  return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for key in ('p', 'nu', 'mu') for x, y in zip(a[key], b[key]))


@pytest.mark.parametrize('case,fused', CASE_PATHS)
def test_against_float64(case, fused):
  """Every element of p, mu and nu and the four metrics after each step."""
  want_all = cases.reference64(case)
  got_all = _run(case, fused)
  assert len(got_all) == len(want_all) == cases.STEPS
  for step, (got, want) in enumerate(zip(got_all, want_all)):
    worst = cases.worst_ratios([got], [want])
    print(f'{cases.tag(case)} {"fused" if fused else "composed"} step {step}: ' +
          ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (step, worst)


@pytest.mark.parametrize('name', ['one', 'seventy', 'wide'])
def test_two_launches_per_step_and_one_for_the_metrics(name):
  case = _first(name)
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
  """No floating-point atomics on any sum, and every workgroup sums the global
  norm in the same order: two optimizers from the same state hold the same bits
  after 4 steps, metrics included."""
  case = _first(name, clip=True)
  a, b = _run(case, True), _run(case, True)
  for x, y in zip(a, b):
    assert _same_bits(x, y) and np.array_equal(x['metrics'], y['metrics'])


def test_views_have_the_bits_of_tensors_allocated_on_their_own():
  """`views`: tensors behind 1 .. 3 scalar elements of a flat buffer and at
  mismatched offsets (every access scalar) against the same tensors each in an
  allocation of its own (vectors from element 0): p, mu and nu have the same bits
  in every tensor.  The case is the one of `views` with the clip switched off:
  which elements a thread adds up within a chunk follows the chunk's alignment,
  so the last bits of a chunk's sum g^2, and with them those of a clipped g1, may
  differ between the two placements (as the metrics' may); the element chain
  itself does not depend on the placement.  The clipped cases of `views` are held
  to float64 in `test_against_float64`."""
  case = _first('views', clip=False)
  c = cases.CASES[case]
  specs = cases.LISTS['views']
  assert any(s.poff for s in specs) and any((s.poff or 0) % 4 != (s.goff or 0) % 4 for s in specs)
  own = tuple(s._replace(poff=None, goff=None) for s in specs)
  a = _run(case, True)
  b = _run_from(_make_from(own, cases.inputs(case), c.hyper, True), cases.STEPS)
  for x, y in zip(a, b):
    assert _same_bits(x, y)
    assert cases.ratio(x['metrics'], y['metrics']) <= 1.0


@PATHS
def test_the_clip_decision_is_global(fused):
  """Two tensors, clip = 10: the first gradient alone has norm 6, below the
  bound; the pair has norm sqrt(6^2 + 12^2) = 13.4, above it.  Both tensors are
  scaled, and by the same factor: after one update from zero moments mu is
  (1 - beta1) g1, so mu / ((1 - beta1) g) is that factor, clip / gnorm, at every
  element of both."""
  rng = np.random.default_rng(5)
  shapes = ((cases.C + 3,), (3, 5))
  raw = [rng.standard_normal(s) for s in shapes]
  grads = [(x * (norm / np.linalg.norm(x.ravel()))).astype(np.float32) for x, norm in zip(raw, (6.0, 12.0))]
  assert np.linalg.norm(grads[0].ravel()) < 10.0 < cases.global_norm(grads)
  factor = 10.0 / cases.global_norm(grads)
  for which, expect in (((0, 1), factor), ((0,), 1.0)):            # the pair; the first tensor alone: not clipped
    params = [torch.zeros(shapes[i], device='cuda') for i in which]
    opt = Adam(params, lr=1e-3, clip=10.0, warmup=0, fused=fused)
    for param, i in zip(params, which):
      param.grad = torch.from_numpy(grads[i]).cuda()
    opt.step()
    for param, i in zip(params, which):
      mu = opt.state[param]['mu'].double().cpu().numpy()
      got = mu / ((1 - cases.BETA1) * grads[i].astype(np.float64))
      assert np.abs(got / expect - 1).max() < 1e-5, (which, i, float(got.min()), float(got.max()), expect)
    assert abs(float(opt.metrics()['grad_norm']) / cases.global_norm([grads[i] for i in which]) - 1) < 1e-5


def _poisoned(case, fused, value, tensor, element):
  """The state after two steps, the second one with `value` at one element of one gradient."""
  made = _make(case, fused)
  inp = made[2]

  def grads_of(step):
    grads = [g.copy() for g in inp['g'][step]]
    if step == 1:
      grads[tensor].reshape(-1)[element] = value
    return grads

  opt, params = made[0], made[1]
  for step in range(2):
    _set_grads(params, grads_of(step), made[3], made[4].bf16)
    opt.step()
  return _state(opt, params)


@PATHS
def test_a_nan_gradient_reaches_every_tensor(fused):
  """One NaN in one element of one gradient: the global norm is NaN, `gnorm <
  clip` is false, g / NaN * clip is NaN: p, mu and nu are NaN in every element of
  every tensor.  The reference's behaviour, unlike LaProp's per-tensor one."""
  case = _first('sizes', clip=True, bf16=False)
  got = _poisoned(case, fused, np.nan, 2, cases.C // 2)
  for key in ('p', 'nu', 'mu'):
    for i, x in enumerate(got[key]):
      assert np.isnan(x).all(), (key, i)


@PATHS
def test_an_infinite_gradient_zeroes_the_finite_elements(fused):
  """One +inf and no NaN: gnorm = inf, g / inf * clip is 0 at every finite
  element of every tensor and NaN at the infinite one.  So mu = beta1 mu and nu =
  beta2 nu of the step before everywhere else, and nothing else is NaN."""
  case = _first('sizes', clip=True, bf16=False)
  tensor, element = 6, cases.C + 3                    # 2C + 5 elements, three chunks
  before = _run(case, fused, steps=1)[0]
  got = _poisoned(case, fused, np.inf, tensor, element)
  for key, beta in (('mu', cases.BETA1), ('nu', cases.BETA2)):
    for i, (x, old) in enumerate(zip(got[key], before[key])):
      mask = np.isnan(x).reshape(-1)
      assert mask.sum() == (1 if i == tensor else 0) and (i != tensor or mask[element]), (key, i, int(mask.sum()))
      want = (np.float32(beta) * old).reshape(-1)[~mask]          # + (1 - beta) * 0
      assert np.array_equal(x.reshape(-1)[~mask], want), (key, i)
  for i, x in enumerate(got['p']):
    mask = np.isnan(x).reshape(-1)
    assert mask.sum() == (1 if i == tensor else 0) and (i != tensor or mask[element]), ('p', i)


@PATHS
def test_state_dict_round_trip_continues_bit_identically(fused):
  case = _first('sizes', warmup=True, wd=True)
  whole = _run(case, fused)
  opt, params, inp, specs, h = _make(case, fused)
  for step in range(2):
    _set_grads(params, inp['g'][step], specs, h.bf16)
    opt.step()
  saved = opt.state_dict()
  fresh_params = [p.clone() for p in params]
  fresh = Adam(fresh_params, lr=h.lr, clip=h.clip, wd=h.wd, warmup=h.warmup, fused=fused)
  fresh.load_state_dict(saved)
  assert fresh.param_groups[0]['updates'] == 2
  for step in range(2, cases.STEPS):
    _set_grads(fresh_params, inp['g'][step], specs, h.bf16)
    fresh.step()
    assert _same_bits(_state(fresh, fresh_params), whole[step]), step


@pytest.mark.parametrize('name', ['sizes', 'seventy'])
def test_reallocated_gradients_refresh_the_table(name):
  """Gradient tensors that come back at other addresses every step, as after
  `zero_grad(set_to_none=True)`, give the bits of gradients written in place; the
  table is uploaded once in place and once per step otherwise."""
  case = _first(name, clip=True)
  moving = _make(case, True)
  still = _make(case, True)
  inp, specs, h = moving[2], moving[3], moving[4]
  _set_grads(still[1], inp['g'][0], specs, h.bf16)
  keep = []                                          # the old gradients stay allocated: the new ones are elsewhere
  for step in range(cases.STEPS):
    keep.append([p.grad for p in moving[1]])
    moving[0].zero_grad(set_to_none=True)
    _set_grads(moving[1], inp['g'][step], specs, h.bf16)
    for param, g in zip(still[1], inp['g'][step]):
      param.grad.copy_(torch.from_numpy(g.copy()).cuda())
    moving[0].step()
    still[0].step()
    assert _same_bits(_state(moving[0], moving[1]), _state(still[0], still[1])), step
  assert still[0].table_uploads == 1 and moving[0].table_uploads == cases.STEPS


def test_a_non_contiguous_parameter_takes_the_composed_path():
  case = _first('two')
  inp, specs = cases.inputs(case), cases.LISTS['two']
  params = _params(inp, specs)
  wide = torch.zeros(3, 2, device='cuda')
  params[1] = wide.t()                               # (1, 3) would be contiguous either way: a (2, 3) transpose
  with pytest.raises(ValueError, match=r'Adam\(fused=True\): parameter 1 of shape \(2, 3\) is not contiguous'):
    Adam(params, fused=True)
  opt = Adam(params, lr=1e-2, warmup=0, fused=None)
  assert opt.fused is False
  before = optimizer_launches()
  params[0].grad = torch.from_numpy(inp['g'][0][0].copy()).cuda()
  params[1].grad = torch.ones(2, 3, device='cuda')
  opt.step()
  assert optimizer_launches() == before
  # Adam's first update is -lr * sign(g) up to eps
  assert torch.allclose(params[1], torch.full((2, 3), -1e-2, device='cuda'), rtol=1e-5)
  contiguous = Adam(_params(inp, specs), fused=None)
  assert contiguous.fused is True


# ---- past the first iteration of the kernels' loops: the lists of tests/adam_sweep_cases.py.  `many` has more
# chunks than kMaxBlocks workgroups, than the metrics kernel has threads and than a workgroup has threads to sum the
# global norm with; `deep` has more than the last.  The clip regime sits on the chunks only a later iteration reads,
# and the bfloat16 cases of `many` mix both gradient dtypes within a workgroup.

SWEEP_PATHS = [pytest.param(case, fused, id=f'{sweep.tag(case)}-{"fused" if fused else "composed"}')
               for case in sweep.CASES for fused in (True, False)]
SWEEP_LISTS = pytest.mark.parametrize('name', ['many', 'deep'])


def _make_sweep(case, fused):
  name, i = case
  h = sweep.HYPERS[name][i]
  return _make_from(sweep.LISTS[name], sweep.inputs(name, h.bf16), h, fused)


def _sweep_first(name, **want):
  """The first sweep case of the list `name` whose hyper-parameters satisfy `want` (truthiness)."""
  return next(case for case in sweep.CASES
              if case[0] == name and all(bool(getattr(sweep.HYPERS[name][case[1]], k)) == v for k, v in want.items()))


@pytest.mark.parametrize('case,fused', SWEEP_PATHS)
def test_sweep_lists_against_float64(case, fused):
  """Every element of p, mu and nu and the four metrics after every step."""
  name = case[0]
  specs = sweep.LISTS[name]
  assert sweep.chunks(sweep.LISTS['many']) > max(sweep.K.values())
  assert sweep.chunks(sweep.LISTS['deep']) > sweep.K['kThreads']
  got_all = _run_from(_make_sweep(case, fused), sweep.STEPS[name])
  want_all = sweep.reference(case)
  assert len(got_all) == len(want_all) == sweep.STEPS[name] and len(got_all[0]['p']) == len(specs)
  for step, (got, want) in enumerate(zip(got_all, want_all)):
    worst = sweep.worst_ratios([got], [want])
    print(f'{sweep.tag(case)} {"fused" if fused else "composed"}, {sweep.chunks(specs)} chunks, step {step}: ' +
          ', '.join(f'{k} {v:.3g}' for k, v in worst.items()) + ' of its bar')
    assert max(worst.values()) <= 1.0, (step, worst)


@SWEEP_LISTS
def test_sweep_lists_take_two_launches_per_step_and_one_for_the_metrics(name):
  case = _sweep_first(name, clip=True)
  opt, params, inp, specs, h = _make_sweep(case, True)
  for step in range(2):
    _set_grads(params, inp['g'][step], specs, inp['bf16'])
    before = optimizer_launches()
    opt.step()
    assert optimizer_launches() == before + 2, len(params)
  opt.metrics()
  assert optimizer_launches() == before + 3
  composed, cparams, _, _, _ = _make_sweep(case, False)
  _set_grads(cparams, inp['g'][0], specs, inp['bf16'])
  before = optimizer_launches()
  composed.step()
  composed.metrics()
  assert optimizer_launches() == before


@SWEEP_LISTS
def test_sweep_lists_identical_state_gives_identical_bits(name):
  """Every workgroup sums all partials in the same order over more than one round
  of its threads, and its own chunks over more than one grid pass: the same bits
  twice, metrics included, with the clip on."""
  case = _sweep_first(name, clip=True)
  a, b = (_run_from(_make_sweep(case, True), sweep.STEPS[name]) for _ in range(2))
  assert len(a) == len(b) == sweep.STEPS[name]
  for x, y in zip(a, b):
    assert _same_bits(x, y) and np.array_equal(x['metrics'], y['metrics'])


def _poisoned_sweep(case, fused, value, tensor, element, at):
  """The optimizer and its state after `at + 1` steps, the last one with `value` at one element of one gradient."""
  opt, params, inp, specs, h = _make_sweep(case, fused)
  assert h.clip and not h.bf16
  for step in range(at + 1):
    grads = [g.copy() for g in inp['g'][step]]
    if step == at:
      grads[tensor].reshape(-1)[element] = value
    _set_grads(params, grads, specs, inp['bf16'])
    opt.step()
  return opt, _state(opt, params)


@PATHS
@pytest.mark.parametrize('name', ['many', 'deep'])
def test_a_nan_only_a_later_loop_iteration_reads_reaches_every_tensor(name, fused):
  """`many`: the NaN is in the gradient of the last tensor, chunk 2 kMaxBlocks + 2:
  its workgroup's third, behind kThreads and kMetricThreads in either sum of the
  partials.  `deep`: in the last element of tensor 0, chunk kThreads + 1, the
  first one the second round of the global-norm sum reads, in the ragged scalar
  tail.  One step with the clip on: p, mu and nu are NaN in every element of
  every tensor and `grad_norm` is NaN."""
  case = _sweep_first(name, clip=True, bf16=False)
  specs = sweep.LISTS[name]
  if name == 'many':
    tensor, element = len(specs) - 1, 0
    assert sweep.chunks(specs[:tensor]) == 2 * sweep.BLOCKS + 2 > max(sweep.K.values())
  else:
    tensor, element = 0, sweep.DEEP - 1
    assert element // cases.C == sweep.K['kThreads'] + 1 and sweep.DEEP % 4 == 3      # past the last whole vector
  opt, got = _poisoned_sweep(case, fused, np.nan, tensor, element, at=0)
  for key in ('p', 'nu', 'mu'):
    assert len(got[key]) == len(specs)
    for i, x in enumerate(got[key]):
      assert np.isnan(x).all(), (key, i)
  assert np.isnan(float(opt.metrics()['grad_norm']))


@PATHS
def test_an_infinity_in_a_second_pass_chunk_zeroes_the_finite_elements(fused):
  """`many`, second step, +inf in tensor kMaxBlocks + 5 (a workgroup's second
  chunk) and no NaN: gnorm = inf, g / inf * clip is 0 at every finite element of
  every tensor and NaN at the infinite one, so mu = beta1 mu and nu = beta2 nu of
  the step before everywhere else, bit for bit."""
  case = _sweep_first('many', clip=True, bf16=False)
  tensor, element = sweep.BLOCKS + 5, 0
  before = _run_from(_make_sweep(case, fused), 1)[0]
  _, got = _poisoned_sweep(case, fused, np.inf, tensor, element, at=1)
  for key, beta in (('mu', cases.BETA1), ('nu', cases.BETA2)):
    for i, (x, old) in enumerate(zip(got[key], before[key])):
      mask = np.isnan(x).reshape(-1)
      assert mask.sum() == (1 if i == tensor else 0) and (i != tensor or mask[element]), (key, i, int(mask.sum()))
      want = (np.float32(beta) * old).reshape(-1)[~mask]          # + (1 - beta) * 0
      assert np.array_equal(x.reshape(-1)[~mask], want), (key, i)
  for i, x in enumerate(got['p']):
    mask = np.isnan(x).reshape(-1)
    assert mask.sum() == (1 if i == tensor else 0) and (i != tensor or mask[element]), ('p', i)


@PATHS
def test_a_gradient_dtype_that_changes_between_steps(fused):
  """`sizes`, clip on: float32 gradients on steps 0 and 2, bfloat16 ones (bf16
  values) on steps 1 and 3, against `restate` in float64 over exactly those
  values.  Each tensor's gradient lives in one buffer read as either dtype, so no
  address changes between the steps: the table is uploaded again, four times in
  all, because a dtype flag differs and for no other reason."""
  plain_case, rounded_case = _first('sizes', clip=True, bf16=False), _first('sizes', clip=True, bf16=True)
  h = cases.CASES[rounded_case].hyper
  specs = cases.LISTS['sizes']
  plain, rounded = cases.inputs(plain_case), cases.inputs(rounded_case)
  assert all(np.array_equal(a, b) for a, b in zip(plain['p'], rounded['p']))
  as_bf16 = (False, True, False, True)
  inp = {'p': plain['p'], 'g': [(rounded if flag else plain)['g'][step] for step, flag in enumerate(as_bf16)]}
  for step, flag in enumerate(as_bf16):
    assert cases.regime(inp['g'][step], h.clip)[1] >= cases.MARGIN
    assert all(np.array_equal(g, cases.bf16_round(g).reshape(g.shape)) for g in inp['g'][step]) == flag
  want_all = cases.restate(inp, h, specs, torch.float64)
  opt, params, _, _, _ = _make_from(specs, inp, h, fused)
  buffers = [torch.zeros(max(x.size, 1), dtype=torch.float32, device='cuda') for x in inp['p']]
  before = optimizer_launches()
  got_all, addresses = [], []
  for step, flag in enumerate(as_bf16):
    for param, buffer, g in zip(params, buffers, inp['g'][step]):
      view = (buffer.view(torch.bfloat16) if flag else buffer)[:g.size].view(g.shape)
      view.copy_(torch.from_numpy(g.copy()).cuda())          # bfloat16 values: the narrowing is exact
      param.grad_dtype = None
      param.grad = view
    addresses.append([param.grad.data_ptr() for param in params])
    assert {param.grad.dtype for param in params} == {torch.bfloat16 if flag else torch.float32}
    opt.step()
    state = _state(opt, params)
    m = opt.metrics()
    state['metrics'] = np.array([float(m[key]) for key in cases.METRICS])
    got_all.append(state)
  assert all(a == addresses[0] for a in addresses)
  for step, (got, want) in enumerate(zip(got_all, want_all)):
    worst = cases.worst_ratios([got], [want])
    print(f'sizes, dtype per step {as_bf16}, {"fused" if fused else "composed"} step {step}: ' +
          ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (step, worst)
  if fused:
    assert opt.table_uploads == 4 and optimizer_launches() == before + 3 * 4
  else:
    assert opt.table_uploads == 0 and optimizer_launches() == before
