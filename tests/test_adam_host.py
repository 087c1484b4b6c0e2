"""`embodied_amd.optim.Adam`, `emb_optim_grad_norms` and `emb_optim_adam_update`
as far as they go without a GPU: the declarations and the binding, the definition
(tests/adam_cases.py: `restate`) against an independent implementation, the bars,
what the cases cover, the composed path over host tensors, the refusals that
happen before any launch, and `LaProp`'s unchanged surface.  CPU only."""
import ctypes as C
import inspect
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import adam_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ('emb_optim_grad_norms', 'emb_optim_adam_update')


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  from embodied_amd.optim import Adam                      # fails without the feature
  from tests.test_abi_symbols import declared_symbols
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'ppo/agent.py:114-124' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [5, 15]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  count = len(declared_symbols())
  assert f'it exports ({count} functions)' in text
  assert f'the C ABI ({count} entry points' in (ROOT / 'README.md').read_text()
  assert emb.Adam is Adam and issubclass(Adam, torch.optim.Optimizer)
  # the host sanitizer soak links kernels_abi.cpp against stand-in launchers: nothing of the optimizer is in it
  assert 'optim' not in (ROOT / 'embodied_amd' / 'csrc' / 'kernels_abi.cpp').read_text()
  soak = (ROOT / 'tools' / 'run_sanitizers.sh').read_text()
  assert 'optim_abi.cpp' not in soak
  kernel = (ROOT / 'embodied_amd' / 'csrc' / 'optim.hip').read_text()
  assert 'atomicAdd' not in kernel and 'cooperative' not in kernel.lower()
  assert 'optim_adam_update_kernel' in kernel and 'optim_norms_kernel<false>' in kernel


def _clip_coefficient(grads, clip):
  """optax.clip_by_global_norm by hand, in float64: what every gradient is multiplied by."""
  norm = np.sqrt(sum(np.square(g.astype(np.float64)).sum() for g in grads))
  return 1.0 if not clip or norm < clip else clip / norm


def _adamw_run(case):
  """p after every step from `torch.optim.AdamW` in float64 on the CPU."""
  c = cases.CASES[case]
  out = adamw_run_over(cases.inputs(case), cases.LISTS[c.list], c.hyper)
  assert len(out) == cases.STEPS
  return out


def adamw_run_over(inp, specs, h):
  """The same over any inputs, tensor list and hyper-parameters (tests/test_adam_sweep_host.py runs its lists through it)."""
  params = [torch.from_numpy(x.copy()).double() for x in inp['p']]
  mask = cases.mask_of(specs)
  groups = [{'params': [p for p, m in zip(params, mask) if m], 'weight_decay': h.wd},
            {'params': [p for p, m in zip(params, mask) if not m], 'weight_decay': 0.0}]
  opt = torch.optim.AdamW([g for g in groups if g['params']], lr=1.0, betas=(cases.BETA1, cases.BETA2), eps=cases.EPS)
  out = []
  for step in range(len(inp['g'])):
    coefficient = _clip_coefficient(inp['g'][step], h.clip)
    for param, g in zip(params, inp['g'][step]):
      param.grad = torch.from_numpy(g.astype(np.float64) * coefficient)
    for group in opt.param_groups:
      group['lr'] = cases.schedule(h.lr, h.warmup, step)
    opt.step()
    out.append([p.detach().numpy().copy() for p in params])
  return out


def test_the_restatement_equals_an_independent_implementation():
  """`restate` in float64 against torch's AdamW over hand-clipped gradients, p
  after each of the four steps of every case, to 1e-12.  (torch's own
  `clip_grad_norm_` is not the comparison: it adds 1e-6 to the norm.)"""
  for case in range(len(cases.CASES)):
    want = _adamw_run(case)
    mine = cases.reference64(case)
    assert len(mine) == len(want) == cases.STEPS
    for step in range(cases.STEPS):
      for i, (a, b) in enumerate(zip(mine[step]['p'], want[step])):
        assert a.dtype == np.float64 and a.shape == b.shape
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12), (cases.tag(case), step, i, float(np.abs(a - b).max(initial=0)))


def test_float32_definition_against_the_bars():
  """`restate` in float32 on the CPU against its float64 run over every case:
  the worst ratio per list and quantity, printed.  A (list, quantity) that
  misses must be in `cases.EXEMPT` with its reason; nothing else may miss."""
  worst = {}
  for case, c in enumerate(cases.CASES):
    got = cases.restate(cases.inputs(case), c.hyper, cases.LISTS[c.list], torch.float32)
    for key, value in cases.worst_ratios(got, cases.reference64(case)).items():
      worst[(c.list, key)] = max(worst.get((c.list, key), 0.0), value)
  for slot in sorted(worst):
    print(f'float32 restated, list {slot[0]}, {slot[1]}: {worst[slot]:.3g} of its bar')
  missed = {slot for slot, value in worst.items() if value > 1.0}
  assert missed <= {entry[:2] for entry in cases.EXEMPT}, {slot: worst[slot] for slot in missed}


def test_the_cases_cover_what_they_claim():
  c = cases.C
  assert len(cases.FULL) == 72 == len(set(cases.FULL))
  assert len(cases.CASES) == 72 + 6 * len(cases.COVER)
  for field, values in (('lr', cases.LRS), ('clip', cases.CLIPS), ('wd', cases.WDS), ('warmup', cases.WARMUPS),
                        ('bf16', (False, True))):
    assert {getattr(h, field) for h in cases.COVER} == set(values), field
    assert {getattr(h, field) for h in cases.FULL} == set(values), field
  assert set(cases.LISTS) == {'clip', 'one', 'two', 'sizes', 'seventy', 'wide', 'views'}
  assert set(cases.mask_of(cases.LISTS['clip'])) == {False, True} and len(cases.LISTS['clip']) == 3
  sizes = [int(np.prod(s.shape)) for s in cases.LISTS['sizes']]
  assert {1, 3, c - 1, c, c + 1, 2 * c + 5, 0} <= set(sizes)
  assert len(cases.LISTS['seventy']) == 70 and -(-int(np.prod(cases.LISTS['wide'][0].shape)) // c) == 70
  assert {s.poff for s in cases.LISTS['views']} >= {1, 2, 3}
  assert any(s.poff % 4 != s.goff % 4 for s in cases.LISTS['views'])
  # the three regimes of the clip, in `clip` at either bound and with either gradient dtype; no case of any list
  # comes closer to its bound than MARGIN, so float32 and float64 take the same branch
  for clip in (10.0, 0.5):
    for bf16 in (False, True):
      case = next(i for i, k in enumerate(cases.CASES) if k.list == 'clip' and k.hyper.clip == clip and k.hyper.bf16 == bf16)
      seen = [cases.regime(grads, clip) for grads in cases.inputs(case)['g']]
      far = {side for side, gap in seen if gap > 0.5}
      near = [gap for side, gap in seen if gap < 2 * cases.NEAR]
      assert far == {'below', 'above'} and len(near) == 1 and near[0] >= 2e-3, (clip, bf16, seen)
  for case, k in enumerate(cases.CASES):
    for step, grads in enumerate(cases.inputs(case)['g']):
      side, gap = cases.regime(grads, k.hyper.clip)
      assert gap >= cases.MARGIN, (cases.tag(case), step, side, gap)
      assert (side == 'off') == (k.hyper.clip == 0.0)
  # warm-up: the first update has step size 0 and moves no parameter, the moments move
  assert cases.schedule(1.0, 3, 0) == 0.0 and cases.schedule(1.0, 3, 3) == 1.0 and cases.schedule(1.0, 0, 0) == 1.0
  case = next(i for i, k in enumerate(cases.CASES) if k.list == 'clip' and k.hyper.warmup)
  first = cases.reference64(case)[0]
  assert all(np.array_equal(a, b.astype(np.float64)) for a, b in zip(first['p'], cases.inputs(case)['p']))
  assert all(np.abs(m).min() > 0 for m in first['mu'])
  # bfloat16 cases hold bfloat16 values; the shared inputs cannot be written
  case = next(i for i, k in enumerate(cases.CASES) if k.hyper.bf16)
  g = cases.inputs(case)['g'][0][0]
  assert np.array_equal(g, cases.bf16_round(g).reshape(g.shape)) and not g.flags.writeable


def test_the_mu_bar_sees_small_gradients():
  """`ratio_mu` is relative to the condition of the sum: an error of 1e-4 of mu
  fails it at any scale of the gradients, where `ratio`'s absolute 1e-5 passes."""
  want = np.array([1e-7, -2e-7, 3e-9])
  amu = np.abs(want)
  assert cases.ratio_mu(want * (1 + 1e-4), want, amu) > 1.0 > cases.ratio(want * (1 + 1e-4), want)
  assert cases.ratio_mu(want * (1 + 1e-6), want, amu) < 1.0
  assert cases.ratio_mu(np.zeros(3), np.zeros(3), np.zeros(3)) == 0.0


def test_refusals_before_any_launch():
  from embodied_amd import _lib, optim
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def update(table=x, chunks=x, n=3, partials=x, lr=1e-3, beta1=0.9, omb1=0.1, c1=0.1, beta2=0.999, omb2=0.001, c2=0.001,
             eps=1e-7, clip=10.0, wd=0.0):
    return raws['emb_optim_adam_update'](table, chunks, n, partials, lr, beta1, omb1, c1, beta2, omb2, c2, eps, clip, wd,
                                         None)

  before = optim.optimizer_launches()
  nan, inf = float('nan'), float('inf')
  refused = [('a pointer is null', dict(table=None)), ('a pointer is null', dict(chunks=None)),
             ('a pointer is null', dict(partials=None)), ('chunks is outside 1 ..', dict(n=0)),
             ('chunks is outside 1 ..', dict(n=-1)), ('chunks is outside 1 ..', dict(n=1 << 31)),
             ('lr must be finite', dict(lr=nan)), ('lr must be finite', dict(lr=inf)),
             ('a beta outside', dict(beta1=1.0)), ('a beta outside', dict(beta2=-0.1)), ('a beta outside', dict(beta1=nan)),
             ('a beta outside', dict(beta2=1.5)),
             ('1 - beta outside', dict(omb1=0.0)), ('1 - beta outside', dict(omb2=1.5)),
             ('a bias correction outside', dict(c1=0.0)), ('a bias correction outside', dict(c2=nan)),
             ('must be finite and not negative', dict(eps=-1.0)), ('must be finite and not negative', dict(eps=nan)),
             ('must be finite and not negative', dict(clip=-0.5)), ('must be finite and not negative', dict(clip=nan)),
             ('must be finite and not negative', dict(clip=inf)), ('must be finite and not negative', dict(wd=-0.1)),
             ('must be finite and not negative', dict(wd=nan)), ('must be finite and not negative', dict(wd=inf))]
  for message, kw in refused:
    status = update(**kw)
    assert status == _lib.ERR_INVALID, (message, kw, status)
    assert b'optim_adam_update' in _lib.lib.emb_last_error()
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  norms = raws['emb_optim_grad_norms']
  for args in ((None, x, 3, x), (x, None, 3, x), (x, x, 3, None), (x, x, 0, x), (x, x, -1, x), (x, x, 1 << 31, x)):
    assert norms(*args, None) == _lib.ERR_INVALID, args
    assert b'optim_grad_norms' in _lib.lib.emb_last_error()
  assert optim.optimizer_launches() == before


@pytest.fixture
def on_host(monkeypatch):
  """The facade over host tensors: the device check is lifted, so the composed
  path and every refusal behind it can run without a device."""
  from embodied_amd import optim
  monkeypatch.setattr(optim, '_check_param', lambda index, param: None)
  return optim


def test_facade_refuses_host_tensors_and_other_dtypes():
  import embodied_amd as emb
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Adam([torch.zeros(3)])
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Adam([torch.zeros(3, device='meta')])
  for dtype in (torch.float64, torch.bfloat16, torch.float16, torch.int32):
    with pytest.raises(TypeError, match='parameter 0 must be float32.*no CPU fallback'):
      emb.Adam([torch.zeros(3, dtype=dtype), torch.zeros(3)])
  with pytest.raises(TypeError, match='not a tensor'):
    emb.Adam([np.zeros(3, np.float32)])


def test_hyper_parameter_refusals(on_host):
  params = [torch.zeros(3), torch.zeros(2, 2)]
  nan, inf = float('nan'), float('inf')
  for kw, match in ((dict(beta1=1.0), 'Adam: beta1'), (dict(beta2=-0.1), 'beta2'), (dict(beta1=nan), 'beta1'),
                    (dict(clip=-0.5), 'Adam: clip'), (dict(clip=nan), 'clip'), (dict(clip=inf), 'clip'),
                    (dict(eps=-1e-7), 'eps'), (dict(eps=nan), 'eps'), (dict(wd=-0.1), 'wd'), (dict(wd=nan), 'wd'),
                    (dict(wd=inf), 'wd'), (dict(warmup=-1), 'warmup'), (dict(warmup=2.5), 'warmup'),
                    (dict(lr=nan), 'lr'), (dict(lr=lambda count: 1.0, warmup=3), 'callable'),
                    (dict(lr=lambda count: 1.0), 'callable'),                    # the default warmup is 1000
                    (dict(wd_mask=[True]), 'wd_mask has 1 entries for 2'), (dict(wd_mask=[True] * 3), 'wd_mask has 3')):
    with pytest.raises(ValueError, match=match):
      on_host.Adam(params, **kw)
  with pytest.raises(ValueError, match='one parameter group'):
    on_host.Adam([{'params': params[:1]}, {'params': params[1:]}])
  opt = on_host.Adam(params, fused=False)
  assert opt.wd_mask == (False, True)                    # None: dim() >= 2, the reference's /kernel$
  group = opt.param_groups[0]                            # ppo/configs.yaml:101
  assert (group['lr'], group['clip'], group['eps'], group['wd'], group['warmup']) == (3e-4, 10.0, 1e-7, 0.0, 1000)
  assert (group['beta1'], group['beta2'], group['updates']) == (0.9, 0.999, 0)
  assert sorted(opt.state[params[0]]) == ['mu', 'nu']
  params[0].grad = torch.ones(3)
  with pytest.raises(ValueError, match='Adam.step: parameter 1 has no gradient'):
    opt.step()
  assert opt.param_groups[0]['updates'] == 0 and not params[0].any()      # refused before anything moved
  params[1].grad = torch.ones(2, 2)
  params[0].grad_dtype = None
  params[0].grad = torch.ones(3, dtype=torch.float16)
  with pytest.raises(TypeError, match='gradient of parameter 0 must be float32 or bfloat16'):
    opt.step()
  with pytest.raises(RuntimeError, match='Adam.metrics: no step yet'):
    opt.metrics()
  strided = torch.zeros(4, 3).t()
  assert on_host.Adam([params[0], strided]).fused is False and on_host.Adam(params).fused is True
  with pytest.raises(ValueError, match=r'Adam\(fused=True\): parameter 1 of shape \(3, 4\) is not contiguous'):
    on_host.Adam([params[0], strided], fused=True)


def test_composed_path_is_the_restatement(on_host):
  """The composed path over host tensors equals `restate` in float32 bit for bit
  (the same torch operations in the same order), a callable lr sees the number
  of updates so far, `clip=0` switches the clip off, and `state_dict` carries
  the moments and the count."""
  picks = [0, 13, 29, 46, 71] + [i for i, c in enumerate(cases.CASES) if c.list in ('two', 'seventy')]
  assert {cases.CASES[i].hyper.clip for i in picks} == set(cases.CLIPS)
  for case in picks:
    c = cases.CASES[case]
    h, specs, inp = c.hyper, cases.LISTS[c.list], cases.inputs(case)
    want = cases.restate(inp, h, specs, torch.float32)
    params = [torch.from_numpy(x.copy()) for x in inp['p']]
    seen = []

    def lr(count, h=h, seen=seen):
      seen.append(count)
      return cases.schedule(h.lr, h.warmup, count)

    opt = on_host.Adam(params, lr=lr, clip=h.clip, wd=h.wd, warmup=0, fused=False)
    for step in range(cases.STEPS):
      for param, g in zip(params, inp['g'][step]):
        param.grad_dtype = None
        param.grad = torch.from_numpy(g.copy()).to(torch.bfloat16 if h.bf16 else torch.float32)
      opt.step()
      for i, param in enumerate(params):
        assert np.array_equal(param.numpy(), want[step]['p'][i]), (case, step, i)
        assert np.array_equal(opt.state[param]['nu'].numpy(), want[step]['nu'][i]), (case, step, i)
        assert np.array_equal(opt.state[param]['mu'].numpy(), want[step]['mu'][i]), (case, step, i)
      m = opt.metrics()
      got = np.array([float(m[key]) for key in cases.METRICS], np.float32)
      assert np.array_equal(got, want[step]['metrics']), (case, step)
      assert m['updates'] == step + 1 and m['param_count'] == sum(x.size for x in inp['p'])
      assert sorted(m) == sorted(cases.METRICS + ('updates', 'param_count'))
    assert seen == [0, 1, 2, 3]
    saved = opt.state_dict()
    assert saved['param_groups'][0]['updates'] == cases.STEPS and len(saved['state']) == len(params)
    # the float lr with warmup is the same schedule
    again = [torch.from_numpy(x.copy()) for x in inp['p']]
    other = on_host.Adam(again, lr=h.lr, clip=h.clip, wd=h.wd, warmup=h.warmup, fused=False)
    for param, g in zip(again, inp['g'][0]):
      param.grad = torch.from_numpy(g.copy())
    other.step()
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(again, want[0]['p']))


def test_laprop_keeps_its_public_surface(on_host):
  """The helpers moved into a shared base; `LaProp`'s constructor and the
  attributes its tests read did not."""
  signature = inspect.signature(on_host.LaProp.__init__)
  assert list(signature.parameters) == ['self', 'params', 'lr', 'agc', 'pmin', 'eps', 'beta1', 'beta2', 'nesterov', 'wd',
                                        'wd_mask', 'warmup', 'fused']
  defaults = {k: v.default for k, v in signature.parameters.items() if v.default is not inspect.Parameter.empty}
  assert defaults == dict(lr=4e-5, agc=0.3, pmin=1e-3, eps=1e-20, beta1=0.9, beta2=0.999, nesterov=False, wd=0.0,
                          wd_mask=None, warmup=0, fused=None)
  assert list(inspect.signature(on_host.Adam.__init__).parameters) == [
      'self', 'params', 'lr', 'clip', 'eps', 'beta1', 'beta2', 'wd', 'wd_mask', 'warmup', 'fused']
  for cls in (on_host.LaProp, on_host.Adam):
    opt = cls([torch.zeros(3), torch.zeros(2, 2)])
    assert opt._plan is None and opt.table_uploads == 0 and opt._sums is None and opt._schedule is None
    assert opt.wd_mask == (False, True) and opt.fused is True and opt.param_count == 7
    for name in ('_misfit', '_gradients', '_make_plan', '_refresh', '_hyper', 'metrics', 'step'):
      assert callable(getattr(opt, name)), name
    assert getattr(cls, '_refresh') is getattr(on_host.LaProp, '_refresh')      # one definition for both
  assert sorted(on_host.LaProp([torch.zeros(3)]).param_groups[0]) == sorted(
      ['params', 'lr', 'agc', 'pmin', 'eps', 'beta1', 'beta2', 'nesterov', 'wd', 'warmup', 'updates'])
