"""`embodied_amd.outs.Normal` / `normal_policy_loss` and `emb_normal_*` as far as
they go without a GPU: the fixture, the restatement the GPU tests rely on, the
bars, the declarations and the binding, the path decision and what the facade
hands the launch, the refusals that happen before any launch.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import normal_policy_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'normal_policy.npz'
NAMES = ('emb_normal_policy_loss', 'emb_normal_policy_loss_grad', 'emb_normal_sample', 'emb_philox_normal',
         'emb_normal_policy_launches')


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_normal_policy', ROOT / 'tools' / 'gen_normal_policy_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key], equal_nan=f[key].dtype.kind == 'f'), key


def _case_arrays(f, case):
  name = cases.tag(case)
  return f[f'out64_{name}'], f[f'out_{name}'], f[f'adv_{name}'], f[f'weight_{name}']


def _args(inp, c, adv, weight, gout=None):
  return (inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, cases.ACTENT, c.kind, 1 if c.actions else 0, 1, gout)


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_forward_bar():
  """The fixture belongs to `cases.inputs`; `cases.reference64` agrees with the
  reference's own float64 run of imag_loss on every case; the reference's float32
  run sits inside the forward bar 1e-5 (1 + S)."""
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_imag_loss']) == (382, 446) and tuple(f['lines_lambda_return']) == (482, 490)
    assert tuple(f['lines_Agg']) == (40, 76) and tuple(f['lines_Normal']) == (161, 186)
    assert tuple(f['lines_bounded_normal']) == (146, 155) and tuple(f['lines_normal_logstd']) == (157, 162)
    assert len(cases.CASES) == 97 and sum(c.actions == 0 for c in cases.CASES) == 1
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      inp = cases.inputs(case)
      assert np.array_equal(f[f'in_{name}'], cases.digest(inp)), name
      assert np.abs(inp['act'].reshape(cases.N * cases.T, -1)[::7]).max() <= 1.0
      want, got32, adv, weight = _case_arrays(f, case)
      assert want.dtype == np.float64 and got32.dtype == adv.dtype == weight.dtype == np.float32
      assert want.shape == got32.shape == (len(cases.FIELDS), cases.N, cases.T - 1) and np.isfinite(want).all(), name
      assert np.array_equal(adv, f[f'adv64_{name}']) and np.array_equal(weight, f[f'weight64_{name}'])
      ref = cases.reference64(*_args(inp, c, adv, weight))
      mine = np.stack([ref[key] for key in cases.FIELDS])
      scale = 1 + np.abs(want)
      assert np.all(np.abs(mine - want) <= 1e-12 * np.maximum(scale, 1 + ref['S'])), name
      cut = cases.reference64(*_args(inp, c, adv, weight[:, :-1]))          # the (N, T - 1) layout of weight
      assert np.array_equal(cut['loss'], ref['loss'])
      got = dict(zip(cases.FIELDS, got32))
      worst = max(worst, cases.forward_ratios(got, ref, adv, weight[:, :-1], cases.ACTENT))
    assert any((f[f'weight_{cases.tag(i)}'] == 0).any() for i in range(len(cases.CASES)))
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0
  assert GOLDEN.stat().st_size < 900_000


def test_float32_definition_against_both_bars():
  """The restated arithmetic in float32 on the CPU over every case of the fixture,
  float32 and bfloat16-rounded inputs: its worst forward and gradient ratios
  against float64, printed per head.  No case is exempt from either bar."""
  rng = np.random.default_rng(11)
  forward, gradient = {}, {}
  with np.load(GOLDEN) as f:
    for case, c in enumerate(cases.CASES):
      _, _, adv, weight = _case_arrays(f, case)
      inp = cases.inputs(case)
      gout = rng.standard_normal(adv.shape).astype(np.float32)
      for rounded in (False, True):
        run = dict(inp)
        if rounded:
          run.update(mean_raw=cases.bf16_round(inp['mean_raw']), std_raw=cases.bf16_round(inp['std_raw']))
        args = _args(run, c, adv, weight, gout)
        want, got = cases.reference64(*args), cases.restate(*args, dtype=torch.float32)
        key = (c.kind, c.scale)
        forward[key] = max(forward.get(key, 0.0), cases.forward_ratios(got, want, adv, weight[:, :-1], cases.ACTENT))
        s = cases.row_scale(gout, weight[:, :-1], adv, cases.ACTENT)
        for name in ('grad_mean', 'grad_std'):
          assert not want[name][:, -1].any() and not got[name][:, -1].any()       # the dropped step
          ratio = cases.grad_ratio(got[name][:, :-1], want[name][:, :-1], s)
          gradient[key] = max(gradient.get(key, 0.0), ratio)
  for key in sorted(forward):
    print(f'float32 definition, {key[0]} scale {key[1]:g}: forward {forward[key]:.3g}, '
          f'gradient {gradient[key]:.3g} of their bars')
  assert max(forward.values()) <= 1.0, forward
  assert max(gradient.values()) <= 1.0, gradient


def test_draw_definition():
  """The numpy Box-Muller the GPU test holds `philox_normal` to: word 0 is the
  word of the uniform stream, u1 never 0, the moments of a standard normal."""
  from tests import onehot_sample_cases as uniform
  words = cases.philox_words(7, 3, 5, 64)
  u = (words[0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
  assert np.array_equal(u, uniform.uniforms(7, 3, 5, 64))
  eps = cases.box_muller64(1234, 5, 0, 1 << 16)
  assert np.isfinite(eps).all() and abs(eps.mean()) < 0.02 and abs(eps.var() - 1) < 0.03
  assert not np.array_equal(eps[:64], cases.box_muller64(1234, 6, 0, 64))


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  for cited in ('dreamerv3/agent.py:411-415', 'embodied/jax/heads.py:146-162', 'embodied/jax/outs.py:40-76'):
    assert cited in text, cited
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [19, 19, 13, 6, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'normal_policy.hip' in sources and 'normal_policy_abi.cpp' in sources
  kernels_abi = (ROOT / 'embodied_amd' / 'csrc' / 'kernels_abi.cpp').read_text()
  assert 'normal_policy' not in kernels_abi                # that file is linked into the host sanitizer soak
  assert emb.Normal is emb.outs.Normal and emb.normal_policy_loss is emb.outs.normal_policy_loss
  assert emb.philox_normal is emb.outs.philox_normal
  assert emb.normal_policy_launches() == emb.outs.normal_policy_launches()
  # the segment butterflies and the Philox rounds are included, not copied
  csrc = ROOT / 'embodied_amd' / 'csrc'
  body = (csrc / 'normal_policy.hip').read_text()
  assert '#include "onehot_segment.h"' in body and '#include "philox.h"' in body
  assert '__shfl_xor' not in body and '0xD2511F53' not in body
  sample = (csrc / 'onehot_sample.hip').read_text()
  assert '#include "philox.h"' in sample and '0xD2511F53' not in sample
  assert 'kNormalMaxBlocks = 2048' in (csrc / 'normal_policy.h').read_text()


def test_refusals_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import outs
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def forward(mean=x, std=x, act=x, dtype=_lib.F32, n=2, t=3, drop=1, a=6, kind=0, lo=0.1, hi=1.0, actent=3e-4, adv=x,
              weight=x, stride=3, loss=x, logpi=x, ent=x):
    return raws['emb_normal_policy_loss'](mean, std, act, dtype, n, t, drop, a, kind, lo, hi, actent, adv, weight,
                                          stride, loss, logpi, ent, None)

  def grad(mean=x, std=x, act=x, dtype=_lib.BF16, n=2, t=3, drop=1, a=6, kind=0, lo=0.1, hi=1.0, actent=3e-4, adv=x,
           weight=x, stride=3, gout=x, grad_mean=x, grad_std=x):
    return raws['emb_normal_policy_loss_grad'](mean, std, act, dtype, n, t, drop, a, kind, lo, hi, actent, adv,
                                               weight, stride, gout, grad_mean, grad_std, None)

  def sample(mean=x, std=x, dtype=_lib.F32, rows=4, a=6, kind=0, lo=0.1, hi=1.0, eps=x, act=x):
    return raws['emb_normal_sample'](mean, std, dtype, rows, a, kind, lo, hi, 1, 0, eps, act, None)

  before = outs.normal_policy_launches()
  head = [('dtype must be', dict(dtype=_lib.F16)), ('dtype must be', dict(dtype=_lib.F64)),
          ('kind must be', dict(kind=2)), ('kind must be', dict(kind=-1)),
          ('hi >= lo > 0', dict(lo=0.0)), ('hi >= lo > 0', dict(lo=-0.1)), ('hi >= lo > 0', dict(lo=2.0)),
          ('hi >= lo > 0', dict(lo=float('nan'))), ('hi >= lo > 0', dict(hi=float('inf'))),
          ('hi >= lo > 0', dict(hi=float('nan')))]
  shape = [('negative N or T', dict(n=-1)), ('negative N or T', dict(t=-1)), ('drop must be', dict(drop=2)),
           ('drop must be', dict(drop=-1)), ('A outside 1 .. 256', dict(a=0)), ('A outside 1 .. 256', dict(a=257)),
           ('A outside 1 .. 256', dict(a=-3)), ('more than 2^31 - 1', dict(n=(1 << 31) // 64, t=4, a=16, stride=4)),
           ('more than 2^31 - 1', dict(n=1 << 62, t=1 << 20, a=256)),
           ('actent must be finite', dict(actent=float('nan'))), ('actent must be finite', dict(actent=float('inf'))),
           ('weight_stride below', dict(stride=1))]
  refused = []
  for call in (forward, grad):
    refused += [(call, message, kw) for message, kw in head + shape]
    refused += [(call, 'a pointer is null', dict(mean=None)), (call, 'a pointer is null', dict(std=None))]
  refused += [(forward, 'are all null', dict(loss=None, logpi=None, ent=None)),
              (grad, 'a pointer is null', dict(grad_mean=None)), (grad, 'a pointer is null', dict(grad_std=None)),
              (grad, 'gout is null', dict(gout=None))]
  refused += [(sample, message, kw) for message, kw in head]
  refused += [(sample, 'negative rows', dict(rows=-1)), (sample, 'A must be at least 1', dict(a=0)),
              (sample, 'more than 2^31 - 1', dict(rows=1 << 31, a=1)), (sample, 'a pointer is null', dict(mean=None)),
              (sample, 'a pointer is null', dict(std=None)), (sample, 'a pointer is null', dict(act=None))]
  for call, message, kw in refused:
    status = call(**kw)
    assert status == _lib.ERR_INVALID, (call.__name__, message, kw, status)
    assert message.encode() in _lib.lib.emb_last_error(), (call.__name__, message, _lib.lib.emb_last_error())
  # logstd takes no bounds; the largest product that is taken passes the size check (refused for its null pointer)
  assert forward(kind=1, lo=0.0, hi=0.0, mean=None) == _lib.ERR_INVALID
  assert b'a pointer is null' in _lib.lib.emb_last_error()
  assert forward(n=(1 << 31) // 64 - 1, t=4, a=16, stride=4, mean=None) == _lib.ERR_INVALID
  assert b'a pointer is null' in _lib.lib.emb_last_error()
  # no output rows: nothing to do, nothing launched, whatever the device pointers are
  assert forward(n=0) == _lib.OK and forward(n=0, mean=None, logpi=None) == _lib.OK
  assert forward(t=1, drop=1) == _lib.OK and forward(t=0, drop=0, mean=None) == _lib.OK
  assert grad(n=0) == _lib.OK and grad(n=0, mean=None, grad_mean=None) == _lib.OK and grad(t=0, grad_std=None) == _lib.OK
  assert sample(rows=0, mean=None, act=None) == _lib.OK
  philox = raws['emb_philox_normal']
  assert philox(1, 0, 0, 0, None, None) == _lib.OK
  assert philox(1, 0, 0, -1, x, None) == _lib.ERR_INVALID and b'negative count' in _lib.lib.emb_last_error()
  assert philox(1, 0, 0, 4, None, None) == _lib.ERR_INVALID and b'out is null' in _lib.lib.emb_last_error()
  assert outs.normal_policy_launches() == before
  assert raws['emb_normal_policy_launches'](None) == _lib.ERR_INVALID
  with pytest.raises(ValueError, match='negative N or T'):     # the same through the binding that raises
    _lib.api.emb_normal_policy_loss(x, x, x, _lib.F32, -1, 3, 1, 6, 0, 0.1, 1.0, 3e-4, x, x, 3, x, x, x, None)


def test_facade_refuses_host_tensors():
  import embodied_amd as emb
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Normal(torch.zeros(3, 4, 6), torch.zeros(3, 4, 6))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.normal_policy_loss(torch.zeros(3, 4, 6), torch.zeros(3, 4, 6), torch.zeros(3, 4, 6), torch.zeros(3, 3),
                           torch.zeros(3, 4))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Normal(torch.empty(3, 4, 6, device='meta'), torch.empty(3, 4, 6, device='meta'))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.philox_normal(1, device='cpu')


def test_path_decision():
  from embodied_amd import outs
  assert outs.NORMAL_MAX_ACTIONS == 256
  for actions in (1, 2, 6, 64, 65, 96, 256):
    assert outs._normal_path(None, 16384 * 16, actions) is True and outs._normal_path(True, 5, actions) is True
    assert outs._normal_path(False, 5, actions) is False
  assert outs._normal_path(None, 5, 257) is False and outs._normal_path(False, 5, 257) is False
  with pytest.raises(ValueError, match=r'fused=True.*257 action dimensions.*at most 256'):
    outs._normal_path(True, 5, 257)
  assert outs._normal_path(None, (1 << 31) // 64, 64) is False
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    outs._normal_path(True, (1 << 31) // 64, 64)


@pytest.fixture
def recorded(monkeypatch):
  """The facade on host tensors with the launches replaced by recorders: what
  it decides and what it hands the kernels, without a device."""
  from embodied_amd import _lib
  from embodied_amd import outs
  calls = []
  monkeypatch.setattr(outs, '_check_device', lambda tensor: None)
  monkeypatch.setattr(_lib, 'raw_stream', lambda device: None)
  for kind, name in (('forward', 'emb_normal_policy_loss'), ('grad', 'emb_normal_policy_loss_grad'),
                     ('sample', 'emb_normal_sample')):
    monkeypatch.setattr(outs.api, name, lambda *a, kind=kind: calls.append((kind, a)), raising=False)
  return calls


def test_what_the_facade_hands_the_launch(recorded):
  from embodied_amd import _lib
  from embodied_amd import outs
  mean = torch.zeros(2, 3, 5, 6, requires_grad=True)                      # (N.., T, actions)
  std = torch.zeros(2, 3, 5, 6, requires_grad=True)
  act = torch.zeros(2, 3, 5, 6, dtype=torch.float64)
  adv, weight = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
  out = outs.normal_policy_loss(mean, std, act, adv, weight, actent=0.5, fused=True)
  assert [kind for kind, _ in recorded] == ['forward']
  a = recorded[0][1]
  assert a[3:8] == (_lib.F32, 6, 5, 1, 6) and a[8] == _lib.NORMAL_BOUNDED and a[11] == 0.5 and a[14] == 5 and len(a) == 19
  assert a[9:11] == (float(np.float32(0.1)), 1.0)
  assert all(out[key].shape == (2, 3, 4) for key in ('loss', 'logpi', 'ent'))
  assert out['loss'].requires_grad and not out['logpi'].requires_grad and not out['ent'].requires_grad
  out['loss'].sum().backward()
  assert [kind for kind, _ in recorded] == ['forward', 'grad']
  g = recorded[1][1]
  assert g[3:12] == a[3:12] and g[14] == 5 and len(g) == 19
  assert mean.grad.shape == mean.shape and std.grad.shape == std.shape
  # weight as (N.., T - 1): its own row stride; no time axis dropped: every row, T = 1; dims = 0: one action
  recorded.clear()
  outs.normal_policy_loss(mean, std, act, adv, weight[..., :-1], kind='logstd', fused=None)
  assert recorded[0][1][14] == 4 and recorded[0][1][8] == _lib.NORMAL_LOGSTD
  assert recorded[0][1][11] == pytest.approx(3e-4)
  outs.normal_policy_loss(mean.detach()[..., 0], std.detach()[..., 0], act[..., 0], weight, weight, dims=0,
                          drop_last=False, fused=True)
  assert recorded[1][1][4:8] == (30, 1, 0, 1) and recorded[1][1][14] == 1
  # no output rows: nothing is launched, the composed path answers
  recorded.clear()
  single = torch.zeros(4, 1, 6, requires_grad=True)
  out = outs.normal_policy_loss(single, single.detach(), torch.zeros(4, 1, 6), torch.zeros(4, 0), torch.zeros(4, 1),
                                fused=True)
  out['loss'].sum().backward()
  assert out['loss'].shape == (4, 0) and not single.grad.any() and single.grad.shape == (4, 1, 6)
  empty = outs.normal_policy_loss(torch.zeros(0, 3, 6), torch.zeros(0, 3, 6), torch.zeros(0, 3, 6), torch.zeros(0, 2),
                                  torch.zeros(0, 3))
  assert empty['loss'].shape == (0, 2) and not recorded
  # Normal: logp is the launch with actent 0, entropy the one with no action and actent -1
  dist = outs.Normal(mean, std, 'bounded', 0.1, 1.0, fused=True)
  entropy = lambda s: (0.5 * np.log(2 * np.pi * s * s) + 0.5) * 6
  assert dist.fused is True and dist.minent == pytest.approx(entropy(0.1)) and dist.maxent == pytest.approx(entropy(1.0))
  dist.logp(act)
  dist.entropy()
  dist.sample(seed=3, offset=9)
  (_, lp), (_, en), (_, sm) = recorded
  assert lp[4:8] == (30, 1, 0, 6) and lp[2] is not None and lp[11] == 0.0 and lp[12] is None and lp[13] is None
  assert en[4:8] == (30, 1, 0, 6) and en[2] is None and en[11] == -1.0
  assert sm[3:5] == (30, 6) and sm[8:11] == (3, 9, None) and len(sm) == 13
  assert outs.Normal(mean, std).pred().shape == (2, 3, 5, 6) and not outs.Normal(mean, std).pred().requires_grad
  assert outs.Normal(mean, std, 'logstd').minent is None
  # where the kernels do not fit
  wide = torch.zeros(3, 2, 257)
  assert outs.Normal(wide, wide).fused is False
  with pytest.raises(ValueError, match=r'fused=True.*257 action dimensions.*at most 256'):
    outs.Normal(wide, wide, fused=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 action dimensions'):
    outs.normal_policy_loss(wide, wide, wide, torch.zeros(3, 1), torch.zeros(3, 2), fused=True)


def test_facade_refusals(recorded):
  from embodied_amd import outs
  x = torch.zeros(3, 4, 6)
  adv, weight = torch.zeros(3, 3), torch.zeros(3, 4)
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    outs.Normal(x.double(), x.double())
  with pytest.raises(TypeError, match='std_raw'):
    outs.Normal(x, x.bfloat16())
  with pytest.raises(ValueError, match='std_raw of'):
    outs.Normal(x, x[:, :3])
  with pytest.raises(ValueError, match='dims'):
    outs.Normal(x, x, dims=2)
  with pytest.raises(ValueError, match='kind'):
    outs.Normal(x, x, kind='tanh')
  with pytest.raises(ValueError, match='minstd'):
    outs.Normal(x, x, minstd=0.0)
  with pytest.raises(ValueError, match='minstd'):
    outs.Normal(x, x, minstd=2.0, maxstd=1.0)
  with pytest.raises(TypeError, match='must be floating point'):
    outs.Normal(x, x).logp(torch.zeros(3, 4, 6, dtype=torch.int32))
  with pytest.raises(TypeError, match='must be floating point'):
    outs.normal_policy_loss(x, x, torch.zeros(3, 4, 6, dtype=torch.int64), adv, weight)
  with pytest.raises(ValueError, match=r'actions of shape \(3, 3, 6\)'):
    outs.normal_policy_loss(x, x, x[:, :3], adv, weight)
  with pytest.raises(ValueError, match=r'adv of shape \(3, 4\)'):
    outs.normal_policy_loss(x, x, x, weight, weight)
  with pytest.raises(ValueError, match=r'weight of shape \(3, 2\)'):
    outs.normal_policy_loss(x, x, x, adv, weight[:, :2])
  with pytest.raises(ValueError, match='actent'):
    outs.normal_policy_loss(x, x, x, adv, weight, actent=float('nan'))
  with pytest.raises(ValueError, match='time axis'):
    outs.normal_policy_loss(x[0, 0, 0], x[0, 0, 0], x[0, 0, 0], adv[0, 0], weight[0, 0], dims=0)
  with pytest.raises(TypeError, match='eps must be'):
    outs.Normal(x, x).sample(eps=torch.zeros(3, 4, 6, dtype=torch.float64))
  with pytest.raises(ValueError, match='eps of shape'):
    outs.Normal(x, x).sample(eps=torch.zeros(3, 4))
  with pytest.raises(TypeError, match='seed must be an integer'):
    outs.Normal(x, x).sample()
  assert not recorded
