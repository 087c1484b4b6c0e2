"""`embodied_amd.outs.Categorical` / `policy_loss` and `emb_policy_loss*` as far as
they go without a GPU: the fixture, the restatement the GPU tests rely on, the
bars, the declarations and the binding, the path decision and what the facade
hands the launch, the refusals that happen before any launch.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import policy_loss_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'policy_loss.npz'
NAMES = ('emb_policy_loss', 'emb_policy_loss_grad', 'emb_policy_loss_launches')


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_policy_loss', ROOT / 'tools' / 'gen_policy_loss_golden.py')
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


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_forward_bar():
  """The fixture belongs to `cases.inputs`; `cases.reference64` agrees with the
  reference's own float64 run of imag_loss on every case; the reference's float32
  run sits inside the forward bar 1e-5 + 1e-5 |want|."""
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_imag_loss']) == (382, 446) and tuple(f['lines_lambda_return']) == (482, 490)
    assert tuple(f['lines_Agg']) == (40, 76) and tuple(f['lines_Categorical']) == (208, 240)
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      inp = cases.inputs(case)
      assert np.array_equal(f[f'in_{name}'], cases.digest(inp)), name
      want, got32, adv, weight = _case_arrays(f, case)
      assert want.dtype == np.float64 and got32.dtype == adv.dtype == weight.dtype == np.float32
      assert want.shape == got32.shape == (len(cases.FIELDS), cases.N, cases.T - 1) and np.isfinite(want).all(), name
      assert adv.shape == (cases.N, cases.T - 1) and weight.shape == (cases.N, cases.T)
      assert np.array_equal(adv, f[f'adv64_{name}']) and np.array_equal(weight, f[f'weight64_{name}'])
      ref = cases.reference64(inp['logits'], inp['act'], adv, weight, cases.ACTENT, c.unimix, 1 if c.groups else 0, 1)
      mine = np.stack([ref[key] for key in cases.FIELDS])
      assert np.allclose(mine, want, rtol=1e-12, atol=1e-12), name
      # the (N, T - 1) layout of weight is the same thing
      cut = cases.reference64(inp['logits'], inp['act'], adv, weight[:, :-1], cases.ACTENT, c.unimix,
                              1 if c.groups else 0, 1)
      assert np.array_equal(cut['loss'], ref['loss'])
      # the out-of-range actions of the first row add exactly nothing
      if not c.groups:
        assert want[0, 0, 2] == 0.0 and want[0, 0, 3] == 0.0 and want[0, 0, 0] != 0.0
      worst = max(worst, cases.forward_ratio(got32, want))
    assert any((f[f'weight_{cases.tag(i)}'] == 0).any() for i in range(len(cases.CASES)))
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0
  assert GOLDEN.stat().st_size < 900_000


def test_float32_definition_against_both_bars():
  """The restated arithmetic in float32 on the CPU over every case of the fixture,
  float32 and bfloat16-rounded logits: its worst forward and gradient ratios
  against float64, printed per (unimix, scale).  A family that misses the
  gradient bar must be listed in `cases.GRAD_EXEMPT`; nothing else may miss."""
  rng = np.random.default_rng(11)
  forward, gradient = {}, {}
  with np.load(GOLDEN) as f:
    for case, c in enumerate(cases.CASES):
      _, _, adv, weight = _case_arrays(f, case)
      inp = cases.inputs(case)
      gout = rng.standard_normal(adv.shape).astype(np.float32)
      for rounded in (False, True):
        logits = cases.bf16_round(inp['logits']) if rounded else inp['logits']
        args = (logits, inp['act'], adv, weight, cases.ACTENT, c.unimix, 1 if c.groups else 0, 1, gout)
        want, got = cases.reference64(*args), cases.restate(*args, dtype=torch.float32)
        key = (c.unimix, c.scale)
        ratio = max(cases.forward_ratio(got[k], want[k]) for k in cases.FIELDS)
        forward[key] = max(forward.get(key, 0.0), ratio)
        assert not want['grad'][:, -1].any() and not got['grad'][:, -1].any()       # the dropped step
        assert np.isfinite(got['grad']).all()
        s = cases.row_scale(gout, weight[:, :-1], adv, cases.ACTENT)
        ratio = cases.grad_ratio(got['grad'][:, :-1], want['grad'][:, :-1], s)
        gradient[key] = max(gradient.get(key, 0.0), ratio)
  for key in sorted(forward):
    print(f'float32 definition, unimix {key[0]:g} scale {key[1]:g}: forward {forward[key]:.3g}, '
          f'gradient {gradient[key]:.3g} of their bars')
  assert max(forward.values()) <= 1.0, forward
  missed = {key: ratio for key, ratio in gradient.items() if ratio > 1.0}
  assert set(missed) <= set(cases.GRAD_EXEMPT), missed


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/agent.py:411-415' in text and 'embodied/jax/outs.py:208-234' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [17, 16, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'policy_loss.hip' in sources and 'policy_loss_abi.cpp' in sources
  kernels_abi = (ROOT / 'embodied_amd' / 'csrc' / 'kernels_abi.cpp').read_text()
  assert 'policy_loss' not in kernels_abi                  # that file is linked into the host sanitizer soak
  assert emb.Categorical is emb.outs.Categorical and emb.policy_loss is emb.outs.policy_loss
  assert emb.policy_loss_launches() == emb.outs.policy_loss_launches()
  # both kernels' translation units take the one-operand pieces from one header
  csrc = ROOT / 'embodied_amd' / 'csrc'
  for unit in ('onehot_kl.hip', 'policy_loss.hip'):
    body = (csrc / unit).read_text()
    assert '#include "onehot_segment.h"' in body and 'struct Side' not in body, unit
  assert 'struct Side' in (csrc / 'onehot_segment.h').read_text()


def test_refusals_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import outs
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def forward(logits=x, act=x, dtype=_lib.F32, n=2, t=3, drop=1, groups=2, classes=8, unimix=0.01, actent=3e-4, adv=x,
              weight=x, stride=3, loss=x, logpi=x, ent=x):
    return raws['emb_policy_loss'](logits, act, dtype, n, t, drop, groups, classes, unimix, actent, adv, weight,
                                   stride, loss, logpi, ent, None)

  def grad(logits=x, act=x, dtype=_lib.BF16, n=2, t=3, drop=1, groups=2, classes=8, unimix=0.01, actent=3e-4, adv=x,
           weight=x, stride=3, gout=x, grad=x):
    return raws['emb_policy_loss_grad'](logits, act, dtype, n, t, drop, groups, classes, unimix, actent, adv, weight,
                                        stride, gout, grad, None)

  before = outs.policy_loss_launches()
  shape = [('negative N or T', dict(n=-1)), ('negative N or T', dict(t=-1)), ('drop must be', dict(drop=2)),
           ('drop must be', dict(drop=-1)), ('groups must be', dict(groups=0)),
           ('classes outside 1 .. 256', dict(classes=0)), ('classes outside 1 .. 256', dict(classes=257)),
           ('more than 2^31 - 1', dict(n=(1 << 31) // 64, t=4, stride=4)),
           ('more than 2^31 - 1', dict(n=1 << 62, t=1 << 20, groups=1 << 20, classes=256)),
           ('more than 2^31 - 1', dict(n=1, t=1, groups=1 << 31, classes=2)),
           ('dtype must be', dict(dtype=_lib.F16)), ('dtype must be', dict(dtype=_lib.F64)),
           ('unimix outside', dict(unimix=-0.1)), ('unimix outside', dict(unimix=1.0)),
           ('unimix outside', dict(unimix=float('nan'))), ('actent must be finite', dict(actent=float('nan'))),
           ('actent must be finite', dict(actent=float('inf'))), ('weight_stride below', dict(stride=1))]
  refused = []
  for call in (forward, grad):
    refused += [(call, message, kw) for message, kw in shape]
    refused += [(call, 'a pointer is null', dict(logits=None))]
  refused += [(forward, 'a pointer is null', dict(logpi=None)), (forward, 'a pointer is null', dict(ent=None)),
              (grad, 'a pointer is null', dict(grad=None)), (grad, 'gout is null', dict(gout=None))]
  for call, message, kw in refused:
    status = call(**kw)
    assert status == _lib.ERR_INVALID, (call.__name__, message, kw, status)
    assert message.encode() in _lib.lib.emb_last_error(), (call.__name__, message, _lib.lib.emb_last_error())
  # the largest product that is taken passes the size check (and is refused for its null pointer)
  assert forward(n=(1 << 31) // 64 - 1, t=4, stride=4, logits=None) == _lib.ERR_INVALID
  assert b'a pointer is null' in _lib.lib.emb_last_error()
  # no output rows: nothing to do, nothing launched, whatever the device pointers are
  assert forward(n=0) == _lib.OK and forward(n=0, logits=None, logpi=None) == _lib.OK
  assert forward(t=1, drop=1) == _lib.OK and forward(t=0, drop=0, logits=None) == _lib.OK
  assert grad(n=0) == _lib.OK and grad(n=0, logits=None, grad=None) == _lib.OK and grad(t=0, grad=None) == _lib.OK
  assert outs.policy_loss_launches() == before
  assert raws['emb_policy_loss_launches'](None) == _lib.ERR_INVALID
  with pytest.raises(ValueError, match='negative N or T'):     # the same through the binding that raises
    _lib.api.emb_policy_loss(x, x, _lib.F32, -1, 3, 1, 2, 8, 0.01, 3e-4, x, x, 3, x, x, x, None)


def test_facade_refuses_host_tensors():
  import embodied_amd as emb
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Categorical(torch.zeros(3, 4, 8))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.policy_loss(torch.zeros(3, 4, 8), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 4))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Categorical(torch.empty(3, 4, 8, device='meta'))


def test_path_decision():
  from embodied_amd import outs
  assert outs.POLICY_MAX_CLASSES == 256
  for classes in (1, 2, 18, 64, 96, 256):
    assert outs._policy_path(None, 16384 * 16, 1, classes) is True and outs._policy_path(True, 5, 1, classes) is True
    assert outs._policy_path(False, 5, 1, classes) is False
  assert outs._policy_path(None, 5, 2, 257) is False and outs._policy_path(False, 5, 2, 257) is False
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    outs._policy_path(True, 5, 2, 257)
  assert outs._policy_path(None, (1 << 31) // 2048, 32, 64) is False
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    outs._policy_path(True, (1 << 31) // 2048, 32, 64)


@pytest.fixture
def recorded(monkeypatch):
  """The facade on host tensors with both launches replaced by recorders: what
  it decides and what it hands the kernels, without a device."""
  from embodied_amd import _lib
  from embodied_amd import outs
  calls = []
  monkeypatch.setattr(outs, '_check_device', lambda logits: None)
  monkeypatch.setattr(_lib, 'raw_stream', lambda device: None)
  monkeypatch.setattr(outs.api, 'emb_policy_loss', lambda *a: calls.append(('forward', a)), raising=False)
  monkeypatch.setattr(outs.api, 'emb_policy_loss_grad', lambda *a: calls.append(('grad', a)), raising=False)
  return calls


def test_what_the_facade_hands_the_launch(recorded):
  from embodied_amd import _lib
  from embodied_amd import outs
  logits = torch.zeros(2, 3, 5, 4, 8, requires_grad=True)                 # (N.., T, groups, classes)
  act = torch.zeros(2, 3, 5, 4, dtype=torch.int64)
  adv, weight = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
  out = outs.policy_loss(logits, act, adv, weight, actent=0.5, unimix=0.01, dims=1, fused=True)
  assert [kind for kind, _ in recorded] == ['forward']
  a = recorded[0][1]
  assert a[2:10] == (_lib.F32, 6, 5, 1, 4, 8, 0.01, 0.5) and a[12] == 5 and len(a) == 17
  assert all(out[key].shape == (2, 3, 4) for key in ('loss', 'logpi', 'ent'))
  assert out['loss'].requires_grad and not out['logpi'].requires_grad and not out['ent'].requires_grad
  out['loss'].sum().backward()
  assert [kind for kind, _ in recorded] == ['forward', 'grad']
  g = recorded[1][1]
  assert g[2:10] == a[2:10] and g[12] == 5 and len(g) == 16 and logits.grad.shape == logits.shape
  # weight as (N.., T - 1): its own row stride; no time axis dropped: every row, T = 1
  recorded.clear()
  outs.policy_loss(logits, act, adv, weight[..., :-1], dims=1, fused=None)
  assert recorded[0][1][12] == 4 and recorded[0][1][9] == pytest.approx(3e-4)
  outs.policy_loss(logits.detach()[..., 0, :], act[..., 0], weight, weight, dims=0, drop_last=False, fused=True)
  assert recorded[1][1][3:8] == (30, 1, 0, 1, 8) and recorded[1][1][12] == 1
  # no output rows: nothing is launched, the composed path answers
  recorded.clear()
  single = torch.zeros(4, 1, 8, requires_grad=True)
  out = outs.policy_loss(single, torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, 0), torch.zeros(4, 1), fused=True)
  out['loss'].sum().backward()
  assert out['loss'].shape == (4, 0) and not single.grad.any() and single.grad.shape == (4, 1, 8)
  empty = outs.policy_loss(torch.zeros(0, 3, 8), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 2),
                           torch.zeros(0, 3))
  assert empty['loss'].shape == (0, 2) and not recorded
  # Categorical: logp is the launch with actent 0, entropy the one with no action and actent -1
  dist = outs.Categorical(logits, unimix=0.01, dims=1, fused=True)
  assert dist.fused is True and dist.minent == 0 and dist.maxent == pytest.approx(np.log(8) * 4)
  dist.logp(act)
  dist.entropy()
  (_, lp), (_, en) = recorded
  assert lp[3:8] == (30, 1, 0, 4, 8) and lp[1] is not None and lp[9] == 0.0 and lp[10] is None and lp[11] is None
  assert en[3:8] == (30, 1, 0, 4, 8) and en[1] is None and en[9] == -1.0
  assert outs.Categorical(logits, dims=1).pred().shape == (2, 3, 5, 4)
  # where the kernels do not fit
  wide = torch.zeros(3, 2, 257)
  assert outs.Categorical(wide).fused is False and outs.Categorical(wide, dims=1).maxent == pytest.approx(np.log(257) * 2)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    outs.Categorical(wide, fused=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes'):
    outs.policy_loss(wide, torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 1), torch.zeros(3, 2), fused=True)


def test_facade_refusals(recorded):
  from embodied_amd import outs
  x = torch.zeros(3, 4, 8)
  act, adv, weight = torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 4)
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    outs.Categorical(x.double())
  with pytest.raises(ValueError, match='dims'):
    outs.Categorical(x, dims=2)
  with pytest.raises(ValueError, match='unimix'):
    outs.Categorical(x, unimix=1.0)
  with pytest.raises(ValueError, match='groups, classes'):
    outs.Categorical(x[0, 0], dims=1)
  with pytest.raises(TypeError, match='must be integers'):
    outs.Categorical(x).logp(torch.zeros(3, 4))
  with pytest.raises(ValueError, match=r'actions of shape \(3, 3\)'):
    outs.policy_loss(x, act[:, :3], adv, weight)
  with pytest.raises(ValueError, match=r'adv of shape \(3, 4\)'):
    outs.policy_loss(x, act, weight, weight)
  with pytest.raises(ValueError, match=r'weight of shape \(3, 2\)'):
    outs.policy_loss(x, act, adv, weight[:, :2])
  with pytest.raises(ValueError, match='actent'):
    outs.policy_loss(x, act, adv, weight, actent=float('nan'))
  with pytest.raises(ValueError, match='time axis'):
    outs.policy_loss(x[0, 0], act[0, 0], adv[0, 0], weight[0, 0])
  assert not recorded
