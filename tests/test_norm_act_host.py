"""`embodied_amd.nets.norm_act` / `NormAct` and `emb_norm_act*` as far as they go
without a GPU: the fixture, the restatement the GPU tests rely on, the bars, the
declarations and the binding, the refusals that happen before any launch.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from embodied_amd import nets

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _central(f, x, gout, step=1e-6):
  """d sum(f(x) * gout) / dx by central differences in float64."""
  grad = np.zeros_like(x)
  flat, out = x.reshape(-1), grad.reshape(-1)
  for i in range(flat.size):
    keep = flat[i]
    flat[i] = keep + step
    hi = (f(x) * gout).sum()
    flat[i] = keep - step
    lo = (f(x) * gout).sum()
    flat[i] = keep
    out[i] = (hi - lo) / (2 * step)
  return grad


def _fresh():
  """Where the reference tree exists: the fixtures regenerated in memory."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'rssm.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_rssm_core', ROOT / 'tools' / 'gen_rssm_core_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  return tool

from tests import norm_act_cases as norms

GOLDEN = ROOT / 'tests' / 'golden' / 'norm_act.npz'
NAMES = ('emb_norm_act', 'emb_norm_act_grad', 'emb_norm_act_launches')


def test_fixture_is_current():
  fresh = _fresh().generate_norm()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_forward_bar():
  """The fixture belongs to `cases.inputs`; `reference64` agrees with the
  reference's own float64 run of Norm.__call__ and act on every case; its
  float32 run sits inside the forward bar."""
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_Norm']) == (361, 409) and tuple(f['lines_act']) == (26, 39)
    for case, c in enumerate(norms.CASES):
      name, inp = norms.tag(case), norms.inputs(case)
      assert np.array_equal(f[f'in_{name}'], norms.digest(norms.present(inp))), name
      want, got32 = f[f'out64_{name}'], f[f'out_{name}']
      assert want.dtype == np.float64 and got32.dtype == np.float32 and np.isfinite(want).all()
      mine = norms.reference64(inp['x'], inp['scale'], inp['shift'], c.impl, c.act, c.eps)['out']
      assert np.allclose(mine, want, rtol=1e-12, atol=1e-12), name
      worst = max(worst, norms.out_ratio(got32, want))
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0
  assert GOLDEN.stat().st_size < 900_000
  assert {c.impl for c in norms.CASES} == set(norms.IMPLS) and {c.act for c in norms.CASES} == set(norms.ACTS)
  assert {c.eps for c in norms.CASES} == set(norms.EPS) and {c.affine for c in norms.CASES} == {True, False}

@pytest.mark.parametrize('impl', norms.IMPLS)
@pytest.mark.parametrize('act', norms.ACTS)
def test_norm_act_gradients_agree_with_central_differences(impl, act):
  rng = np.random.default_rng([norms.IMPLS.index(impl), norms.ACTS.index(act)])
  inp = norms.inputs_of(3, 7, impl, True, 1.0, rng)
  x, scale, gout = (inp[k].astype(np.float64) for k in ('x', 'scale', 'gout'))
  shift = None if inp['shift'] is None else inp['shift'].astype(np.float64)
  ref = norms.reference64(x, scale, shift, impl, act, 1e-4, gout)
  assert np.allclose(ref['dx'], _central(lambda v: norms.reference64(v, scale, shift, impl, act, 1e-4)['out'], x, gout),
                     rtol=1e-6, atol=1e-8)
  assert np.allclose(ref['dscale'], _central(lambda v: norms.reference64(x, v, shift, impl, act, 1e-4)['out'], scale, gout),
                     rtol=1e-6, atol=1e-8)
  if shift is not None:
    assert np.allclose(ref['dshift'], _central(lambda v: norms.reference64(x, scale, v, impl, act, 1e-4)['out'], shift, gout),
                       rtol=1e-6, atol=1e-8)


def test_float32_definition_sits_inside_the_bars():
  """The restated arithmetic in float32 on the CPU against float64: worst share
  of every bar over the impls, activations, eps, input scales and a few widths."""
  worst = {}
  for units in (1, 3, 65, 257, 1025, 4097):
    for impl in norms.IMPLS:
      for act in norms.ACTS:
        for eps in norms.EPS:
          for scale in norms.SCALES:
            rng = np.random.default_rng([units, int(eps * 1e7)])
            inp = norms.inputs_of(3, units, impl, True, scale, rng)
            args = (inp['x'], inp['scale'], inp['shift'], impl, act, eps, inp['gout'])
            want, got = norms.reference64(*args), norms.evaluate(*args, dtype=np.float32)
            s = norms.row_scale(inp['gout'], inp['scale'], want['rstd'])
            ratios = {'out': norms.out_ratio(got['out'], want['out']), 'dx': norms.grad_ratio(got['dx'], want['dx'], s)}
            if units in (3, 65, 1025):                     # the column sums: cases.SUM_ROWS rows (see there)
              inp = norms.inputs_of(norms.SUM_ROWS, units, impl, True, scale, rng)
              args = (inp['x'], inp['scale'], inp['shift'], impl, act, eps, inp['gout'])
              want, got = norms.reference64(*args), norms.evaluate(*args, dtype=np.float32)
              ratios['dscale'] = norms.sum_ratio(got['dscale'], want['dscale'], want['dscale_abs'])
              ratios['dshift'] = norms.sum_ratio(got['dshift'], want['dshift'], want['dshift_abs'])
            for key, ratio in ratios.items():
              worst[key] = max(worst.get(key, 0.0), ratio)
  for key, ratio in sorted(worst.items()):
    print(f'float32 definition, {key}: {ratio:.3g} of its bar')
  assert max(worst.values()) <= 1.0, worst


def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'embodied/jax/nets.py:361-399' in text and 'embodied/jax/nets.py:26-39' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [11, 16, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays


def test_abi_refuses_bad_arguments_without_a_gpu():
  from embodied_amd import _lib
  raw, F32 = _lib.lib, _lib.F32
  for name in NAMES:
    getattr(raw, name).argtypes, getattr(raw, name).restype = _lib.SIGNATURES[name], C.c_int32
  buf = np.zeros(64, np.float32).ctypes.data
  norm = lambda **kw: raw.emb_norm_act(*[{**dict(x=buf, scale=None, shift=None, dtype=F32, rows=2, units=8, impl=0, act=1,
                                                 eps=1e-4, out=buf, stream=None), **kw}[k] for k in
                                         ('x', 'scale', 'shift', 'dtype', 'rows', 'units', 'impl', 'act', 'eps', 'out', 'stream')])
  for bad in (dict(x=None), dict(out=None), dict(units=0), dict(units=16385), dict(impl=2), dict(act=4), dict(act=-1),
              dict(dtype=_lib.F16), dict(rows=-1), dict(eps=-1.0), dict(eps=float('nan')), dict(rows=2 ** 31, units=8)):
    assert norm(**bad) == _lib.ERR_INVALID, bad
    assert b'norm_act' in raw.emb_last_error()
  assert norm(rows=0, x=None, out=None) == 0                 # no rows: nothing to do
  grad = lambda **kw: raw.emb_norm_act_grad(*[{**dict(x=buf, scale=None, shift=None, gout=buf, dtype=F32, rows=2, units=8,
                                                      impl=0, act=1, eps=1e-4, dx=buf, dscale=None, dshift=None,
                                                      partials=None, floats=0, stream=None), **kw}[k] for k in
                                              ('x', 'scale', 'shift', 'gout', 'dtype', 'rows', 'units', 'impl', 'act', 'eps',
                                               'dx', 'dscale', 'dshift', 'partials', 'floats', 'stream')])
  for bad in (dict(x=None), dict(gout=None), dict(dx=None), dict(dscale=buf), dict(dscale=buf, partials=buf, floats=15),
              dict(units=0), dict(impl=7)):
    assert grad(**bad) == _lib.ERR_INVALID, bad
  assert grad(dscale=buf, partials=buf, floats=15) == _lib.ERR_INVALID and b'16 float32' in raw.emb_last_error()
  assert raw.emb_norm_act_launches(None) == _lib.ERR_INVALID
  # the facade's count of partial sums is the library's, at every step of the width ladder
  for rows, units in ((1, 1), (5, 1024), (5, 1025), (2047, 512), (2048, 512), (2049, 512), (511, 4096), (513, 4096),
                      (600, 16384), (3, 8193)):
    floats = nets._partial_floats(rows, units)
    assert grad(rows=rows, units=units, dscale=buf, partials=buf, floats=floats - 1) == _lib.ERR_INVALID
    assert f'must hold {floats} float32'.encode() in raw.emb_last_error(), (rows, units)
def test_facade_refuses_cpu_tensors_and_bad_arguments():
  import embodied_amd as emb
  assert emb.nets is nets and emb.norm_act is nets.norm_act and emb.NormAct is nets.NormAct
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    nets.norm_act(torch.zeros(2, 8))
  assert nets._eps_of('rms1em6', 1e-4) == ('rms', 1e-6) and nets._eps_of('layer', 1e-4) == ('layer', 1e-4)
  with pytest.raises(ValueError, match='16384'):
    nets._norm_path(True, 2, 16385)
  with pytest.raises(ValueError, match='2\\^31 - 1'):
    nets._norm_path(True, 2 ** 20, 4096)
  assert nets._norm_path(None, 2, 16385) is False and nets._norm_path(None, 2, 16384) is True
  assert nets._norm_path(False, 2, 8) is False
  with pytest.raises(TypeError, match='float32'):
    nets._check_param('norm_act', 'scale', torch.ones(8, dtype=torch.float64), 8, torch.zeros(1))
  with pytest.raises(ValueError, match='shape'):
    nets._check_param('norm_act', 'scale', torch.ones(7), 8, torch.zeros(1))
