"""`embodied_amd.nets.gru_gate` and `emb_gru_gate*` as far as they go without a
GPU: the fixture, the restatement the GPU tests rely on, the bars, the
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

from tests import gru_gate_cases as gates

GOLDEN = ROOT / 'tests' / 'golden' / 'gru_gate.npz'
NAMES = ('emb_gru_gate', 'emb_gru_gate_grad', 'emb_gru_gate_launches')


def test_fixture_is_current():
  fresh = _fresh().generate_gate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_forward_bar():
  """`reference64` agrees with the reference's own float64 run of RSSM._core (its
  layers replaced by stand-ins, so that it returns the gate of x and deter) on
  every case; its float32 run sits inside the forward bar."""
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines__core']) == (135, 159)
    for case, (deter, blocks, scale) in enumerate(gates.CASES):
      name, inp = gates.tag(case), gates.inputs(case)
      assert np.array_equal(f[f'in_{name}'], gates.digest(inp)), name
      want, got32 = f[f'out64_{name}'], f[f'out_{name}']
      assert want.dtype == np.float64 and got32.dtype == np.float32 and want.shape == (gates.GOLDEN_ROWS, deter)
      assert np.allclose(gates.reference64(inp['x'], inp['deter'], blocks)['out'], want, rtol=1e-12, atol=1e-12), name
      worst = max(worst, gates.out_ratio(got32, want))
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0

def test_gru_gate_gradients_agree_with_central_differences():
  rng = np.random.default_rng(5)
  inp = gates.inputs_of(2, 12, 2.0, rng)
  x, d, gout = (inp[k].astype(np.float64) for k in ('x', 'deter', 'gout'))
  ref = gates.reference64(x, d, 4, gout)
  assert np.allclose(ref['dx'], _central(lambda v: gates.reference64(v, d, 4)['out'], x, gout), rtol=1e-6, atol=1e-9)
  assert np.allclose(ref['ddeter'], _central(lambda v: gates.reference64(x, v, 4)['out'], d, gout), rtol=1e-6, atol=1e-9)
  # the indexing of rssm.py:153-154, element by element
  h = 3
  for k in range(4):
    for j in range(h):
      r = 1 / (1 + np.exp(-x[1, 3 * h * k + j]))
      c = np.tanh(r * x[1, 3 * h * k + h + j])
      u = 1 / (1 + np.exp(-(x[1, 3 * h * k + 2 * h + j] - 1)))
      assert np.isclose(ref['out'][1, h * k + j], u * c + (1 - u) * d[1, h * k + j], rtol=1e-14)


def test_float32_definition_sits_inside_the_bars():
  worst = {}
  for rows, deter, blocks in ((3, 8, 4), (3, 12, 4), (37, 64, 8)):
    for scale in gates.SCALES + (30.0, 90.0):
      inp = gates.inputs_of(rows, deter, scale, np.random.default_rng([rows, deter]))
      args = (inp['x'], inp['deter'], blocks, inp['gout'])
      want, got = gates.reference64(*args), gates.evaluate(*args, dtype=np.float32)
      s = gates.row_scale(inp['gout'], inp['x'], inp['deter'])
      for key in ('dx', 'ddeter'):
        worst[key] = max(worst.get(key, 0.0), gates.grad_ratio(got[key], want[key], s))
      worst['out'] = max(worst.get('out', 0.0), gates.out_ratio(got['out'], want['out']))
  for key, ratio in sorted(worst.items()):
    print(f'float32 definition, {key}: {ratio:.3g} of its bar')
  assert max(worst.values()) <= 1.0, worst


def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/rssm.py:152-159' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [8, 10, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays


def test_abi_refuses_bad_arguments_without_a_gpu():
  from embodied_amd import _lib
  raw, F32 = _lib.lib, _lib.F32
  for name in NAMES:
    getattr(raw, name).argtypes, getattr(raw, name).restype = _lib.SIGNATURES[name], C.c_int32
  buf = np.zeros(64, np.float32).ctypes.data
  assert raw.emb_gru_gate(None, buf, F32, 2, 8, 4, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate(buf, buf, F32, 2, 8, 3, buf, None) == _lib.ERR_INVALID and b'divide' in raw.emb_last_error()
  assert raw.emb_gru_gate(buf, buf, F32, 2, 0, 1, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate(buf, buf, F32, 2, 8, 0, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate(buf, buf, _lib.F64, 2, 8, 4, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate(buf, buf, F32, 2 ** 28, 8, 4, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate_grad(buf, buf, None, F32, 2, 8, 4, buf, buf, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate_grad(buf, buf, buf, F32, 2, 8, 4, None, None, None) == _lib.ERR_INVALID
  assert raw.emb_gru_gate(None, None, F32, 0, 8, 4, None, None) == 0
  assert raw.emb_gru_gate_launches(None) == _lib.ERR_INVALID


def test_facade_refuses_cpu_tensors_and_bad_arguments():
  import embodied_amd as emb
  assert emb.nets is nets and emb.gru_gate is nets.gru_gate
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    nets.gru_gate(torch.zeros(2, 24), torch.zeros(2, 8), 4)
  with pytest.raises(ValueError, match='2\\^31 - 1'):
    nets._gate_path(True, 2 ** 20, 8192, 8)
  assert nets._gate_path(None, 2 ** 20, 8192, 8) is False and nets._gate_path(None, 16, 8192, 8) is True
