"""`emb_normalize` / `DeviceNormalize` as far as they go without a GPU: the
declaration, the binding, the refusals that happen before any launch, and the
'none' normaliser.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_header_declares_and_binding_covers_emb_normalize():
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  assert re.search(r'int32_t\s+emb_normalize\s*\(', text)
  assert 'embodied/jax/utils.py:16-91' in text
  for name in ('emb_normalize', 'emb_normalize_launches'):
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'emb_normalize' in _lib.fast.SHAPES
  assert _lib.lib.emb_abi_version() == 5                   # an addition: the version stays
  # emb_normalize_config_t: two int32, four double
  assert C.sizeof(_lib.NormalizeConfig) == 40
  assert _lib.NormalizeConfig.perclo.offset == 24


def _config(impl=1, debias=1, rate=0.01, limit=1e-8, perclo=5.0, perchi=95.0):
  from embodied_amd import _lib
  return _lib.NormalizeConfig(impl, debias, rate, limit, perclo, perchi)


def test_bad_arguments_are_refused_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import normalize
  raw = _lib.lib.emb_normalize
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_normalize'], C.c_int32
  fake = np.zeros(64, np.float32)          # never dereferenced: every call below is refused first
  x = state = C.c_void_p(fake.ctypes.data)
  good = _config()
  before = normalize.launches()
  cases = [
      ('config is null', (None, x, 8, state, 1, None, None, None)),
      ('state is null', (C.byref(good), x, 8, None, 1, None, None, None)),
      ('x is null', (C.byref(good), None, 8, state, 1, None, None, None)),
      ('negative n', (C.byref(good), x, -1, state, 1, None, None, None)),
      ('unknown impl', (C.byref(_config(impl=7)), x, 8, state, 1, None, None, None)),
      ('unknown impl', (C.byref(_config(impl=0)), x, 8, state, 1, None, None, None)),
      ('percentile outside', (C.byref(_config(impl=2, perclo=-0.5)), x, 8, state, 1, None, None, None)),
      ('percentile outside', (C.byref(_config(impl=2, perchi=100.5)), x, 8, state, 1, None, None, None)),
      ('percentile outside', (C.byref(_config(impl=2, perchi=float('nan'))), x, 8, state, 1, None, None, None)),
      ('rate outside', (C.byref(_config(rate=1.5)), x, 8, state, 1, None, None, None)),
      ('update needs at least one value', (C.byref(good), x, 0, state, 1, None, None, None)),
      ('sub without out', (C.byref(good), x, 8, state, 1, x, None, None)),
  ]
  for message, args in cases:
    status = raw(*args)
    assert status == _lib.ERR_INVALID, (message, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert normalize.launches() == before
  with pytest.raises(ValueError, match='negative n'):         # the same through the call shim
    _lib.fast.emb_normalize(C.addressof(good), fake.ctypes.data, -1, fake.ctypes.data, 1, None, None, None)
  assert _lib.lib.emb_normalize_launches(None) == _lib.ERR_INVALID


def test_none_normaliser_needs_no_gpu():
  import embodied_amd as emb
  from embodied_amd import normalize
  norm = emb.DeviceNormalize('none')
  before = normalize.launches()
  x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
  assert norm(x) == (0.0, 1.0) and norm(x, update=False) == (0.0, 1.0) and norm.stats() == (0.0, 1.0)
  norm.update(x)
  assert torch.equal(norm.normalize(x), x)
  assert torch.equal(norm.normalize(x, sub=torch.ones_like(x)), x - 1)
  out = torch.empty_like(x)
  assert norm.normalize(x, out=out) is out and torch.equal(out, x)
  assert norm.state_dict() == {}
  norm.load_state_dict({})
  assert normalize.launches() == before


def test_unknown_impl_and_host_input():
  import embodied_amd as emb
  with pytest.raises(NotImplementedError):
    emb.DeviceNormalize('bogus')
  norm = emb.DeviceNormalize('perc')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    norm(torch.zeros(4))


def test_checkpoint_before_the_device_is_known():
  """A state loaded from host numbers is kept until the first call names the
  device; until then state_dict() hands the same numbers back."""
  import embodied_amd as emb
  norm = emb.DeviceNormalize('meanstd')
  norm.load_state_dict({'mean': 1.5, 'sqrs': torch.tensor(4.0), 'corr': 0.25, 'lo': 9.0})
  state = norm.state_dict()
  assert sorted(state) == ['corr', 'mean', 'sqrs']
  assert [float(state[k]) for k in ('mean', 'sqrs', 'corr')] == [1.5, 4.0, 0.25]
  assert sorted(emb.DeviceNormalize('perc', debias=False).state_dict()) == ['hi', 'lo']
