"""`emb_scan_lambda_cont`, `emb_dreamer_targets` / `scans.dreamer_targets` as far
as they go without a GPU: the declarations, the binding, the call shim, the
refusals that happen before any launch, the path decision and the fixture's
inputs.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import dreamer_target_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'dreamer_targets.npz'
NAMES = ('emb_scan_lambda_cont', 'emb_dreamer_targets', 'emb_dreamer_targets_launches')


def _config(impl=2, debias=1, rate=0.01, limit=1e-8, perclo=5.0, perchi=95.0):
  from embodied_amd import _lib
  return _lib.NormalizeConfig(impl, debias, rate, limit, perclo, perchi)


def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/agent.py:397-419' in text and 'dreamerv3/agent.py:401-405,482-490' in text
  assert re.search(r'#define\s+EMB_NORM_NONE\s+0', text) and _lib.NORM_NONE == 0
  assert len(_lib.SIGNATURES['emb_scan_lambda_cont']) == 9
  assert len(_lib.SIGNATURES['emb_dreamer_targets']) == 20
  assert _lib.fast.SHAPES['emb_scan_lambda_cont'] == 'scan_cont'
  assert _lib.fast.SHAPES['emb_dreamer_targets'] == 'dreamer_targets'
  assert _lib.fast.module is not None
  assert hasattr(_lib.fast.module, 'scan_cont') and hasattr(_lib.fast.module, 'dreamer_targets')
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  assert 'dreamer_targets.hip' in __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES


def test_scan_lambda_cont_refusals():
  from embodied_amd import _lib
  raw = _lib.lib.emb_scan_lambda_cont
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_scan_lambda_cont'], C.c_int32
  fake = np.zeros(16, np.float32)          # never dereferenced: every call below is refused or launches nothing
  x = C.c_void_p(fake.ctypes.data)

  def args(rew=x, con=x, boot=x, B=2, T=4, ret=x):
    return (rew, con, boot, B, T, 1.0, 0.95, ret, None)

  refused = [
      ('a pointer is null', args(rew=None)), ('a pointer is null', args(con=None)),
      ('a pointer is null', args(boot=None)), ('a pointer is null', args(ret=None)),
      ('negative B', args(B=-1)), ('T < 2', args(T=1)), ('T < 2', args(T=0)), ('T < 2', args(T=-2)),
      ('more than 2^31 - 1', args(B=1 << 16, T=1 << 15)), ('more than 2^31 - 1', args(B=1, T=1 << 31)),
      ('more than 2^31 - 1', args(B=1 << 62, T=1 << 62)),
  ]
  for message, call in refused:
    status = raw(*call)
    assert status == _lib.ERR_INVALID, (message, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert raw(*args(B=0)) == _lib.OK and raw(*args(B=0, T=0)) == _lib.OK
  with pytest.raises(ValueError, match='negative B'):        # the same through the call shim
    _lib.fast.emb_scan_lambda_cont(x.value, x.value, x.value, -1, 4, 1.0, 0.95, x.value, None)
  _lib.fast.emb_scan_lambda_cont(x.value, x.value, x.value, 0, 4, 1.0, 0.95, x.value, None)


def test_dreamer_targets_refusals_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import scans
  raw = _lib.lib.emb_dreamer_targets
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_dreamer_targets'], C.c_int32
  fake = np.zeros(64, np.float32)          # never dereferenced: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  s1, s2, s3 = (C.c_void_p(fake.ctypes.data + 32 * k) for k in (1, 2, 3))
  perc, meanstd, none = C.byref(_config()), C.byref(_config(impl=1)), C.byref(_config(impl=0))

  def args(rcfg=perc, vcfg=meanstd, acfg=meanstd, rew=x, con=x, pred=x, N=2, T=4, ret=x, weight=x, adv=x,
           adv_normed=x, tar_padded=x, rstate=s1, vstate=s2, astate=s3):
    return (rcfg, vcfg, acfg, rew, con, pred, N, T, 1.0, 0.95, 1, ret, weight, adv, adv_normed, tar_padded,
            rstate, vstate, astate, None)

  before = scans.dreamer_targets_launches()
  refused = [
      ('retnorm config is null', args(rcfg=None)), ('retnorm state is null', args(rstate=None)),
      ('retnorm must be EMB_NORM_PERC', args(rcfg=meanstd)), ('retnorm must be EMB_NORM_PERC', args(rcfg=none)),
      ('valnorm must be EMB_NORM_MEANSTD or none', args(vcfg=perc)),
      ('advnorm must be EMB_NORM_MEANSTD or none', args(acfg=perc)),
      ('emb_scan_lambda_cont + emb_normalize', args(rcfg=meanstd)),
      ('valnorm state is null', args(vstate=None)), ('advnorm state is null', args(astate=None)),
      ('share one state', args(vstate=s1)), ('share one state', args(astate=s1)),
      ('share one state', args(astate=s2)),
      ('an input is null', args(rew=None)), ('an input is null', args(con=None)),
      ('an input is null', args(pred=None)),
      ('an output is null', args(ret=None)), ('an output is null', args(weight=None)),
      ('an output is null', args(adv=None)), ('an output is null', args(adv_normed=None)),
      ('an output is null', args(tar_padded=None)),
      ('negative N', args(N=-1)), ('T < 2', args(T=1)), ('T < 2', args(T=0)), ('T < 2', args(T=-3)),
      ('T < 2', args(N=0, T=1)),
      ('more than 16384 returns', args(N=1024, T=18)), ('more than 16384 returns', args(N=1, T=16386)),
      ('more than 16384 returns', args(N=1 << 62, T=1 << 62)),
      ('emb_scan_lambda_cont + emb_normalize', args(N=16385, T=2)),
      ('rate outside', args(rcfg=C.byref(_config(rate=1.5)))),
      ('rate outside', args(vcfg=C.byref(_config(impl=1, rate=-0.1)))),
      ('rate outside', args(acfg=C.byref(_config(impl=1, rate=float('nan'))))),
      ('percentile outside', args(rcfg=C.byref(_config(perclo=-1.0)))),
      ('percentile outside', args(rcfg=C.byref(_config(perchi=100.5)))),
  ]
  for message, call in refused:
    status = raw(*call)
    assert status == _lib.ERR_INVALID, (message, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  # N = 0: nothing to do, nothing launched -- with every flavour of "no normaliser"
  assert raw(*args(N=0)) == _lib.OK
  assert raw(*args(N=0, rew=None, ret=None)) == _lib.OK
  assert raw(*args(N=0, vcfg=None, acfg=None, vstate=None, astate=None)) == _lib.OK
  assert raw(*args(N=0, vcfg=none, acfg=none, vstate=s1, astate=s1)) == _lib.OK     # states of none are not read
  assert scans.dreamer_targets_launches() == before
  config = _config()
  with pytest.raises(ValueError, match='negative N'):        # the same through the call shim
    _lib.fast.emb_dreamer_targets(
        C.addressof(config), None, None, x.value, x.value, x.value, -1, 4, 1.0, 0.95, 1, x.value, x.value,
        x.value, x.value, x.value, s1.value, None, None, None)
  _lib.fast.emb_dreamer_targets(
      C.addressof(config), None, None, None, None, None, 0, 4, 1.0, 0.95, 1, None, None, None, None, None,
      s1.value, None, None, None)
  assert scans.dreamer_targets_launches() == before
  assert _lib.lib.emb_dreamer_targets_launches(None) == _lib.ERR_INVALID


def test_facade_refuses_host_tensors_and_decides_the_path():
  import embodied_amd as emb
  from embodied_amd import scans
  x = torch.zeros(2, 4)
  norms = [emb.DeviceNormalize(impl) for impl in ('perc', 'none', 'none')]
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    scans.dreamer_targets(x, x, x, *norms)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    scans.lambda_return_cont(x, x, x, 1.0, 0.95)
  assert emb.DeviceNormalize('none').fused(torch.device('cuda', 0)) == (None, None)
  assert 'lambda_return_cont' in scans.lambda_return.__doc__

  path = scans._dreamer_targets_path
  norm = {impl: emb.DeviceNormalize(impl) for impl in ('perc', 'meanstd', 'none')}
  fits = [('perc', 'none', 'none'), ('perc', 'meanstd', 'meanstd'), ('perc', 'meanstd', 'none'),
          ('perc', 'none', 'meanstd')]
  other = [('meanstd', 'none', 'none'), ('none', 'none', 'none'), ('perc', 'perc', 'none'),
           ('perc', 'none', 'perc')]
  assert scans.DREAMER_TARGETS_FUSED_MAX <= 16384
  for impls in fits:
    trio = [norm[i] for i in impls]
    assert path(True, *trio, 16, 16) is True
    assert path(None, *trio, 16, 16) is (16 * 15 <= scans.DREAMER_TARGETS_FUSED_MAX)
    assert path(None, *trio, 1024, 16) is (1024 * 15 <= scans.DREAMER_TARGETS_FUSED_MAX)
    assert path(None, *trio, 1024, 18) is False
    assert path(False, *trio, 16, 16) is False
    assert path(True, *trio, 1024, 17) is True              # exactly the LDS limit
    with pytest.raises(ValueError, match=r'fused=True.*17408 returns.*16384'):
      path(True, *trio, 1024, 18)
  for impls in other:
    trio = [norm[i] for i in impls]
    with pytest.raises(ValueError, match="fused=True.*'perc' retnorm.*'%s', '%s' and '%s'" % impls):
      path(True, *trio, 16, 16)
    assert path(None, *trio, 16, 16) is False
    assert path(False, *trio, 16, 16) is False


def test_fixture_inputs_match_their_digests():
  with np.load(GOLDEN) as f:
    assert int(f['steps']) == cases.STEPS
    for case, c in enumerate(cases.CASES):
      N, T = c.shape
      name = cases.tag(case)
      for step in range(cases.STEPS):
        inp = cases.inputs(case, step)
        assert all(inp[k].shape == (N, T) and inp[k].dtype == np.float32 for k in ('rew', 'con', 'pred', 'slow'))
        assert ((inp['con'] == 0) | (inp['con'] == 1) | ((inp['con'] >= 0.9) & (inp['con'] < 1))).all()
        assert not np.array_equal(inp['pred'], inp['slow'])
        assert np.array_equal(f[f'in_{name}'][step], cases.digest(inp)), (name, step)
      for key in ('ret', 'adv', 'advnormed'):
        assert f[f'{key}_{name}'].shape == (cases.STEPS, N, T - 1), key
      for key in ('weight', 'tarpadded'):
        assert f[f'{key}_{name}'].shape == (cases.STEPS, N, T), key
      assert f[f'stats_{name}'].shape == (cases.STEPS, 6)
      assert np.isfinite(f[f'ret_{name}']).all()
      assert not f[f'tarpadded_{name}'][:, :, -1].any()
    # con really is a probability in the fixture: fractions, exact zeros and exact ones
    con = np.concatenate([cases.inputs(1, s)['con'].reshape(-1) for s in range(cases.STEPS)])
    assert 0.01 < (con == 0).mean() < 0.06 and 0.01 < (con == 1).mean() < 0.06
    # the tie case: both order statistics of both percentiles inside runs of equal values
    c = cases.CASES[cases.TIE_CASE]
    for ret in f[f'ret_{cases.tag(cases.TIE_CASE)}']:
      ordered = np.sort(ret.reshape(-1))
      for q in (5.0, 95.0):
        k = int(np.floor(q / 100 * (ordered.size - 1)))
        assert ordered[k] == ordered[k + 1] and (ordered == ordered[k]).sum() >= c.shape[0]
  assert GOLDEN.stat().st_size < 900_000


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location(
      '_gen_dreamer_targets', ROOT / 'tools' / 'gen_dreamer_targets_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key
