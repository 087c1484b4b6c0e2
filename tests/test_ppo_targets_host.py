"""`emb_ppo_targets` / `scans.ppo_targets` as far as they go without a GPU: the
declaration, the binding, the call shim, the refusals that happen before any
launch, and the fixture's inputs.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import ppo_target_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'ppo_targets.npz'


def _config(impl=1, debias=1, rate=0.01, limit=1e-8):
  from embodied_amd import _lib
  return _lib.NormalizeConfig(impl, debias, rate, limit, 5.0, 95.0)


def test_header_declares_and_binding_covers_emb_ppo_targets():
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  assert re.search(r'int32_t\s+emb_ppo_targets\s*\(', text)
  assert re.search(r'int32_t\s+emb_ppo_targets_launches\s*\(', text)
  assert 'ppo/agent.py:188-210' in text
  for name in ('emb_ppo_targets', 'emb_ppo_targets_launches'):
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert len(_lib.SIGNATURES['emb_ppo_targets']) == 19
  assert _lib.fast.SHAPES['emb_ppo_targets'] == 'ppo_targets'
  assert _lib.fast.module is not None and hasattr(_lib.fast.module, 'ppo_targets')
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays


def test_bad_arguments_are_refused_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import scans
  raw = _lib.lib.emb_ppo_targets
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_ppo_targets'], C.c_int32
  fake = np.zeros(64, np.float32)          # never dereferenced: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  other = C.c_void_p(fake.ctypes.data + 32)
  good = C.byref(_config())

  def args(vcfg=good, acfg=good, rew=x, pred=x, last=x, term=x, B=2, T=4, tarclip=10.0, adv=x, tar=x,
           tar_normed=x, adv_normed=x, vstate=x, astate=other):
    return (vcfg, acfg, rew, pred, last, term, B, T, 0.995, 0.8, tarclip, 1, adv, tar, tar_normed,
            adv_normed, vstate, astate, None)

  before = scans.ppo_targets_launches()
  refused = [
      ('a config is null', args(vcfg=None)), ('a config is null', args(acfg=None)),
      ('a state is null', args(vstate=None)), ('a state is null', args(astate=None)),
      ('share one state', args(astate=x)),
      ('an input is null', args(rew=None)), ('an input is null', args(pred=None)),
      ('an input is null', args(last=None)), ('an input is null', args(term=None)),
      ('an output is null', args(adv=None)), ('an output is null', args(tar=None)),
      ('an output is null', args(tar_normed=None)), ('an output is null', args(adv_normed=None)),
      ('negative B', args(B=-1)), ('T < 2', args(T=1)), ('T < 2', args(T=0)), ('T < 2', args(T=-3)),
      ('more than 2^31 - 1', args(B=1 << 16, T=1 << 15)), ('more than 2^31 - 1', args(B=1, T=1 << 31)),
      ('more than 2^31 - 1', args(B=1 << 62, T=1 << 62)),
      ('EMB_NORM_MEANSTD', args(vcfg=C.byref(_config(impl=2)))),
      ('EMB_NORM_MEANSTD', args(acfg=C.byref(_config(impl=2)))),
      ('EMB_NORM_MEANSTD', args(acfg=C.byref(_config(impl=0)))),
      ('rate outside', args(vcfg=C.byref(_config(rate=1.5)))),
      ('negative tarclip', args(tarclip=-1.0)), ('negative tarclip', args(tarclip=float('nan'))),
  ]
  for message, call in refused:
    status = raw(*call)
    assert status == _lib.ERR_INVALID, (message, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert raw(*args(B=0)) == _lib.OK                          # nothing to do, nothing launched
  assert raw(*args(B=0, T=0, rew=None, adv=None)) == _lib.OK
  assert scans.ppo_targets_launches() == before
  config = _config()
  with pytest.raises(ValueError, match='negative B'):        # the same through the call shim
    _lib.fast.emb_ppo_targets(
        C.addressof(config), C.addressof(config), x.value, x.value, x.value, x.value, -1, 4, 0.995, 0.8, 10.0,
        1, x.value, x.value, x.value, x.value, x.value, other.value, None)
  _lib.fast.emb_ppo_targets(
      C.addressof(config), C.addressof(config), None, None, None, None, 0, 4, 0.995, 0.8, 10.0, 1, None, None,
      None, None, x.value, other.value, None)
  assert scans.ppo_targets_launches() == before
  assert _lib.lib.emb_ppo_targets_launches(None) == _lib.ERR_INVALID


def test_facade_refuses_host_tensors_and_other_impls():
  import embodied_amd as emb
  from embodied_amd import scans
  x, flag = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.bool)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    scans.ppo_targets(x, x, flag, flag, emb.DeviceNormalize('meanstd'), emb.DeviceNormalize('meanstd'))

  class OnDevice:                      # enough of a CUDA tensor for the checks that come before any launch
    is_cuda, device, dtype, shape = True, torch.device('cuda', 0), torch.float32, (2, 4)

  # (refused on the normalisers' impls before a tensor is touched)
  for valnorm, advnorm in (('perc', 'meanstd'), ('meanstd', 'perc'), ('none', 'meanstd')):
    with pytest.raises(ValueError, match="fused=True.*'meanstd'"):
      scans._ppo_targets_path(True, emb.DeviceNormalize(valnorm), emb.DeviceNormalize(advnorm), 2, 4)
  meanstd = emb.DeviceNormalize('meanstd')
  assert scans._ppo_targets_path(None, meanstd, meanstd, 16, 64) is (16 * 64 <= scans.PPO_TARGETS_FUSED_MAX)
  assert scans._ppo_targets_path(None, meanstd, meanstd, 1 << 16, 64) is False
  assert scans._ppo_targets_path(None, meanstd, emb.DeviceNormalize('perc'), 2, 4) is False
  assert scans._ppo_targets_path(False, meanstd, meanstd, 2, 4) is False
  assert scans._ppo_targets_path(True, meanstd, meanstd, 1 << 16, 64) is True


def test_fixture_inputs_match_their_digests():
  with np.load(GOLDEN) as f:
    assert int(f['steps']) == cases.STEPS
    for case, ((B, T), tarclip) in enumerate(cases.CASES):
      name = cases.tag(case)
      for step in range(cases.STEPS):
        inp = cases.inputs(case, step)
        assert inp['rew'].shape == (B, T) and inp['last'].dtype == bool
        for row in (0, B - 1):
          assert inp['last'][row, 1] and inp['term'][row, T - 1]
        assert np.array_equal(f[f'in_{name}'][step], cases.digest(inp)), (name, step)
      assert f[f'adv_{name}'].shape == (cases.STEPS, B, T - 1)
      assert f[f'tarnormed_{name}'].shape == (cases.STEPS, B, T)
      assert f[f'stats_{name}'].shape == (cases.STEPS, 4)
      assert not f[f'tarnormed_{name}'][:, :, -1].any()
    clipped = np.abs(f[f'tarnormed_{cases.tag(cases.CLIP_CASE)}'][:, :, :-1]) == np.float32(2.0)
    assert 0.01 <= clipped.mean() <= 0.5


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'ppo' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_ppo_targets', ROOT / 'tools' / 'gen_ppo_targets_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key
