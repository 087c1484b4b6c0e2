"""`embodied_amd.nets.pool_norm_act` / `norm_act_upsample` and `emb_pool_norm_act*`,
`emb_norm_act_upsample*` as far as they go without a GPU: the fixture, the
restatement the GPU tests rely on (forward, gradients, the tie rule), the
declarations and the binding, the refusals that happen before any launch.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from embodied_amd import nets
from tests import conv_stage_cases as stages
from tests import norm_act_cases as norms
from tests.test_norm_act_host import _central

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'conv_stage.npz'
NAMES = ('emb_pool_norm_act', 'emb_pool_norm_act_grad', 'emb_norm_act_upsample', 'emb_norm_act_upsample_grad',
         'emb_conv_stage_launches')


def test_fixture_is_current():
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'rssm.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_conv_stage', ROOT / 'tools' / 'gen_conv_stage_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_forward_bar():
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_Norm']) == (361, 409) and tuple(f['lines_act']) == (26, 39)
    assert tuple(f['lines_pool']) == (239, 240) and tuple(f['lines_repeat']) == (336,)
    for case, c in enumerate(stages.CASES):
      name, inp = stages.tag(case), stages.inputs(case)
      assert np.array_equal(f[f'in_{name}'], stages.digest(stages.present(inp))), name
      want, got32 = f[f'out64_{name}'], f[f'out_{name}']
      assert want.dtype == np.float64 and got32.dtype == np.float32 and np.isfinite(want).all()
      assert want.shape == stages.out_shape(c.stage, inp['x'].shape)
      mine = stages.reference(c.stage, inp['x'], inp['scale'], inp['shift'], c.impl, c.act, c.eps)['out']
      assert np.allclose(mine, want, rtol=1e-12, atol=1e-12), name
      worst = max(worst, norms.out_ratio(got32, want))
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0
  assert GOLDEN.stat().st_size < 900_000
  cases = stages.CASES
  assert len(cases) == 12 and {c.stage for c in cases} == set(stages.STAGES)
  assert {c.impl for c in cases} == set(stages.IMPLS) and {c.act for c in cases} == set(stages.ACTS)
  assert {c.units for c in cases} == {1, 3, 65, 257} and {(c.height, c.width) for c in cases} == {(2, 2), (2, 6), (4, 4)}
  assert {(c.stage, c.impl) for c in cases} == {(s, i) for s in stages.STAGES for i in stages.IMPLS}


@pytest.mark.parametrize('stage', stages.STAGES)
@pytest.mark.parametrize('impl', stages.IMPLS)
@pytest.mark.parametrize('act', stages.ACTS)
def test_stage_gradients_agree_with_central_differences(stage, impl, act):
  """On inputs without ties (a tie is a kink: no derivative to difference)."""
  rng = np.random.default_rng([stages.STAGES.index(stage), stages.IMPLS.index(impl), stages.ACTS.index(act)])
  inp = stages.inputs_of(stage, 2, 2, 4, 5, impl, True, 1.0, rng)
  x, scale, gout = (inp[k].astype(np.float64) for k in ('x', 'scale', 'gout'))
  shift = None if inp['shift'] is None else inp['shift'].astype(np.float64)
  if stage == 'pool':
    win = np.sort(stages.windows(x), 1)
    assert (win[:, 3] - win[:, 2] > 1e-3).all()                    # no ties, and none within the difference step
  ref = stages.reference(stage, x, scale, shift, impl, act, 1e-4, gout)
  run = lambda x, scale, shift: stages.reference(stage, x, scale, shift, impl, act, 1e-4)['out']
  assert np.allclose(ref['dx'], _central(lambda v: run(v, scale, shift), x, gout), rtol=1e-6, atol=1e-8)
  assert np.allclose(ref['dscale'], _central(lambda v: run(x, v, shift), scale, gout), rtol=1e-6, atol=1e-8)
  if shift is not None:
    assert np.allclose(ref['dshift'], _central(lambda v: run(x, scale, v), shift, gout), rtol=1e-6, atol=1e-8)


def test_tie_rule_against_a_hand_written_window():
  """One 2x2 image of four channels: no tie, and a 2-, 3- and 4-way tie.  With
  impl rms, act none and eps 0 the pooled row m has the gradient
  g = r gout - m r^3 (gout . m) / 4, r = 1 / sqrt(mean(m^2))."""
  x = np.array([[[1., 2., 3., 0.], [0., 2., 3., 0.]],
                [[0., 1., 3., -0.], [0., 0., 1., 0.]]])[None]      # (1, 2, 2, 4); channel 3: +0 and -0 tie
  gout = np.array([1., -2., 3., 5.]).reshape(1, 1, 1, 4)
  m = np.array([1., 2., 3., 0.])
  r = 1 / np.sqrt((m * m).mean())
  g = r * gout.reshape(4) - m * r ** 3 * (gout.reshape(4) * m).sum() / 4
  want = np.zeros((1, 2, 2, 4))
  want[0, 0, 0, 0] = g[0]
  want[0, 0, 0, 1] = want[0, 0, 1, 1] = g[1] / 2
  want[0, 0, 0, 2] = want[0, 0, 1, 2] = want[0, 1, 0, 2] = g[2] / 3
  want[0, :, :, 3] = g[3] / 4
  ref = stages.reference('pool', x, None, None, 'rms', 'none', 0.0, gout)
  assert np.allclose(ref['out'].reshape(4), m * r, rtol=1e-14)
  assert np.allclose(ref['dx'], want, rtol=1e-13, atol=0) and (ref['dx'][want == 0] == 0).all()
  # torch.amax on the CPU splits the same way: the composed path's rule
  t = torch.tensor(x, requires_grad=True)
  nets._composed_pool_norm_act(t, None, None, 'rms', 'none', 0.0).backward(torch.tensor(gout))
  assert np.allclose(t.grad.numpy(), want, rtol=1e-5, atol=1e-7) and (t.grad.numpy()[want == 0] == 0).all()
  # ... and the composed upsample repeats element by element, not tile by tile
  u = torch.arange(8.).reshape(1, 2, 2, 2) + 1
  up = nets._composed_norm_act_upsample(u, None, None, 'rms', 'none', 0.0)
  small = nets._composed_norm_act(u, None, None, 'rms', 'none', 0.0)
  assert up.shape == (1, 4, 4, 2)
  for i in (0, 1):
    for j in (0, 1):
      assert torch.equal(up[:, i::2, j::2], small)


def test_float32_definition_sits_inside_the_bars():
  """The restated stages in float32 on the CPU against float64, column sums too."""
  worst = {}
  for stage in stages.STAGES:
    for units in (3, 65, 257):
      for impl in stages.IMPLS:
        for act in stages.ACTS:
          rng = np.random.default_rng([units, stages.ACTS.index(act)])
          images, height, width = (4, 20, 16) if stage == 'pool' else (4, 10, 8)      # 320 Norm rows >= SUM_ROWS
          inp = stages.inputs_of(stage, images, height, width, units, impl, True, 1.0, rng)
          args = (stage, inp['x'], inp['scale'], inp['shift'], impl, act, 1e-4, inp['gout'])
          want, got = stages.reference(*args), stages.reference(*args, dtype=np.float32)
          found = stages.ratios(stage, want, got['out'], got['dx'], got['dscale'], got['dshift'], sums=True)
          for key, ratio in found.items():
            worst[key] = max(worst.get(key, 0.0), ratio)
  for key, ratio in sorted(worst.items()):
    print(f'float32 definition, {key}: {ratio:.3g} of its bar')
  assert max(worst.values()) <= 1.0, worst


def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib
  from tests.test_abi_symbols import declared_symbols
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/rssm.py:238-241' in text and 'dreamerv3/rssm.py:327, 336-338, 346' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [13, 18, 13, 18, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  count = len(declared_symbols())
  assert f'it exports ({count} functions)' in text
  assert f'the C ABI ({count} entry points' in (ROOT / 'README.md').read_text()
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'conv_stage.hip' in sources and 'conv_stage_abi.cpp' in sources


FORWARD = ('x', 'scale', 'shift', 'dtype', 'images', 'H', 'W', 'C', 'impl', 'act', 'eps', 'out', 'stream')
GRAD = ('x', 'scale', 'shift', 'gout', 'dtype', 'images', 'H', 'W', 'C', 'impl', 'act', 'eps', 'dx', 'dscale', 'dshift',
        'partials', 'floats', 'stream')


@pytest.mark.parametrize('stage', stages.STAGES)
def test_abi_refuses_bad_arguments_without_a_gpu(stage):
  from embodied_amd import _lib
  raw, F32 = _lib.lib, _lib.F32
  for name in NAMES:
    getattr(raw, name).argtypes, getattr(raw, name).restype = _lib.SIGNATURES[name], C.c_int32
  pool = stage == 'pool'
  who = b'pool_norm_act' if pool else b'norm_act_upsample'
  forward = raw.emb_pool_norm_act if pool else raw.emb_norm_act_upsample
  backward = raw.emb_pool_norm_act_grad if pool else raw.emb_norm_act_upsample_grad
  buf = np.zeros(256, np.float32).ctypes.data
  base = dict(x=buf, scale=None, shift=None, dtype=F32, images=2, H=2, W=4, C=8, impl=0, act=1, eps=1e-4, out=buf,
              stream=None)
  call = lambda **kw: forward(*[{**base, **kw}[k] for k in FORWARD])
  # the larger tensor: x of the pool (H W C), the result of the upsample (4 H W C)
  too_many = dict(images=2 ** 20, H=64, W=32, C=1) if pool else dict(images=2 ** 20, H=32, W=16, C=1)
  bad_calls = [dict(x=None), dict(out=None), dict(C=0), dict(C=1025), dict(impl=2), dict(act=4), dict(act=-1),
               dict(dtype=_lib.F16), dict(images=-1), dict(H=0), dict(W=0), dict(eps=-1.0), dict(eps=float('nan')),
               dict(eps=float('inf')), too_many]
  if pool:
    bad_calls += [dict(H=3), dict(W=5)]
  for bad in bad_calls:
    assert call(**bad) == _lib.ERR_INVALID, bad
    assert who in raw.emb_last_error(), bad
  if pool:
    assert call(H=3) == _lib.ERR_INVALID and b'odd H' in raw.emb_last_error()
    assert call(W=5) == _lib.ERR_INVALID and b'odd W' in raw.emb_last_error()
  else:
    assert call(H=3, W=5, x=None) == _lib.ERR_INVALID and b'null' in raw.emb_last_error()    # odd sizes are fine here
  assert call(C=1025) == _lib.ERR_INVALID and b'1024' in raw.emb_last_error()
  assert call(**too_many) == _lib.ERR_INVALID and b'2^31 - 1' in raw.emb_last_error()
  assert call(images=0, x=None, out=None) == 0                 # no images: nothing to do
  gbase = dict(x=buf, scale=None, shift=None, gout=buf, dtype=F32, images=2, H=2, W=4, C=8, impl=0, act=1, eps=1e-4,
               dx=buf, dscale=None, dshift=None, partials=None, floats=0, stream=None)
  grad = lambda **kw: backward(*[{**gbase, **kw}[k] for k in GRAD])
  bad_calls = [dict(x=None), dict(gout=None), dict(dx=None), dict(dscale=buf), dict(dscale=buf, partials=buf, floats=15),
               dict(C=0), dict(C=1025), dict(impl=7), dict(act=9), dict(dtype=_lib.I32), dict(eps=-1e-4), too_many]
  if pool:
    bad_calls += [dict(H=3), dict(W=5)]
  for bad in bad_calls:
    assert grad(**bad) == _lib.ERR_INVALID, bad
    assert who in raw.emb_last_error(), bad
  assert grad(dx=None) == _lib.ERR_INVALID and b'no output' in raw.emb_last_error()
  assert grad(dx=None, images=0) == _lib.ERR_INVALID           # no output requested, even with nothing to do
  assert grad(images=0, x=None, gout=None) == 0
  assert grad(dscale=buf, partials=buf, floats=15) == _lib.ERR_INVALID and b'16 float32' in raw.emb_last_error()
  # the facade's count of partial sums is the library's, at every step of the lanes ladder and past the cap
  for pixels_h, pixels_w, units in ((1, 1, 1), (1, 31, 64), (1, 33, 64), (2, 8, 65), (3, 11, 128), (3, 11, 129),
                                    (5, 7, 256), (5, 7, 257), (1, 5, 1024), (200, 200, 3), (130, 130, 64), (70, 60, 512)):
    height, width = (2 * pixels_h, 2 * pixels_w) if pool else (pixels_h, pixels_w)
    floats = nets._stage_partial_floats(pixels_h * pixels_w, units)
    assert floats == 2 * min(-(-pixels_h * pixels_w // (256 // stages.lanes(units))), stages.MAX_PARTIALS) * units
    assert grad(images=1, H=height, W=width, C=units, dscale=buf, partials=buf, floats=floats - 1) == _lib.ERR_INVALID
    assert f'must hold {floats} float32'.encode() in raw.emb_last_error(), (pixels_h, pixels_w, units)
  assert raw.emb_conv_stage_launches(None) == _lib.ERR_INVALID


def test_facade_refuses_cpu_tensors_and_bad_arguments():
  import embodied_amd as emb
  assert emb.pool_norm_act is nets.pool_norm_act and emb.norm_act_upsample is nets.norm_act_upsample
  assert emb.PoolNormAct is nets.PoolNormAct and emb.NormActUpsample is nets.NormActUpsample
  assert issubclass(nets.PoolNormAct, nets.NormAct) and issubclass(nets.NormActUpsample, nets.NormAct)
  for call in (nets.pool_norm_act, nets.norm_act_upsample):
    with pytest.raises(RuntimeError, match='no CPU fallback'):
      call(torch.zeros(2, 4, 4, 8))
  for path, name in ((nets._pool_path, 'pool_norm_act'), (nets._upsample_path, 'norm_act_upsample')):
    with pytest.raises(ValueError, match=f'{name}.*1024'):
      path(True, 2, 4, 4, 1025)
    with pytest.raises(ValueError, match='2\\^31 - 1'):
      path(True, 2 ** 20, 64, 64, 8)
    assert path(None, 2, 4, 4, 1025) is False and path(False, 2, 4, 4, 8) is False and path(True, 2, 4, 4, 1024) is True
  # the index limit is on the larger tensor: the upsample's result is four times its x
  assert nets._pool_path(True, 1, 2 ** 10, 2 ** 10, 1024) is True
  assert nets._upsample_path(None, 1, 2 ** 10, 2 ** 10, 1024) is False
  assert [stages.lanes(u) for u in (1, 64, 65, 128, 129, 256, 257, 1024)] == [
      nets._stage_lanes(u) for u in (1, 64, 65, 128, 129, 256, 257, 1024)] == [8, 8, 16, 16, 32, 32, 64, 64]
