"""`embodied_amd.outs.OneHot` / `rssm_kl` and `emb_onehot_kl*` as far as they go
without a GPU: the fixture, the restatement the GPU tests rely on, the bars,
the declarations and the binding, the refusals that happen before any launch.
CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import rssm_kl_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'rssm_kl.npz'
NAMES = ('emb_onehot_kl', 'emb_onehot_kl_grad', 'emb_onehot_kl_launches')


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'rssm.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_rssm_kl', ROOT / 'tools' / 'gen_rssm_kl_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key], equal_nan=f[key].dtype.kind == 'f'), key


def test_restatement_equals_the_fixture_and_float32_sits_inside_the_bars():
  """The fixture belongs to `cases.inputs`; `cases.reference64` agrees with the
  reference's own float64 run on every case; the reference's float32 run sits
  inside the forward bars 1e-5 + 1e-5 |want|, so they leave room for another
  reduction order and not more."""
  worst = 0.0
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_loss']) == (120, 133) and tuple(f['lines__dist']) == (173, 176)
    assert tuple(f['lines_Agg']) == (40, 76) and tuple(f['lines_Categorical']) == (208, 240)
    assert tuple(f['lines_OneHot']) == (243, 270)
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      inp = cases.inputs(case)
      assert np.array_equal(f[f'in_{name}'], cases.digest(inp)), name
      want, got32 = f[f'out64_{name}'], f[f'out_{name}']
      assert want.dtype == np.float64 and got32.dtype == np.float32
      assert want.shape == got32.shape == (len(cases.FIELDS), cases.ROWS) and np.isfinite(want).all(), name
      ref = {free: cases.reference64(inp['post'], inp['prior'], c.unimix, free) for free in cases.FREE_NATS}
      mine = np.stack([ref[0.0]['kl'], ref[1.0]['dyn'], ref[1.0]['ent_post'], ref[1.0]['ent_prior']])
      assert np.allclose(mine, want, rtol=1e-12, atol=1e-12), name
      assert np.array_equal(ref[0.0]['dyn'], ref[0.0]['kl']) and np.array_equal(ref[1.0]['rep'], ref[1.0]['dyn'])
      assert np.array_equal(ref[1.0]['dyn'], np.maximum(ref[1.0]['kl'], 1.0))
      worst = max(worst, cases.forward_ratio(got32, want))
    # both sides of free_nats = 1 occur, inside one case too
    below = [(f[f'out64_{cases.tag(i)}'][0] < 1.0) for i in range(len(cases.CASES))]
    assert any(b.any() and not b.all() for b in below) and any(b.all() for b in below)
  print(f'the reference in float32: {worst:.3g} of the forward bar')
  assert worst <= 1.0
  assert GOLDEN.stat().st_size < 900_000


def test_float32_definition_against_the_gradient_bar():
  """The composed arithmetic in float32 on the CPU, rows 37, float32 and
  bfloat16-rounded inputs: inside the gradient bar 1e-5 |g| (1 + |want|) with
  unimix = 0.01 at every scale and with unimix = 0 at scales <= 1; at larger
  scales unimix = 0 multiplies by log p - log q of order 1e2 .. 1e5 and only
  finiteness is asked, there and on the GPU."""
  rng = np.random.default_rng(5)
  worst = {}
  for stoch, classes in ((32, 32), (3, 5)):
    for scale in cases.SCALES:
      for unimix in cases.UNIMIX:
        for rounded in (False, True):
          post, prior = cases.logits_of(cases.ROWS, stoch, classes, scale, rng)
          if rounded:
            post, prior = cases.bf16_round(post), cases.bf16_round(prior)
          g_dyn, g_rep = rng.standard_normal((2, cases.ROWS)).astype(np.float32)
          want = cases.reference64(post, prior, unimix, 0.0, g_dyn, g_rep)
          got = cases.restate(post, prior, unimix, 0.0, g_dyn, g_rep, torch.float32)
          forward = max(cases.forward_ratio(got[k], want[k]) for k in ('kl', 'ent_post', 'ent_prior'))
          assert forward <= 1.0, (stoch, classes, scale, unimix, forward)
          if unimix == 0.0 and scale not in cases.GRAD_SCALES_NO_UNIMIX:
            assert np.isfinite(got['grad_post']).all() and np.isfinite(got['grad_prior']).all()
            continue
          ratio = max(cases.grad_ratio(got['grad_post'], want['grad_post'], g_rep),
                      cases.grad_ratio(got['grad_prior'], want['grad_prior'], g_dyn))
          worst[unimix] = max(worst.get(unimix, 0.0), ratio)
  print(f'float32 definition, gradient: {worst} of the bar')
  assert max(worst.values()) <= 1.0, worst


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/rssm.py:123-132' in text and 'embodied/jax/outs.py:208-263' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [14, 14, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'onehot_kl.hip' in sources and 'onehot_kl_abi.cpp' in sources
  kernels_abi = (ROOT / 'embodied_amd' / 'csrc' / 'kernels_abi.cpp').read_text()
  assert 'onehot' not in kernels_abi                       # that file is linked into the host sanitizer soak
  assert emb.OneHot is emb.outs.OneHot and emb.rssm_kl is emb.outs.rssm_kl
  assert emb.onehot_kl_launches() == emb.outs.onehot_kl_launches()


def test_refusals_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import outs
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def forward(post=x, prior=x, dtype=_lib.F32, rows=4, stoch=2, classes=8, unimix=0.01, free=1.0, kl=x, ep=x, eq=x,
              dyn=x, rep=x):
    return raws['emb_onehot_kl'](post, prior, dtype, rows, stoch, classes, unimix, free, kl, ep, eq, dyn, rep, None)

  def grad(post=x, prior=x, dtype=_lib.BF16, rows=4, stoch=2, classes=8, unimix=0.01, free=1.0, kl=x, g_rep=x,
           g_dyn=x, grad_post=x, grad_prior=x):
    return raws['emb_onehot_kl_grad'](post, prior, dtype, rows, stoch, classes, unimix, free, kl, g_rep, g_dyn,
                                      grad_post, grad_prior, None)

  before = outs.onehot_kl_launches()
  shape = [('negative rows', dict(rows=-1)), ('stoch must be', dict(stoch=0)), ('classes outside 1 .. 256', dict(classes=0)),
           ('classes outside 1 .. 256', dict(classes=257)), ('more than 2^31 - 1', dict(rows=(1 << 31) // 16)),
           ('more than 2^31 - 1', dict(rows=1 << 62, stoch=1 << 20, classes=256)),
           ('more than 2^31 - 1', dict(rows=1, stoch=1 << 31, classes=2)),
           ('dtype must be', dict(dtype=_lib.F16)), ('dtype must be', dict(dtype=_lib.F64)),
           ('unimix outside', dict(unimix=-0.1)), ('unimix outside', dict(unimix=1.0)),
           ('unimix outside', dict(unimix=float('nan'))), ('free_nats must be', dict(free=-1.0)),
           ('free_nats must be', dict(free=float('nan')))]
  refused = []
  for call in (forward, grad):
    refused += [(call, message, kw) for message, kw in shape]
    refused += [(call, 'a pointer is null', {key: None}) for key in ('post', 'prior', 'kl')]
  refused += [(forward, 'a pointer is null', dict(ep=None)), (forward, 'a pointer is null', dict(eq=None)),
              (grad, 'both gradients are null', dict(grad_post=None, grad_prior=None)),
              (grad, 'grad_post without g_rep', dict(g_rep=None)), (grad, 'grad_prior without g_dyn', dict(g_dyn=None))]
  for call, message, kw in refused:
    status = call(**kw)
    assert status == _lib.ERR_INVALID, (call.__name__, message, kw, status)
    assert message.encode() in _lib.lib.emb_last_error(), (call.__name__, message, _lib.lib.emb_last_error())
  # the largest product that is taken passes the size check (and is refused for its null pointer)
  assert forward(rows=(1 << 31) // 16 - 1, post=None) == _lib.ERR_INVALID
  assert b'a pointer is null' in _lib.lib.emb_last_error()
  # rows = 0: nothing to do, nothing launched, whatever the device pointers are
  assert forward(rows=0) == _lib.OK and forward(rows=0, post=None, kl=None) == _lib.OK
  assert grad(rows=0) == _lib.OK and grad(rows=0, grad_post=None, grad_prior=None) == _lib.OK
  assert outs.onehot_kl_launches() == before
  assert raws['emb_onehot_kl_launches'](None) == _lib.ERR_INVALID
  with pytest.raises(ValueError, match='negative rows'):     # the same through the binding that raises
    _lib.api.emb_onehot_kl(x, x, _lib.F32, -1, 2, 8, 0.01, 1.0, x, x, x, x, x, None)


def test_facade_refuses_host_tensors_dtypes_and_mismatches():
  import embodied_amd as emb
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.OneHot(torch.zeros(3, 4, 8))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.rssm_kl(torch.zeros(3, 4, 8), torch.zeros(3, 4, 8))
  meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device='meta')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.OneHot(meta(3, 4, 8))


def test_path_decision():
  from embodied_amd import outs
  assert outs.ONEHOT_MAX_CLASSES == 256
  for classes in (1, 2, 24, 64, 96, 256):
    assert outs._kl_path(None, 16384, 32, classes) is True and outs._kl_path(True, 5, 1, classes) is True
    assert outs._kl_path(False, 5, 1, classes) is False
  assert outs._kl_path(None, 5, 2, 257) is False and outs._kl_path(False, 5, 2, 257) is False
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    outs._kl_path(True, 5, 2, 257)
  assert outs._kl_path(None, (1 << 31) // 2048, 32, 64) is False
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    outs._kl_path(True, (1 << 31) // 2048, 32, 64)
