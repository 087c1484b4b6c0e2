"""`embodied_amd.outs` and `emb_twohot_*` as far as they go without a GPU: the
bins, the fixture, the declarations and the binding, the refusals that happen
before any launch.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import twohot_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'twohot.npz'
EDGES = ROOT / 'tests' / 'golden' / 'twohot_edges.npz'
NAMES = ('emb_twohot_stats', 'emb_twohot_loss', 'emb_twohot_grad', 'emb_twohot_launches')


def test_bins_equal_the_fixture_bit_for_bit():
  from embodied_amd import outs
  with np.load(GOLDEN) as f:
    for n in cases.BINS:
      bins = outs.symexp_twohot_bins(n)
      assert bins.dtype == np.float32 and bins.shape == (n,)
      assert bins.tobytes() == f[f'bins_{n}'].tobytes(), n
      assert np.array_equal(bins, -bins[::-1]) or n == 1, n      # antisymmetric (one bin: the lowest alone)
      assert np.all(np.diff(bins) >= 0)
  assert np.array_equal(outs.symexp_twohot_bins(), outs.symexp_twohot_bins(255))
  b255, b256 = outs.symexp_twohot_bins(255), outs.symexp_twohot_bins(256)
  assert b255[127] == 0.0 and not np.signbit(b255[127]) and np.all(np.diff(b255) > 0)
  # an even n has the reference's two zeros side by side (heads.py:141-143): the only tie
  assert b256[127] == 0.0 and b256[128] == 0.0 and (np.diff(b256) > 0).sum() == 254
  assert b255[0] == b256[0] == -np.expm1(np.float32(20)) and b255[-1] == -b255[0]
  with pytest.raises(ValueError):
    outs.symexp_twohot_bins(0)


def test_fixture_inputs_match_their_digests_and_the_restatement():
  """The fixture belongs to `cases.inputs`; `cases.reference64` (what the GPU tests
  use for other shapes) agrees with the reference's own float64 run on every case;
  and the reference's float32 run sits inside both bars of the GPU tests."""
  with np.load(GOLDEN) as f:
    assert tuple(f['twohot_lines']) == (273, 330) and tuple(f['head_lines']) == (132, 144)
    for case, c in enumerate(cases.CASES):
      name, bins = cases.tag(case), f[f'bins_{c.n}']
      inp = cases.inputs(case, bins)
      assert np.array_equal(f[f'in_{name}'], cases.digest(inp)), name
      targets = [inp[f'target{k}'] for k in range(cases.TARGETS)]
      assert np.isposinf(targets[0][-3]) and np.isneginf(targets[0][-2]) and np.isnan(targets[0][-1])
      assert np.isfinite(targets[1]).all()
      outside = np.abs(targets[1]) > bins[-1]
      assert c.rows < 100 or (outside.any() and np.isin(targets[1], bins).sum() >= c.rows // 2)
      pred64, loss64 = f[f'pred64_{name}'], f[f'loss64_{name}']
      assert pred64.shape == (c.rows,) and loss64.shape == (cases.TARGETS, c.rows)
      assert pred64.dtype == loss64.dtype == np.float64
      ref = cases.reference64(inp['logits'], bins, targets)
      assert np.all(np.abs(ref['pred'] - pred64) <= 1e-12 * (1 + ref['scale'])), name
      assert np.allclose(np.stack(ref['loss']), loss64, rtol=1e-12, atol=1e-12, equal_nan=True), name
      assert np.isnan(loss64[0, -1]) == (c.n > 1), name       # one bin: both indices 0, the target drops out
      assert np.isfinite(np.delete(loss64.reshape(-1), c.rows - 1)).all(), name
      assert np.all(np.abs(f[f'pred_{name}'] - pred64) <= 1e-5 * (1 + ref['scale'])), name
      assert np.allclose(f[f'loss_{name}'], loss64, rtol=1e-5, atol=1e-5, equal_nan=True), name
      if c.kind == 'zero' and c.n > 1:
        assert not f[f'pred_{name}'].any(), name               # what the symmetric sum is for
  assert GOLDEN.stat().st_size < 900_000


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_twohot', ROOT / 'tools' / 'gen_twohot_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  for path, fresh in ((GOLDEN, tool.generate()), (EDGES, tool.generate_edges())):
    with np.load(path) as f:
      assert sorted(f.files) == sorted(fresh)
      for key in f.files:
        assert np.array_equal(f[key], fresh[key], equal_nan=f[key].dtype.kind == 'f'), (path.name, key)


def test_edges_fixture_matches_its_digests_and_the_restatement():
  """`cases.reference64` against the reference's own float64 run where the first
  fixture does not reach: bins that are not the symexp set (asymmetric, runs of
  equal neighbours, equal outer bins), the zeros / denormals / outer bins of the
  even symexp set as targets, and logits with -inf, +inf, NaN and |x| up to 1e4.
  The bars of the test above; NaN and +-inf where and only where the class has them."""
  from embodied_amd import outs
  with np.load(EDGES) as f:
    assert tuple(f['twohot_lines']) == (273, 330)
    assert f['bins_symexp64'].tobytes() == outs.symexp_twohot_bins(64).tobytes()
    seen = set()
    for case, c in enumerate(cases.EDGE_CASES):
      name = cases.edge_tag(case)
      bins = cases.edge_bins(c.bins, c.n, outs.symexp_twohot_bins)
      assert bins.tobytes() == f[f'bins_{c.bins}{c.n}'].tobytes(), name
      assert np.array_equal(outs._host_bins(bins, c.n), bins)             # what the facade takes
      inp = cases.edge_inputs(case, bins)
      assert np.array_equal(f[f'in_{name}'], cases.digest(inp)), name
      targets = [inp[f'target{k}'] for k in range(cases.EDGE_TARGETS)]
      pred64, loss64 = f[f'pred64_{name}'], f[f'loss64_{name}']
      assert pred64.shape == (cases.EDGE_ROWS,) and loss64.shape == (cases.EDGE_TARGETS, cases.EDGE_ROWS)
      assert pred64.dtype == loss64.dtype == np.float64
      ref = cases.reference64(inp['logits'], bins, targets)
      loss = np.stack(ref['loss'])
      assert np.array_equal(np.isnan(ref['pred']), np.isnan(pred64)), name
      assert np.array_equal(np.isnan(loss), np.isnan(loss64)), name
      assert np.array_equal(np.isposinf(loss), np.isposinf(loss64)) and not np.isneginf(loss64).any(), name
      ok = ~np.isnan(pred64)
      assert np.all(np.abs(ref['pred'] - pred64)[ok] <= 1e-12 * (1 + ref['scale'][ok])), name
      assert np.allclose(loss, loss64, rtol=1e-12, atol=1e-12, equal_nan=True), name
      # the two-bin sum is the definition wherever the row's logits are finite
      finite = np.isfinite(inp['logits']).all(-1)
      assert np.allclose(np.stack(ref['loss2'])[:, finite], loss64[:, finite], rtol=1e-12, atol=1e-12), name
      if c.logits == 'normal':
        assert np.isfinite(pred64).all() and np.isfinite(loss64).all(), name
      else:
        kinds = np.array(cases.EDGE_KINDS)[np.arange(cases.EDGE_ROWS) % len(cases.EDGE_KINDS)]
        assert np.isnan(pred64[np.isin(kinds, ('all_ninf', 'pinf', 'nan'))]).all(), name
        assert np.isfinite(pred64[~np.isin(kinds, ('all_ninf', 'pinf', 'nan'))]).all(), name
        assert np.isfinite(loss64[:, np.isin(kinds, ('finite', 'big'))]).all(), name
        # a -inf logit: +inf under a weight, NaN (0 * -inf) under none -- never finite for n > 2
        assert not np.isfinite(loss64[:, np.isin(kinds, ('ninf_below', 'ninf_above', 'ninf_else'))]).any(), name
        assert np.isposinf(loss64[0, kinds == 'ninf_below']).all() and np.isnan(loss64[0, kinds == 'ninf_else']).all(), name
        seen |= {(k, 'inf' if np.isposinf(v) else 'nan') for k, v in zip(kinds, loss64[0]) if k == 'ninf_above'}
      if c.bins == 'ties':
        assert (np.diff(bins) == 0).sum() >= 4 and bins[0] == bins[1] and bins[-1] == bins[-2], name
        assert any(np.isin(t, bins[np.r_[np.diff(bins) == 0, False]]).any() for t in targets), name
      if c.bins == 'symexp':
        assert np.array_equal(targets[0][:6].view(np.uint32),
                              np.array([0.0, -0.0, cases.DENORMAL, -cases.DENORMAL, bins[-1], bins[0]], np.float32).view(np.uint32))
    assert ('ninf_above', 'inf') in seen
  assert EDGES.stat().st_size < 100_000


def test_float32_restatement_sits_inside_the_bars_of_three_and_four_targets():
  """The bars of `test_three_and_four_targets` come from the sums' condition
  scales, not from the kernels: float32 numpy over the same seeds must fit."""
  from tests import test_gpu_twohot as device
  worst = [0.0, 0.0]
  for k in (3, 4):
    for rows, n in ((5, 63), (67, 255), (1025, 2)):
      for kind in ('f32', 'bf16'):
        d = device._multi(n, rows, kind)
        coefs = device.COEFS4[:k]
        loss, grad = cases.composed32(d['logits'], d['bins'], d['targets'][:k], coefs, d['gout'])
        want_loss, loss_bar, want_grad, grad_bar = device._sum_bars(d['ref'], coefs, d['gout'])
        worst[0] = max(worst[0], device._match(loss, want_loss, loss_bar))
        worst[1] = max(worst[1], device._match(grad, want_grad, grad_bar))
  print(f'float32 numpy, three and four targets: loss {worst[0]:.3g}, grad {worst[1]:.3g} of their bars')
  assert max(worst) <= 1.0, worst


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'embodied/jax/outs.py:273-330' in text and 'embodied/jax/heads.py:132-144' in text
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [8, 11, 12, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'twohot.hip' in sources and 'twohot_abi.cpp' in sources
  assert emb.TwoHot is emb.outs.TwoHot and emb.symexp_twohot_bins is emb.outs.symexp_twohot_bins
  assert emb.twohot_launches() == emb.outs.twohot_launches()


def test_refusals_before_any_launch():
  from embodied_amd import _lib
  from embodied_amd import outs
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  ptrs = (C.c_void_p * 4)(*([fake.ctypes.data] * 4))
  coefs = (C.c_float * 4)(1.0, 0.7, 0.5, 0.25)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def stats(logits=x, dtype=_lib.F32, rows=4, n=8, bins=x, lse=x, pred=x):
    return raws['emb_twohot_stats'](logits, dtype, rows, n, bins, lse, pred, None)

  def loss(logits=x, dtype=_lib.F32, rows=4, n=8, bins=x, lse=x, targets=ptrs, coefs=coefs, k=2, out=x):
    return raws['emb_twohot_loss'](logits, dtype, rows, n, bins, lse, targets, coefs, k, out, None)

  def grad(logits=x, dtype=_lib.BF16, rows=4, n=8, bins=x, lse=x, targets=ptrs, coefs=coefs, k=2, gout=x, out=x):
    return raws['emb_twohot_grad'](logits, dtype, rows, n, bins, lse, targets, coefs, k, gout, out, None)

  before = outs.twohot_launches()
  shape = [('negative rows', dict(rows=-1)), ('n outside 1 .. 1024', dict(n=0)), ('n outside 1 .. 1024', dict(n=-5)),
           ('n outside 1 .. 1024', dict(n=1025)), ('more than 2^31 - 1', dict(rows=(1 << 31) // 8, n=8)),
           ('more than 2^31 - 1', dict(rows=1 << 62, n=1024)),
           ('dtype must be', dict(dtype=_lib.F16)), ('dtype must be', dict(dtype=_lib.F64)), ('dtype must be', dict(dtype=-1))]
  refused = []
  for call in (stats, loss, grad):
    refused += [(call, message, kw) for message, kw in shape]
    refused += [(call, 'a pointer is null', {key: None}) for key in ('logits', 'bins', 'lse')]
  refused += [(stats, 'a pointer is null', dict(pred=None)), (loss, 'a pointer is null', dict(out=None)),
              (grad, 'a pointer is null', dict(out=None)), (grad, 'a pointer is null', dict(gout=None))]
  one_null = (C.c_void_p * 4)(fake.ctypes.data, None, fake.ctypes.data, fake.ctypes.data)
  for call in (loss, grad):
    refused += [(call, 'k outside 1 .. 4', dict(k=0)), (call, 'k outside 1 .. 4', dict(k=5)),
                (call, 'k outside 1 .. 4', dict(k=-1)), (call, 'k outside 1 .. 4', dict(k=5, rows=0)),
                (call, 'targets or the coefs array is null', dict(targets=None)),
                (call, 'targets or the coefs array is null', dict(coefs=None)),
                (call, 'a target is null', dict(targets=one_null))]
  for call, message, kw in refused:
    status = call(**kw)
    assert status == _lib.ERR_INVALID, (call.__name__, message, kw, status)
    assert message.encode() in _lib.lib.emb_last_error(), (call.__name__, message, _lib.lib.emb_last_error())
  # the largest product that is taken passes the size check (and is refused for its null pointer)
  assert stats(rows=(1 << 31) // 8 - 1, n=8, logits=None) == _lib.ERR_INVALID
  assert b'a pointer is null' in _lib.lib.emb_last_error()
  # rows = 0: nothing to do, nothing launched, whatever the device pointers are
  assert stats(rows=0) == _lib.OK and stats(rows=0, logits=None, lse=None, pred=None) == _lib.OK
  assert loss(rows=0) == _lib.OK and loss(rows=0, logits=None, out=None, targets=one_null) == _lib.OK
  assert grad(rows=0) == _lib.OK and grad(rows=0, gout=None, out=None) == _lib.OK
  assert outs.twohot_launches() == before
  assert raws['emb_twohot_launches'](None) == _lib.ERR_INVALID
  with pytest.raises(ValueError, match='negative rows'):     # the same through the binding that raises
    _lib.api.emb_twohot_stats(x, _lib.F32, -1, 8, x, x, x, None)


def test_facade_refuses_host_tensors_bad_bins_and_too_many_targets():
  import embodied_amd as emb
  from embodied_amd import outs
  bins = emb.symexp_twohot_bins(255)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.TwoHot(torch.zeros(3, 255), bins)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.TwoHot(torch.zeros(3, 256), emb.symexp_twohot_bins(256))       # the reference's two zeros are bins
  swapped = bins.copy()
  swapped[[10, 11]] = swapped[[11, 10]]
  for bad in (bins[::-1].copy(), swapped, np.where(np.arange(255) == 7, np.nan, bins).astype(np.float32),
              np.where(np.arange(255) == 254, np.inf, bins).astype(np.float32), torch.from_numpy(swapped)):
    with pytest.raises(ValueError, match='bins must be finite and increasing'):
      emb.TwoHot(torch.zeros(3, 255), bad)
  with pytest.raises(ValueError, match='bins must be float32'):
    emb.TwoHot(torch.zeros(3, 255), bins.astype(np.float64))
  with pytest.raises(ValueError, match='255 logits per row need 255 bins'):
    emb.TwoHot(torch.zeros(3, 255), bins[:-1])
  t = torch.zeros(3)
  assert outs._check_sum([t] * 4, [1, 2, 3, 4]) == ((t,) * 4, (1.0, 2.0, 3.0, 4.0))
  with pytest.raises(ValueError, match=r'5 targets, one launch takes 1 \.\. 4'):
    outs._check_sum([t] * 5, [1.0] * 5)
  with pytest.raises(ValueError, match='0 targets'):
    outs._check_sum([], [])
  with pytest.raises(ValueError, match='2 targets and 1 coefs'):
    outs._check_sum([t, t], [1.0])


def test_path_decision():
  from embodied_amd import outs
  assert outs.TWOHOT_MAX_BINS == 1024 and outs.TWOHOT_MAX_TARGETS == 4
  for n in (1, 255, 256, 1024):
    assert outs._path(None, n, 16384) is True and outs._path(True, n, 5) is True
    assert outs._path(False, n, 5) is False
  assert outs._path(None, 1025, 5) is False and outs._path(False, 1025, 5) is False
  with pytest.raises(ValueError, match=r'fused=True.*1025 bins.*at most 1024'):
    outs._path(True, 1025, 5)
  assert outs._path(None, 1024, (1 << 31) // 1024) is False
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1'):
    outs._path(True, 1024, (1 << 31) // 1024)
