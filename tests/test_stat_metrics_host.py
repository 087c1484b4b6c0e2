"""`emb_stat_rows`, `emb_mean_fill`, `scans.imag_metrics` and `outs.total_loss` as
far as they go without a GPU: the declarations and the binding, every refusal
(each one alone, all of them before any HIP call), both path decisions, the
composed paths on host tensors, the case table's conditions, the float64
restatement against what the reference's own `imag_loss` returned, and the
float32 definition against the bars.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import dreamer_target_cases as dcases
from tests import stat_metric_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'imag_metrics.npz'
TARGETS = ROOT / 'tests' / 'golden' / 'dreamer_targets.npz'
NAMES = ('emb_stat_rows', 'emb_stat_rows_launches', 'emb_mean_fill')


def _constant(name, text):
  return int(re.search(r'constexpr\s+\w+\s+%s\s*=\s*(\d+)' % name, text).group(1))


def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib
  from tests.test_abi_symbols import declared_symbols
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert 'dreamerv3/agent.py:424-442' in text and 'dreamerv3/agent.py:239-240' in text
  assert _lib.fast.SHAPES['emb_stat_rows'] == 'ints' and _lib.fast.SHAPES['emb_mean_fill'] == 'ints'
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'stat_rows.hip' in sources and 'stat_rows_abi.cpp' in sources
  # the export count: the header's comment, the README and the declarations agree
  count = len(declared_symbols())
  assert f'it exports ({count} functions)' in text
  assert f'the C ABI ({count} entry points' in (ROOT / 'README.md').read_text()
  # one set of constants: the public header, stat_rows.h, the binding, the case table
  assert int(re.search(r'#define\s+EMB_STAT_MAX_ENTRIES\s+(\d+)', text).group(1)) == _lib.STAT_MAX_ENTRIES
  assert int(re.search(r'#define\s+EMB_STAT_VALUES\s+(\d+)', text).group(1)) == _lib.STAT_VALUES == len(cases.COLUMNS)
  for name, value in (('NONE', cases.NONE), ('MUL_ADD', cases.MUL_ADD), ('SUB_DIV', cases.SUB_DIV)):
    assert int(re.search(r'#define\s+EMB_STAT_%s\s+(\d+)' % name, text).group(1)) == value == getattr(_lib, 'STAT_' + name)
  internal = (ROOT / 'embodied_amd' / 'csrc' / 'stat_rows.h').read_text()
  assert 'kStatMaxEntries = EMB_STAT_MAX_ENTRIES' in internal and cases.MAX_ENTRIES == _lib.STAT_MAX_ENTRIES
  assert _constant('kStatThreads', internal) == cases.THREADS and _constant('kStatVector', internal) == cases.VECTOR
  assert 'hip_runtime' not in internal.split('#ifndef EMB_STAT_ROWS_HOST_ONLY')[0]      # the check is plain C++
  assert C.sizeof(_lib.StatEntry) == 48 and C.sizeof(_lib.FillEntry) == 24
  assert cases.COUNTS[-1] == cases.THREADS * cases.VECTOR + 1


# -------------------------------------------------------------- refusals --

def _entry(lib, base, **fields):
  values = dict(x=base, affine=None, rows=3, cols=5, stride=6, mode=lib.STAT_NONE, weight=1.0)
  values.update(fields)
  return lib.StatEntry(**values)


STAT_REFUSALS = {
    'too many elements': ('more than 2^31 - 1 elements', dict(rows=1 << 16, cols=1 << 15, stride=1 << 15)),
    'too many elements, one row': ('more than 2^31 - 1 elements', dict(rows=1, cols=1 << 31, stride=1 << 31)),
    'too many elements, overflow': ('more than 2^31 - 1 elements', dict(rows=1 << 62, cols=1 << 62, stride=1 << 62)),
    'null x': ('a null address', dict(x=None)),
    'null affine, mul-add': ('a null address', dict(mode=1, affine=None)),
    'null affine, sub-div': ('a null address', dict(mode=2, affine=None)),
    'x off 4 bytes': ('an address off 4 bytes', dict(x=+2)),
    'x off 1 byte': ('an address off 4 bytes', dict(x=+1)),
    'affine off 4 bytes': ('an address off 4 bytes', dict(mode=2, affine=+2)),
    'stride < cols': ('stride < cols', dict(stride=4)),
    'stride 0': ('stride < cols', dict(stride=0)),
    'rows 0': ('rows or cols < 1', dict(rows=0)),
    'rows negative': ('rows or cols < 1', dict(rows=-1)),
    'cols 0': ('rows or cols < 1', dict(cols=0, stride=0)),
    'cols negative': ('rows or cols < 1', dict(cols=-3)),
    'unknown mode': ('an unknown affine mode', dict(mode=3)),
}


@pytest.mark.parametrize('which', sorted(STAT_REFUSALS))
def test_stat_rows_refuses_before_any_hip_call(which):
  """One thing wrong with one entry (the last of three): EMB_ERR_INVALID, the
  message, no launch.  The addresses are host memory: nothing dereferences them."""
  from embodied_amd import _lib
  message, fields = STAT_REFUSALS[which]
  fake = np.zeros(64, np.float32)
  base = fake.ctypes.data
  for name in ('x', 'affine'):
    if isinstance(fields.get(name), int):
      fields = dict(fields, **{name: base + fields[name]})
  raw = _lib.lib.emb_stat_rows
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_stat_rows'], C.c_int32
  table = (_lib.StatEntry * 3)(_entry(_lib, base), _entry(_lib, base, mode=2, affine=base + 8),
                               _entry(_lib, base, **fields))
  before = _lib.launches('stat_rows')
  status = raw(table, 3, C.c_void_p(base + 128), None, None)
  assert status == _lib.ERR_INVALID, (which, status)
  assert message.encode() in _lib.lib.emb_last_error(), (which, _lib.lib.emb_last_error())
  with pytest.raises(ValueError, match=re.escape(message)):          # the same through the call shim
    _lib.fast.emb_stat_rows(table, 3, base + 128, None, None)
  assert _lib.launches('stat_rows') == before


def test_stat_rows_refuses_bad_calls_and_launches_nothing_for_none():
  from embodied_amd import _lib
  fake = np.zeros(64, np.float32)
  base = fake.ctypes.data
  raw = _lib.lib.emb_stat_rows
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_stat_rows'], C.c_int32
  good = (_lib.StatEntry * 2)(_entry(_lib, base), _entry(_lib, base))
  many = (_lib.StatEntry * (_lib.STAT_MAX_ENTRIES + 1))(*[_entry(_lib, base)] * (_lib.STAT_MAX_ENTRIES + 1))
  out = C.c_void_p(base + 128)
  before = _lib.launches('stat_rows')
  refused = [
      ('outside 0 .. 2^31 - 1', (good, -1, out, None, None)),
      ('outside 0 .. 2^31 - 1', (good, 1 << 31, out, None, None)),
      ('a null address', (None, 2, out, None, None)),
      ('a null address', (good, 2, None, None, None)),
      ('an address off 4 bytes', (good, 2, C.c_void_p(base + 130), None, None)),
      ('an address off 4 bytes', (good, 2, out, C.c_void_p(base + 66), None)),
      ('a total needs all of its entries in one launch', (many, len(many), out, C.c_void_p(base + 64), None)),
  ]
  for message, call in refused:
    status = raw(*call)
    assert status == _lib.ERR_INVALID, (message, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert raw(good, 0, out, None, None) == _lib.OK and raw(None, 0, None, None, None) == _lib.OK
  assert _lib.launches('stat_rows') == before
  assert _lib.lib.emb_stat_rows_launches(None) == _lib.ERR_INVALID


MEAN_FILL_REFUSALS = {
    'n 0': ('less than 1 element', dict(n=0)),
    'n negative': ('less than 1 element', dict(n=-5)),
    'n too large': ('more than 2^31 - 1 elements', dict(n=1 << 31)),
    'null out': ('a null address', dict(out=None)),
    'out off 4 bytes': ('an address off 4 bytes', dict(out=+2)),
}


@pytest.mark.parametrize('which', sorted(MEAN_FILL_REFUSALS))
def test_mean_fill_refuses_before_any_hip_call(which):
  from embodied_amd import _lib
  message, fields = MEAN_FILL_REFUSALS[which]
  fake = np.zeros(64, np.float32)
  base = fake.ctypes.data
  if isinstance(fields.get('out'), int):
    fields = dict(fields, out=base + fields['out'])
  raw = _lib.lib.emb_mean_fill
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_mean_fill'], C.c_int32
  values = dict(out=base, n=8, scale=1.0, reserved=0)
  table = (_lib.FillEntry * 2)(_lib.FillEntry(**values), _lib.FillEntry(**{**values, **fields}))
  before = _lib.launches('stat_rows')
  assert raw(table, 2, C.c_void_p(base + 128), None) == _lib.ERR_INVALID
  assert message.encode() in _lib.lib.emb_last_error(), (which, _lib.lib.emb_last_error())
  good = (_lib.FillEntry * 1)(_lib.FillEntry(**values))
  for message, call in (('a null address', (good, 1, None, None)), ('a null address', (None, 1, C.c_void_p(base), None)),
                        ('an address off 4 bytes', (good, 1, C.c_void_p(base + 2), None)),
                        ('outside 0 .. 2^31 - 1', (good, -1, C.c_void_p(base), None))):
    assert raw(*call) == _lib.ERR_INVALID
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert raw(good, 0, None, None) == _lib.OK
  assert _lib.launches('stat_rows') == before


# ------------------------------------------------------- paths and facades --

def test_imag_metrics_path_decision():
  from embodied_amd import scans
  path = scans._imag_metrics_path
  assert path(None, True, True, 1024 * 16) is (1024 * 16 <= scans.IMAG_METRICS_FUSED_MAX)
  assert path(None, True, True, 16 * 16) is True
  assert path(True, True, True, 2 ** 31 - 1) is True and path(False, True, True, 256) is False
  assert path(None, False, True, 256) is False and path(None, True, False, 256) is False
  assert path(None, True, True, 2 ** 31) is False
  assert path(None, True, True, scans.IMAG_METRICS_FUSED_MAX + 1) is False
  with pytest.raises(ValueError, match=r'imag_metrics\(fused=True\): the kernel reads float32 CUDA tensors'):
    path(True, False, True, 256)
  with pytest.raises(ValueError, match=r'imag_metrics\(fused=True\): .*unit column stride.*fused=None or False'):
    path(True, True, False, 256)
  with pytest.raises(ValueError, match=r'fused=True\): an array of 2147483648 elements'):
    path(True, True, True, 2 ** 31)


def test_total_loss_path_decision():
  from embodied_amd import _lib, outs
  path = outs._total_loss_path
  k = _lib.STAT_MAX_ENTRIES
  assert path(None, True, True, 10, 1, 1024) is (1024 <= outs.TOTAL_LOSS_FUSED_MAX)
  assert path(None, True, True, 1, 1, 1) is True
  assert path(True, True, True, k, 1, 2 ** 31 - 1) is True and path(False, True, True, 3, 1, 64) is False
  for args in ((False, True, 3, 1, 64), (True, False, 3, 1, 64), (True, True, k + 1, 1, 64), (True, True, 3, 0, 64),
               (True, True, 3, 1, 2 ** 31), (True, True, 3, 1, outs.TOTAL_LOSS_FUSED_MAX + 1)):
    assert path(None, *args) is False, args
  for wording, args in (('float32 CUDA tensors', (False, True, 3, 1, 64)), ('contiguous tensors', (True, False, 3, 1, 64)),
                        (f'{k + 1} losses', (True, True, k + 1, 1, 64)), ('without elements', (True, True, 3, 0, 64)),
                        ('2147483648 elements', (True, True, 3, 1, 2 ** 31))):
    with pytest.raises(ValueError, match=r'total_loss\(fused=True\): .*%s.*fused=None or False' % wording):
      path(True, *args)


def test_facades_refuse_and_compose_on_host_tensors():
  """What the facades refuse whatever the path, and the composed paths -- the
  definition -- on host tensors against the float64 restatement."""
  import embodied_amd as emb
  from embodied_amd import ops, outs, scans
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ops.stat_rows([torch.zeros(4)])
  with pytest.raises(ValueError, match='no entries'):
    ops.stat_rows([])
  assert ops.stat_view(torch.zeros(3, 6)[:, :-1]) == (3, 5, 6) and ops.stat_view(torch.zeros(3, 6)) == (1, 18, 18)
  assert ops.stat_view(torch.zeros(6, 3).t()) is None and ops.stat_view(torch.zeros(2, 3, 4)[:, :, :-1]) is None
  # total_loss
  for count in cases.LOSS_COUNTS:
    losses, scales = cases.loss_inputs(count)
    tensors = {k: torch.from_numpy(v).requires_grad_() for k, v in losses.items()}
    loss, metrics = outs.total_loss(tensors, scales, fused=False)
    total, means, bar, grads = cases.total_loss64(losses, scales)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and list(metrics) == [f'loss/{k}' for k in losses]
    assert abs(float(loss.detach()) - total) <= bar
    loss.backward()
    for k, v in tensors.items():
      assert not metrics[f'loss/{k}'].requires_grad
      assert abs(float(metrics[f'loss/{k}']) - means[k]) <= cases.moment_bar(losses[k])
      np.testing.assert_allclose(v.grad.numpy(), np.full(v.shape, grads[k]), rtol=4 * 2.0 ** -24, atol=0)
    with pytest.raises(ValueError, match=r'fused=True\): the kernels read float32 CUDA tensors'):
      outs.total_loss(tensors, scales, fused=True)
  losses, scales = cases.loss_inputs(3)
  tensors = {k: torch.from_numpy(v) for k, v in losses.items()}
  with pytest.raises(ValueError, match='do not have the same keys'):
    outs.total_loss(tensors, {k: 1.0 for k in list(scales)[:2]})
  with pytest.raises(ValueError, match='do not have the same keys'):
    outs.total_loss(tensors, dict(scales, other=1.0))
  with pytest.raises(ValueError, match='no losses'):
    outs.total_loss({}, {})
  # imag_metrics
  inp = cases.imag_inputs(0, 0)
  N, T = inp['rew'].shape
  rng = np.random.default_rng(5)
  ret, adv = (rng.standard_normal((N, T - 1)).astype(np.float32) for _ in range(2))
  weight, tar = (rng.standard_normal((N, T)).astype(np.float32) for _ in range(2))
  t = lambda a: torch.from_numpy(a)
  targets = scans.DreamerTargets(t(ret), t(weight), t(adv), t(adv), t(tar))
  ents = {k: t(inp[f'ent_{k}']) for k in cases.KEYS}
  none = emb.DeviceNormalize('none')
  args = (targets, t(inp['rew']), t(inp['con']), t(inp['pred']), t(inp['slow']), none)
  got = scans.imag_metrics(*args, vstats=(0.25, 1.5), ents=ents, entlimits=cases.ENTLIMITS, fused=False)
  want, bars = cases.imag_metrics64(inp['rew'], inp['con'], inp['pred'], inp['slow'], ret, adv, weight, tar, (0.0, 1.0),
                                    (0.25, 1.5), {k: inp[f'ent_{k}'] for k in cases.KEYS}, cases.ENTLIMITS)
  assert list(got) == list(cases.METRICS)
  for name in cases.METRICS:
    assert got[name].dtype == torch.float32 and got[name].dim() == 0, name
    assert abs(float(got[name]) - want[name]) <= bars[name], (name, float(got[name]), want[name])
  assert list(scans.imag_metrics(*args, fused=False)) == list(scans.IMAG_METRICS)
  with pytest.raises(ValueError, match=r'fused=True\): the kernel reads float32 CUDA tensors'):
    scans.imag_metrics(*args, fused=True)
  with pytest.raises(ValueError, match='entlimits'):
    scans.imag_metrics(*args, ents=ents, entlimits={'other': (0.0, 1.0)})
  for fused in (None, False, True):
    one = scans.DreamerTargets(t(ret[:, :0]), t(weight[:, :1]), t(adv[:, :0]), t(adv[:, :0]), t(tar[:, :1]))
    with pytest.raises(ValueError, match=r'needs N >= 1 and T >= 2'):
      scans.imag_metrics(one, *(x[:, :1] for x in args[1:5]), none, fused=fused)
    empty = scans.DreamerTargets(t(ret[:0]), t(weight[:0]), t(adv[:0]), t(adv[:0]), t(tar[:0]))
    with pytest.raises(ValueError, match=r'needs N >= 1 and T >= 2'):
      scans.imag_metrics(empty, *(x[:0] for x in args[1:5]), none, fused=fused)
  for doc in (scans.imag_metrics.__doc__, outs.total_loss.__doc__):
    assert 'composed' in doc and 'fused' in doc
  assert 'CLONE' in scans.imag_metrics.__doc__ and 'until the next call' in scans.imag_metrics.__doc__


# ------------------------------------------------- case table and fixture --

def _stat_entries():
  """Every (tag, x') the GPU test holds to the moment bars, and its element count."""
  for n in cases.COUNTS:
    for mode, (offset, scale) in cases.AFFINE.items():
      yield f'count {n} mode {mode}', cases.affine32(cases.stat_data('count', n), mode, offset, scale)
      yield f'edge {n} mode {mode}', cases.affine32(cases.edge_data(n, mode)[0], mode, offset, scale)
  for rows, cols, width in cases.VIEWS:
    yield f'view {rows}x{cols}', cases.stat_data('view', rows * width).reshape(rows, width)[:, :cols]
  for offset in cases.OFFSETS:
    yield f'offset {offset}', cases.stat_data('offset', cases.OFFSET_COUNT + offset)[offset:]
  for count in cases.LAUNCH_COUNTS:
    for index in range(count):
      yield f'launch {count}/{index}', cases.stat_data('launch', 33 + index, seed=count)


def test_case_table_conditions():
  """std >= 0.1 |mean| in every entry whose std is held to a bar (one element has
  std 0: the GPU test holds it exactly, not to the bar); n <= 16 384 in every
  entry whose rate is compared."""
  for tag, xp in _stat_entries():
    assert xp.size <= 16384, tag
    if xp.size > 1:
      mean, std = cases.stats64(xp)[:2]
      assert std >= 0.1 * abs(mean), (tag, mean, std)
  for n in cases.COUNTS:
    for mode in cases.AFFINE:
      x, ones, below = cases.edge_data(n, mode)
      xp = cases.affine32(x, mode, *cases.AFFINE[mode])
      assert (np.abs(xp) == 1.0).sum() >= ones and (np.abs(xp) == np.nextafter(np.float32(1), np.float32(0))).sum() >= below
      if n >= 64:
        assert ones >= 2 and below >= 2, (n, mode, ones, below)
  with np.load(TARGETS) as f:
    for case, (source, c) in enumerate(cases.IMAG_CASES):
      N, T = c.shape
      assert N * (T - 1) <= 16384, c.shape                                     # ret_rate
      if source is not None:
        for adv in f[f'adv_{dcases.tag(source)}']:
          mean, std = cases.stats64(adv)[:2]
          assert std >= 0.1 * abs(mean), (c.shape, mean, std)                   # adv_std
  shapes = [c.shape for _, c in cases.IMAG_CASES]
  assert (1024, 16) in shapes and (16, 16) in shapes


def test_fixture_inputs_match_their_digests():
  with np.load(GOLDEN) as f:
    assert int(f['steps']) == cases.STEPS and tuple(f['names']) == cases.METRICS
    for case, (source, c) in enumerate(cases.IMAG_CASES):
      name = cases.imag_tag(case)
      for step in range(cases.STEPS):
        inp = cases.imag_inputs(case, step)
        assert all(v.shape == c.shape and v.dtype == np.float32 for v in inp.values())
        assert np.array_equal(f[f'in_{name}'][step], cases.digest(inp)), (name, step)
        assert all(np.abs(inp[f'ent_{k}']).min() > 0 for k in cases.KEYS)
        if source is not None:
          same = dcases.inputs(source, step)
          assert all(np.array_equal(inp[k], same[k]) for k in same)
      assert f[f'metrics_{name}'].shape == (cases.STEPS, len(cases.METRICS))
      assert f[f'metrics_{name}'].dtype == np.float32 and np.isfinite(f[f'metrics_{name}']).all()
      assert f[f'vstats_{name}'].shape == f[f'rstats_{name}'].shape == (cases.STEPS, 2)
      if c.valnorm[0] == 'none':
        assert np.array_equal(f[f'vstats_{name}'], np.tile([0.0, 1.0], (cases.STEPS, 1)))
    assert not any(f[key].dtype == object for key in f.files)
  assert GOLDEN.stat().st_size < 100_000


def test_restatement_agrees_with_the_reference():
  """`imag_metrics64` over the arrays the reference's `imag_loss` held (the
  dreamer_targets fixture has them for the cases the two tables share) against the
  metrics the same function returned: the moments at the bar, min, max and rate
  bit for bit.  The reference sums in float32: what is printed is the worst
  share of the bar that this costs."""
  worst = {}
  with np.load(GOLDEN) as f, np.load(TARGETS) as t:
    for case, (source, c) in enumerate(cases.IMAG_CASES):
      if source is None:
        continue
      name, theirs = cases.imag_tag(case), dcases.tag(source)
      for step in range(cases.STEPS):
        inp = cases.imag_inputs(case, step)
        assert np.array_equal(t[f'stats_{theirs}'][step][:2], f[f'rstats_{name}'][step])      # one retnorm, two fixtures
        want, bars = cases.imag_metrics64(
            inp['rew'], inp['con'], inp['pred'], inp['slow'], t[f'ret_{theirs}'][step], t[f'adv_{theirs}'][step],
            t[f'weight_{theirs}'][step], t[f'tarpadded_{theirs}'][step], f[f'rstats_{name}'][step],
            f[f'vstats_{name}'][step], {k: inp[f'ent_{k}'] for k in cases.KEYS}, cases.ENTLIMITS)
        for index, metric in enumerate(cases.METRICS):
          got = f[f'metrics_{name}'][step][index]
          if bars[metric] == 0.0:
            assert np.float32(want[metric]) == got, (name, step, metric, want[metric], got)
          else:
            share = abs(float(got) - want[metric]) / bars[metric]
            worst[metric] = max(worst.get(metric, 0.0), share)
            assert share <= 1.0, (name, step, metric, float(got), want[metric], share)
  print('imag_loss metrics, the reference (float32 sums) against the float64 restatement, worst share of the bar: '
        + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))


def test_float32_definition_stays_inside_the_bars():
  """The float32 definition (numpy's pairwise float32 sums) of every entry of the
  case table against the float64 restatement: the worst share of the bars."""
  worst = dict.fromkeys(cases.COLUMNS[:3], 0.0)
  for tag, xp in _stat_entries():
    got, want, bar = cases.stats32(xp), cases.stats64(xp), cases.moment_bar(xp)
    for index, column in enumerate(cases.COLUMNS[:3]):
      share = abs(got[index] - want[index]) / bar
      worst[column] = max(worst[column], share)
      assert share <= 1.0, (tag, column, got[index], want[index])
    assert np.array_equal(got[3:], want[3:])
  for count in cases.LOSS_COUNTS:
    losses, scales = cases.loss_inputs(count)
    total, _, bar, _ = cases.total_loss64(losses, scales)
    share = abs(float(cases.total_loss32(losses, scales)) - total) / bar
    worst['total'] = max(worst.get('total', 0.0), share)
    assert share <= 1.0, (count, share)
  print('float32 definition against the float64 restatement, worst share of the bar: '
        + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'dreamerv3' / 'agent.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_imag_metrics', ROOT / 'tools' / 'gen_imag_metrics_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key
