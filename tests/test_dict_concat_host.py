"""`emb_dict_concat`, `nets.DictConcat` and `Space.classes` as far as they go
without a GPU: the numpy restatement against what the reference's own
`DictConcat` returned, the declarations and the binding, every refusal of the
table check (all of them before any HIP call), the facade's own refusals and its
path decision, and the GPU sweep's shapes against the grid cap and the packing
ladder as csrc/dict_concat.h spells them.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from embodied_amd.space import Space
from tests import dict_concat_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'dict_concat.npz'
NAMES = ('emb_dict_concat', 'emb_dict_concat_launches')
K = cases.header_constants()


# ------------------------------------------------------------------ fixture --

def test_fixture_inputs_match_their_digests_and_cite_the_reference():
  with np.load(GOLDEN) as f:
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      assert np.array_equal(f[f'in_{name}'], cases.digest(cases.inputs(case))), name
      shape = (c.rows, cases.width_of(c.keys))
      assert f[f'out_{name}'].shape == f[f'out64_{name}'].shape == shape
      assert f[f'out_{name}'].dtype == np.float32 and f[f'out64_{name}'].dtype == np.float64
    assert tuple(f['lines_DictConcat']) == (467, 500) and tuple(f['lines_available']) == (80, 99)
    assert tuple(f['lines_symlog']) == (59, 60) and tuple(f['lines_mask']) == (76, 77) and tuple(f['lines_where']) == (67, 73)
    assert tuple(f['lines_rssm_mask']) == (76, 79) and tuple(f['lines_rssm_clamp']) == (137, 137)
    assert not any(f[key].dtype == object for key in f.files)
  assert GOLDEN.stat().st_size < 100_000
  # what the cases are there for
  names = [c.name for c in cases.CASES]
  assert len(set(names)) == len(names)
  feeds = {k.feed for c in cases.CASES for k in c.keys}
  assert feeds == {'float32', 'bf16', 'int32', 'int64', 'uint8', 'bool'}
  assert any(c.reset and c.unit for c in cases.CASES) and any(c.squish == 'symlog' for c in cases.CASES)


@pytest.mark.parametrize('case', range(len(cases.CASES)))
def test_restatement_agrees_with_the_reference(case):
  """Identity, one-hot, masks and clamp bit for bit in both precisions; symlog
  under the bar against the reference's float64 run."""
  c, name = cases.CASES[case], cases.tag(case)
  inp = cases.inputs(case)
  with np.load(GOLDEN) as f:
    got32 = cases.restate(c.keys, inp, c.squish, c.unit, np.float32)
    got64 = cases.restate(c.keys, inp, c.squish, c.unit, np.float64)
    assert got32.dtype == np.float32 and got64.dtype == np.float64
    if c.squish is None:
      assert np.array_equal(got32, f[f'out_{name}'], equal_nan=True)
      assert np.array_equal(got64, f[f'out64_{name}'], equal_nan=True)
    else:
      worst = cases.ulps(got32, f[f'out64_{name}']).max()
      print(f'{name}: the float32 restatement, worst {worst:.4f} float32 ulp of the float64 value (bar {cases.SYMLOG_BAR_ULP})')
      assert worst <= cases.SYMLOG_BAR_ULP
      assert cases.ulps(got64, f[f'out64_{name}']).max() == 0.0
    # the holes are where the table says: an unavailable row of a key is zeros in that key's span only
    assert np.isnan(got32).sum() == np.isnan(f[f'out_{name}']).sum() > 0 or c.name == 'disc18'


def test_the_bar_is_the_measured_one():
  """Twice the reference's own float32 error over the fixture, not less than one ulp."""
  with np.load(GOLDEN) as f:
    worst = max(cases.ulps(f[f'out_{cases.tag(i)}'], f[f'out64_{cases.tag(i)}']).max()
                for i, c in enumerate(cases.CASES) if c.squish == 'symlog')
  assert abs(worst - cases.SYMLOG_REFERENCE_ULP) < 5e-5, worst
  assert cases.SYMLOG_BAR_ULP == max(2 * cases.SYMLOG_REFERENCE_ULP, 1.0)
  text = (ROOT / 'profiles' / 'dict_concat_accuracy.txt').read_text()
  assert f'{cases.SYMLOG_REFERENCE_ULP:.4f}' in text and f'{cases.SYMLOG_BAR_ULP:.4f}' in text


def test_stored_is_round_then_divide():
  v = np.array([0.5, -0.5, 1.0, -1.0, 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 1.004, -1.004, 1.002, -1.002, 1e4, -1e4, 0.0, 0.3337], np.float32)
  for bf16 in (False, True):
    want = cases.stored(v, bf16, unit=True)
    # divide-then-round, the kernel's order: the same bits for every finite value
    first = (v / np.maximum(np.float32(1), np.abs(v))).astype(np.float32)
    first = cases.bf16_round(first) if bf16 else first
    assert np.array_equal(want.view(np.uint32), first.view(np.uint32))
  # 1.004 rounds up to 1 + 2^-7 in bfloat16 and 1.002 down to 1: either way the clamp stores 1
  assert cases.bf16_round(np.float32(1.004)) == 1.0078125 and cases.bf16_round(np.float32(1.002)) == 1.0
  assert cases.stored(np.float32(1.004), True, unit=True) == 1.0 == cases.stored(np.float32(1.002), True, unit=True)


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'embodied' / 'jax' / 'nets.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_dict_concat', ROOT / 'tools' / 'gen_dict_concat_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key], equal_nan=f[key].dtype.kind == 'f'), key


# ------------------------------------------------------------ Space.classes --

def test_space_classes():
  assert Space(np.int32, (), 0, 18).classes == 18 and isinstance(Space(np.int32, (), 0, 18).classes, int)
  assert Space(np.int64, (), 2, 7).classes == 5
  assert Space(bool).classes == 2 and isinstance(Space(bool).classes, int)
  assert Space(np.uint8, (), 0, 255).classes == 255
  shaped = Space(np.int32, (2, 3), 0, 4).classes
  assert shaped.shape == (2, 3) and (shaped == 4).all()
  mixed = Space(np.int32, (3,), 0, np.array([2, 3, 4])).classes
  assert mixed.tolist() == [2, 3, 4]
  assert (Space(bool, (4,)).classes == 2).all() and Space(bool, (4,)).classes.shape == (4,)
  for space in (Space(np.float32, (3,)), Space(np.float64)):
    with pytest.raises(AssertionError):
      space.classes
  # high is exclusive, as `sample` treats it
  space = Space(np.int32, (1000,), 0, 3)
  assert space.sample().max() == 2 == space.classes[0] - 1


# ------------------------------------------------------ header and binding --

def test_header_declares_and_binding_covers_the_new_symbols():
  from embodied_amd import _lib, nets
  from tests.test_abi_symbols import declared_symbols
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  for cited in ('embodied/jax/nets.py:467-500', 'embodied/jax/nets.py:80-99', 'dreamerv3/rssm.py:76-79',
                'dreamerv3/rssm.py:137', 'dreamerv3/rssm.py:216-220', 'dreamerv3/rssm.py:97'):
    assert cited in text, cited
  assert _lib.fast.SHAPES['emb_dict_concat'] == 'ints'
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'dict_concat.hip' in sources and 'dict_concat_abi.cpp' in sources
  count = len(declared_symbols())
  assert count == 169 and f'it exports ({count} functions)' in text
  assert f'the C ABI ({count} entry points' in (ROOT / 'README.md').read_text()
  for name in ('ONEHOT', 'NONE', 'SYMLOG', 'MAX_KEYS'):
    assert int(re.search(r'#define\s+EMB_DICT_%s\s+(\d+)' % name, text).group(1)) == getattr(_lib, 'DICT_' + name)
  internal = (ROOT / 'embodied_amd' / 'csrc' / 'dict_concat.h').read_text()
  assert 'kDictMaxKeys = EMB_DICT_MAX_KEYS' in internal
  assert 'hip_runtime' not in internal.split('#ifndef EMB_DICT_CONCAT_HOST_ONLY')[0]      # the check is plain C++
  assert C.sizeof(_lib.DictEntry) == 32
  assert (nets.DICT_MAX_KEYS, nets.DICT_MAX_WIDTH, nets.DICT_MAX_CLASSES) == (16, K['max_width'], K['max_classes']) == (16, 16384, 16384)
  assert nets.dict_concat_launches() == _lib.launches('dict_concat')


# ---------------------------------------------------------------- refusals --

def _table(lib, base, *entries):
  """Entries as dicts; defaults: a float32 key of 4 elements.  `first` None: behind the one before."""
  table, first = (lib.DictEntry * max(len(entries), 1))(), 0
  for entry, fields in zip(table, entries):
    values = dict(x=base, dtype=lib.F32, kind=lib.DICT_NONE, elements=4, classes=0, first=None)
    values.update(fields)
    if values['first'] is None:
      values['first'] = first
    for name, value in values.items():
      setattr(entry, name, value)
    first = values['first'] + (values['elements'] * values['classes'] if values['kind'] == lib.DICT_ONEHOT else values['elements'])
  return table


def _raw(lib):
  raw = lib.lib.emb_dict_concat
  raw.argtypes, raw.restype = lib.SIGNATURES['emb_dict_concat'], C.c_int32
  return raw


# message, the entries, then (count, rows, width, out offset, stride, dtype) overrides
ONEHOT = dict(dtype=3, kind=0, elements=2, classes=5)          # EMB_I32, EMB_DICT_ONEHOT
REFUSALS = {
    'spans overlap': ('the spans overlap', [dict(), dict(first=3)], dict(width=7)),
    'spans overlap, same first': ('the spans overlap', [dict(), dict(first=0)], dict(width=4)),
    'a gap between spans': ('the spans do not tile [0, width)', [dict(), dict(first=5)], dict(width=9)),
    'a gap in front': ('the spans do not tile [0, width)', [dict(first=1)], dict(width=5)),
    'short of width': ('the spans do not tile [0, width)', [dict(), dict()], dict(width=9)),
    'past width': ('the spans do not tile [0, width)', [dict(), dict()], dict(width=7)),
    'negative first': ('the spans overlap', [dict(first=-1)], dict(width=3)),
    'unknown dtype': ('an unknown input dtype', [dict(dtype=5)], {}),                      # EMB_F16
    'unknown dtype, float64': ('an unknown input dtype', [dict(dtype=8)], {}),
    'unknown dtype, negative': ('an unknown input dtype', [dict(dtype=-1)], {}),
    'unknown kind': ('an unknown kind', [dict(kind=3)], {}),
    'unknown kind, negative': ('an unknown kind', [dict(kind=-1)], {}),
    'count 0': ('the number of keys is outside 1 .. 16', [dict()], dict(count=0)),
    'count 17': ('the number of keys is outside 1 .. 16', [dict(elements=1)] * 17, dict(count=17, width=17)),
    'count negative': ('the number of keys is outside 1 .. 16', [dict()], dict(count=-1)),
    'null x': ('a null address', [dict(), dict(x=None)], dict(width=8)),
    'null out': ('a null address', [dict()], dict(out=None)),
    'null table': ('a null address', None, {}),
    'one-hot of float32': ('one-hot of a float input', [dict(kind=0, classes=3)], dict(width=12)),
    'one-hot of bfloat16': ('one-hot of a float input', [dict(kind=0, classes=3, dtype=6)], dict(width=12)),
    'symlog of int32': ('squish of an integer input', [dict(kind=2, dtype=3)], {}),
    'symlog of int64': ('squish of an integer input', [dict(kind=2, dtype=4)], {}),
    'symlog of uint8': ('squish of an integer input', [dict(kind=2, dtype=0)], {}),
    'symlog of bool': ('squish of an integer input', [dict(kind=2, dtype=9)], {}),
    'classes 0': ('classes outside 1 .. 16384', [dict(ONEHOT, classes=0)], dict(width=1)),
    'classes 16385': ('classes outside 1 .. 16384', [dict(ONEHOT, elements=1, classes=16385)], dict(width=16384)),
    'elements 0': ('a key of less than 1 element', [dict(elements=0)], dict(width=4)),
    'x off its element size': ('an address off its element size', [dict(x=+2)], {}),
    'out off its element size': ('an address off its element size', [dict()], dict(out=+2)),
    'width 0': ('width outside 1 .. 16384', [dict()], dict(width=0)),
    'width 16385': ('width outside 1 .. 16384', [dict(elements=16385)], dict(width=16385)),
    'stride < width': ('out_stride < width', [dict()], dict(stride=3)),
    'rows negative': ('rows < 0', [dict()], dict(rows=-1)),
    'too many elements': ('more than 2^31 - 1 elements of out', [dict()], dict(rows=1 << 30, stride=4)),
    'out dtype': ('out is neither float32 nor bfloat16', [dict()], dict(dtype=5)),
}


@pytest.mark.parametrize('rows', (0, 3))
@pytest.mark.parametrize('which', sorted(REFUSALS))
def test_dict_concat_refuses_before_any_hip_call(which, rows):
  """EMB_ERR_INVALID, the message, no launch -- with rows = 0 as with rows.  The
  addresses are host memory: nothing dereferences them."""
  from embodied_amd import _lib
  message, entries, call = REFUSALS[which]
  fake = np.zeros(64, np.float32)
  base = fake.ctypes.data
  if entries is not None:
    entries = [dict(e, x=base + e['x']) if isinstance(e.get('x'), int) else e for e in entries]
    table = _table(_lib, base, *entries)
    default_width = sum(e.elements * e.classes if e.kind == _lib.DICT_ONEHOT else e.elements for e in table)
  else:
    table, default_width = None, 4
  width = call.get('width', default_width)
  out = call.get('out', 0)
  count = call['count'] if 'count' in call else 1 if entries is None else len(entries)
  args = (table, count, call.get('rows', rows), width, None if out is None else base + 128 + out, call.get('stride', width),
          call.get('dtype', _lib.F32), None, 0, None)
  before = _lib.launches('dict_concat')
  status = _raw(_lib)(*args)
  assert status == _lib.ERR_INVALID, (which, status)
  assert message.encode() in _lib.lib.emb_last_error(), (which, _lib.lib.emb_last_error())
  with pytest.raises(ValueError, match=re.escape(message)):          # the same through the call shim
    _lib.fast.emb_dict_concat(*args)
  assert _lib.launches('dict_concat') == before


def test_dict_concat_accepts_good_tables_and_launches_nothing_without_rows():
  from embodied_amd import _lib
  fake = np.zeros(64, np.float32)
  base = fake.ctypes.data
  raw = _raw(_lib)
  before = _lib.launches('dict_concat')
  good = [
      (_table(_lib, base, dict()), 4, 4),
      (_table(_lib, base, dict(), ONEHOT, dict(kind=2, elements=3)), 17, 40),
      (_table(_lib, base, dict(first=10), dict(ONEHOT, first=0)), 14, 14),                       # in any order
      (_table(_lib, base, *[dict(elements=1, dtype=d) for d in (7, 6, 3, 4, 0, 9)]), 6, 6),       # none of every dtype
      (_table(_lib, base, *[dict(ONEHOT, dtype=d, elements=1, classes=2) for d in (3, 4, 0, 9)]), 8, 8),
      (_table(_lib, base, *[dict(elements=1024)] * 16), 16384, 16384),
      (_table(_lib, base, dict(ONEHOT, elements=1, classes=16384)), 16384, 1 << 20),
  ]
  for table, width, stride in good:
    for dtype in (_lib.F32, _lib.BF16):
      assert raw(table, len(table), 0, width, C.c_void_p(base + 128), stride, dtype, None, 1, None) == _lib.OK, (width, stride)
  assert _lib.launches('dict_concat') == before
  assert _lib.lib.emb_dict_concat_launches(None) == _lib.ERR_INVALID


# ----------------------------------------------------------------- facade --

def _spaces():
  return {'a': Space(np.float32, (3,)), 'b': Space(np.int32, (), 0, 5)}


def test_facade_refuses_on_host_tensors():
  from embodied_amd import nets
  concat = nets.DictConcat(_spaces())
  assert concat.keys == ['a', 'b'] and concat.width == 8 and concat.dtype == torch.bfloat16
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    concat({'a': torch.zeros(2, 3), 'b': torch.zeros(2, dtype=torch.int32)})
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    nets.dict_concat({'a': np.zeros((2, 3), np.float32), 'b': np.zeros(2, np.int32)}, _spaces())
  with pytest.raises(KeyError, match="no input for \\['b'\\]"):
    concat({'a': torch.zeros(2, 3)})
  with pytest.raises(NotImplementedError, match='Images are not supported.'):
    nets.DictConcat({'image': Space(np.uint8, (8, 8, 3))})
  with pytest.raises(NotImplementedError, match='Images are not supported.'):
    nets.DictConcat({'image': Space(np.uint8, (8, 8))})
  nets.DictConcat({'bytes': Space(np.uint8, (8,), 0, 4)})               # rank 1 is no image
  with pytest.raises(ValueError, match='differ in classes'):
    nets.DictConcat({'b': Space(np.int32, (3,), 0, np.array([2, 3, 4]))})
  with pytest.raises(ValueError, match='fdims'):
    nets.DictConcat(_spaces(), fdims=0)
  with pytest.raises(ValueError, match='squish'):
    nets.DictConcat(_spaces(), squish='symexp')
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    nets.DictConcat(_spaces(), dtype=torch.float16)
  assert nets.DictConcat(_spaces(), squish='symlog').squish == 'symlog' and nets.DictConcat(_spaces(), squish='none').squish is None
  for doc in (nets.DictConcat.__doc__,):
    assert 'composed' in doc and 'fused' in doc and 'int32 range' in doc and 'rssm.py:137' in doc


def test_path_decision_goes_through_the_shared_helper():
  from embodied_amd import nets
  fits = [(True, 'a'), (True, 'b')]
  assert nets._dict_path(None, fits) is True and nets._dict_path(True, fits) is True and nets._dict_path(False, fits) is False
  fits = [(True, 'a'), (False, '17 keys, the kernel takes at most 16')]
  assert nets._dict_path(None, fits) is False and nets._dict_path(False, fits) is False
  with pytest.raises(ValueError, match=r'dict_concat\(fused=True\): 17 keys.*fused=None or False'):
    nets._dict_path(True, fits)
  # what does not fit: fdims > 1, more than 16 keys, widths and classes over the limits, an input that requires grad
  def wordings(concat, xs, rows=4, stride=None):
    return [w for holds, w in concat._fits(xs, rows, concat.width if stride is None else stride) if not holds]
  xs = {'a': torch.zeros(4, 3), 'b': torch.zeros(4, dtype=torch.int32)}
  assert wordings(nets.DictConcat(_spaces()), xs) == []
  assert 'fdims = 2' in wordings(nets.DictConcat(_spaces(), fdims=2), xs)[0]
  many = {f'k{i:02d}': Space(np.float32, (1,)) for i in range(17)}
  assert '17 keys' in wordings(nets.DictConcat(many), {k: torch.zeros(4, 1) for k in many})[0]
  wide = {'a': Space(np.float32, (16385,))}
  assert '16385 columns' in wordings(nets.DictConcat(wide), {'a': torch.zeros(1, 16385)})[0]
  classy = {'b': Space(np.int32, (), 0, 16385)}
  assert any('classes' in w for w in wordings(nets.DictConcat(classy), {'b': torch.zeros(1, dtype=torch.int32)}))
  assert 'requires grad' in wordings(nets.DictConcat(_spaces()), dict(xs, a=torch.zeros(4, 3, requires_grad=True)))[0]
  assert '2^31 - 1' in wordings(nets.DictConcat(_spaces()), xs, rows=1 << 29, stride=8)[0]
  assert 'float64' in wordings(nets.DictConcat(_spaces()), dict(xs, a=torch.zeros(4, 3, dtype=torch.float64)))[0]
  assert 'compares integers' in wordings(nets.DictConcat(_spaces()), dict(xs, b=torch.zeros(4)))[0]
  assert 'squishes floats' in wordings(nets.DictConcat(_spaces(), squish='symlog'), dict(xs, a=torch.zeros(4, 3, dtype=torch.int32)))[0]


def test_key_table_is_built_once_per_signature():
  from embodied_amd import _lib, nets
  concat = nets.DictConcat({'a': Space(np.float32, (2, 3)), 'b': Space(np.int64, (2,), 0, 5), 'c': Space(bool)}, squish='symlog')
  signature = (torch.float32, torch.int64, torch.bool)
  table = concat._table(signature)
  assert concat._table(signature) is table and concat._table((torch.bfloat16, torch.int32, torch.bool)) is not table
  rows = [(e.dtype, e.kind, e.elements, e.classes, e.first) for e in table]
  assert rows == [(_lib.F32, _lib.DICT_SYMLOG, 6, 0, 0), (_lib.I64, _lib.DICT_ONEHOT, 2, 5, 6), (_lib.BOOL, _lib.DICT_ONEHOT, 1, 2, 16)]
  assert concat.width == 18


# --------------------------------------- the GPU sweep covers every path --

def test_sweep_covers_the_ladder_and_the_second_grid_pass():
  assert K['block'] == 256 and K['wave'] == 64 and K['block'] % K['wave'] == 0
  assert len(K['ladder_lanes']) == len(K['ladder_widths']) + 1 and K['ladder_lanes'][-1] == K['wave']
  assert list(K['ladder_widths']) == sorted(K['ladder_widths']) and list(K['ladder_lanes']) == sorted(K['ladder_lanes'])
  assert all(K['wave'] % n == 0 and n & (n - 1) == 0 for n in K['ladder_lanes'])
  # every step of the ladder: the last width of a rung, and one to either side
  for last in K['ladder_widths']:
    assert {last - 1, last, last + 1} <= set(cases.SWEEP_WIDTHS), last
    assert cases.lanes(last, K) < cases.lanes(last + 1, K)
  assert {cases.lanes(w, K) for w in cases.SWEEP_WIDTHS} == set(K['ladder_lanes'])
  assert {1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257} <= set(cases.SWEEP_WIDTHS)
  # widths that are no multiple of a 16-byte group, in both output dtypes, and some that are
  assert any(w % 8 for w in cases.SWEEP_WIDTHS) and any(w % 8 == 0 for w in cases.SWEEP_WIDTHS)
  # more than one workgroup, and rows that do not fill the last one
  assert max(cases.SWEEP_ROWS) > K['block'] // K['ladder_lanes'][-1] and cases.SWEEP_ROWS == (1, 3, 17)
  # the second grid pass, on the narrowest and the widest rung, within about a million elements
  rungs = set()
  for rows, width in cases.PAST_GRID:
    assert cases.pass_rows(width, K) < rows <= cases.pass_rows(width, K) + 64, (rows, width)
    assert rows * width <= 1.1 * 2 ** 20 and rows > cases.DISTINCT
    rungs.add(cases.lanes(width, K))
  assert rungs == {K['ladder_lanes'][0], K['ladder_lanes'][-1]}
  assert cases.KEY_COUNTS == (1, 2, 3, 16) and cases.CLASSES == (1, 2, 18, 255, 257)
  assert {int(np.prod(s)) for s in cases.SHAPED} == {1, 3, 9, 6} and (2, 3) in cases.SHAPED
  for width in cases.SWEEP_WIDTHS:
    for parts in cases.KEY_COUNTS:
      sizes = cases.split_width(width, parts)
      assert sum(sizes) == width and min(sizes) >= 1 and len(sizes) == min(parts, width)
