"""`nets.DictConcat` on the GPU: the kernel (`fused=True`) and the composed path
(`fused=False`) against what the reference's own `DictConcat` returned
(tests/golden/dict_concat.npz) and against the numpy restatement the host test
holds to that fixture, over every width around the packing ladder, past the
capped grid, every input dtype, and the edges of availability, indices, reset,
the clamp and `out=`.  Identity, one-hot, masks and clamp are exact; symlog is
held to the measured bar of tests/dict_concat_cases.py."""
import numpy as np
import pytest
import torch

from embodied_amd import nets
from tests import dict_concat_cases as cases

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
_k = cases._k


@pytest.fixture(scope='module')
def golden():
  with np.load(cases.ROOT / 'tests' / 'golden' / 'dict_concat.npz') as f:
    return {k: f[k] for k in f.files}


def tensors(keys, inp):
  xs = {}
  for k in keys:
    x = torch.from_numpy(np.ascontiguousarray(inp[k.name])).cuda()
    xs[k.name] = x.to(torch.bfloat16) if k.feed == 'bf16' else x         # every value is a bfloat16 number: exact
  return xs


def run(keys, inp, squish=None, unit=False, dtype=torch.float32, fused=True, reset='inp', concat=None, **kw):
  concat = concat or nets.DictConcat(cases.spaces_of(keys), squish=squish, dtype=dtype)
  if isinstance(reset, str):
    reset = inp.get('reset')
  if isinstance(reset, np.ndarray):
    reset = torch.from_numpy(reset).cuda()
  got = concat(tensors(keys, inp), reset=reset, unit=unit, fused=fused, **kw)
  assert got.dtype == dtype and not got.requires_grad and got.is_cuda
  return got.float().cpu().numpy()


def exact(keys, inp, unit, bf16):
  """The reference's stored values of the exact kinds: float32 before the clamp,
  rounded to the compute dtype, then divided."""
  return cases.stored(cases.restate(keys, inp, None, False, np.float32), bf16, unit)


def same_bits(got, want, what=''):
  got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), (what, 'NaNs moved')
  bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
  assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def mixed_keys(width):
  """`width` columns as a one-hot int32 key in the middle of two float keys (floats alone below 4)."""
  if width < 4:
    return cases.float_keys(width, 2)
  classes = width // 2
  left, right = cases.split_width(width - classes, 2)
  return (_k('a', 'float32', (left,)), _k('b', 'int32', (), classes), _k('c', 'float32', (right,), feed='bf16'))


# ---------------------------------------------------------------- fixture --

@pytest.mark.parametrize('fused', (True, False))
@pytest.mark.parametrize('kind', sorted(DTYPES))
@pytest.mark.parametrize('case', range(len(cases.CASES)))
def test_fixture_parity(golden, case, kind, fused):
  c, name = cases.CASES[case], cases.tag(case)
  got = run(c.keys, cases.inputs(case), c.squish, c.unit, DTYPES[kind], fused)
  want32, want64 = golden[f'out_{name}'], golden[f'out64_{name}']
  if c.squish is None:
    # round-then-divide of the float32 run: bf16(v / max(1, |v|)) is bf16(v) / max(1, |bf16(v)|) for every finite v
    same_bits(got, cases.bf16_round(want32) if kind == 'bf16' else want32, name)
    return
  assert np.array_equal(np.isnan(got), np.isnan(want64))
  if kind == 'f32':
    worst = cases.ulps(got, want64).max()
    print(f'{name} fused={fused}: worst {worst:.4f} float32 ulp of the float64 value (bar {cases.SYMLOG_BAR_ULP:.4f})')
    assert worst <= cases.SYMLOG_BAR_ULP
  else:
    ok = np.isnan(want64) | (got == want64)
    share = np.where(ok, 0.0, np.abs(got - want64) / cases.bf16_bar(want64))
    print(f'{name} fused={fused}: worst {share.max():.4f} of the bfloat16 bar')
    assert share.max() <= 1.0


def test_symlog_of_bfloat16_inputs_is_float32_arithmetic():
  keys = (_k('a', 'float32', (9,), feed='bf16'), _k('b', 'float32', (2, 3), feed='bf16'))
  inp = cases.inputs_of(keys, 17, 30.0, np.random.default_rng(11))
  want = cases.restate(keys, inp, 'symlog', False, np.float64)
  got = run(keys, inp, 'symlog')
  assert np.array_equal(np.isnan(got), np.isnan(want)) and cases.ulps(got, want).max() <= cases.SYMLOG_BAR_ULP


# ------------------------------------------------------------------ sweeps --

@pytest.mark.parametrize('width', cases.SWEEP_WIDTHS)
def test_widths_and_rows(width):
  keys = mixed_keys(width)
  assert cases.width_of(keys) == width
  for rows in cases.SWEEP_ROWS:
    inp = cases.inputs_of(keys, rows, 2.0, np.random.default_rng([width, rows]), reset=rows == 17)
    for kind, dtype in DTYPES.items():
      for unit in (False, True):
        got = run(keys, inp, None, unit, dtype)
        same_bits(got, exact(keys, inp, unit, kind == 'bf16'), (width, rows, kind, unit))
    same_bits(run(keys, inp, fused=False), exact(keys, inp, False, False), (width, rows, 'composed'))


@pytest.mark.parametrize('rows,width', cases.PAST_GRID)
def test_past_the_capped_grid(rows, width):
  """A small set of distinct rows, tiled: every row of the large run is the bits of its row in the small one."""
  keys = mixed_keys(width)
  small = cases.inputs_of(keys, cases.DISTINCT, 2.0, np.random.default_rng([rows, width]), reset=True)
  index = np.arange(rows) % cases.DISTINCT
  large = {k: v[index] for k, v in small.items()}
  for kind, dtype in DTYPES.items():
    few = run(keys, small, None, True, dtype)
    same_bits(few, exact(keys, small, True, kind == 'bf16'), (rows, width, kind))
    many = run(keys, large, None, True, dtype)
    assert many.shape == (rows, width)
    same_bits(many, few[index], (rows, width, kind, 'tiled'))


@pytest.mark.parametrize('count', cases.KEY_COUNTS)
def test_key_counts(count):
  width = 48
  kinds = [('float32', None, None), ('int32', 3, None), ('float32', None, 'bf16'), ('int64', 2, None), ('uint8', 4, None), ('bool', 2, None)]
  keys, left = [], width
  for i in range(count):
    dtype, classes, feed = kinds[i % len(kinds)]
    span = left if i == count - 1 else max(1, width // count)
    elements = span if classes is None else max(1, span // classes)
    if i == count - 1 and classes is not None:                         # the last key fills what is left
      dtype, classes, elements = 'float32', None, left
    keys.append(_k(f'k{i:02d}', dtype, (elements,), classes, feed))
    left -= elements * (classes or 1)
  assert left == 0 and len(keys) == count
  inp = cases.inputs_of(keys, 9, 2.0, np.random.default_rng(count), reset=True)
  for kind, dtype in DTYPES.items():
    same_bits(run(keys, inp, None, True, dtype), exact(keys, inp, True, kind == 'bf16'), (count, kind))
  same_bits(run(keys, inp, fused=False), exact(keys, inp, False, False), (count, 'composed'))


def test_all_six_input_dtypes_at_once_and_integers_under_a_float_space():
  keys = (_k('a', 'float32', (3,)), _k('b', 'float32', (2,), feed='bf16'), _k('c', 'int32', (2,), 4),
          _k('d', 'int64', (2,), 7), _k('e', 'uint8', (3,), 9), _k('f', 'bool', (2,), 2))
  inp = cases.inputs_of(keys, 17, 3.0, np.random.default_rng(6), reset=True)
  for kind, dtype in DTYPES.items():
    same_bits(run(keys, inp, None, True, dtype), exact(keys, inp, True, kind == 'bf16'), kind)
  # a continuous space fed integers: the cast alone, -1 still means unavailable for the signed ones
  keys = tuple(_k(n, 'float32', (3,)) for n in 'abcd')
  rng = np.random.default_rng(7)
  inp = {'a': rng.integers(-1, 300, (9, 3)).astype(np.int32), 'b': rng.integers(-1, 2 ** 40, (9, 3)).astype(np.int64),
         'c': rng.integers(0, 256, (9, 3)).astype(np.uint8), 'd': rng.integers(0, 2, (9, 3)).astype(bool)}
  inp['a'][2, 1] = inp['b'][3, 2] = -1
  inp['c'][4] = 255
  want = cases.restate(keys, inp, None, False, np.float32)
  assert (want[2, 0:3] == 0).all() and (want[3, 3:6] == 0).all() and (want[4, 6:9] == 255).all()
  for kind, dtype in DTYPES.items():
    same_bits(run(keys, inp, dtype=dtype), cases.stored(want, kind == 'bf16'), kind)
  same_bits(run(keys, inp, fused=False), want, 'composed')


@pytest.mark.parametrize('shape', cases.SHAPED)
def test_shaped_spaces(shape):
  keys = (_k('a', 'float32', shape), _k('b', 'int32', shape, 5), _k('c', 'int64', shape, 3), _k('d', 'float32', shape, feed='bf16'))
  inp = cases.inputs_of(keys, 17, 2.0, np.random.default_rng(len(shape) * 10 + shape[0]))
  for kind, dtype in DTYPES.items():
    same_bits(run(keys, inp, dtype=dtype), exact(keys, inp, False, kind == 'bf16'), (shape, kind))
  same_bits(run(keys, inp, fused=False), exact(keys, inp, False, False), (shape, 'composed'))
  # more batch axes than one: (3, 4, *shape) gives (3, 4, width)
  inp = cases.inputs_of(keys, 12, 2.0, np.random.default_rng(3), holes=False)
  xs = {k: v.reshape(3, 4, *v.shape[1:]) for k, v in tensors(keys, inp).items()}
  got = nets.DictConcat(cases.spaces_of(keys), dtype=torch.float32)(xs, fused=True)
  assert got.shape == (3, 4, cases.width_of(keys))
  same_bits(got.reshape(12, -1).cpu().numpy(), exact(keys, inp, False, False))


@pytest.mark.parametrize('classes', cases.CLASSES)
def test_classes(classes):
  for dtype in ('int32', 'int64', 'uint8'):
    if dtype == 'uint8' and classes > 255:
      continue
    keys = (_k('a', dtype, (2,), classes), _k('b', 'float32', (3,)))
    inp = cases.inputs_of(keys, 17, 1.0, np.random.default_rng(classes))
    want = exact(keys, inp, False, False)
    there = ~(np.asarray(inp['a']) == -1).any(-1) if dtype != 'uint8' else np.ones(17, bool)
    assert (want[there, :2 * classes].sum(-1) == 2).all()                 # one 1 per element
    for kind, out in DTYPES.items():
      same_bits(run(keys, inp, dtype=out), cases.stored(want, kind == 'bf16'), (classes, dtype, kind))
    same_bits(run(keys, inp, fused=False), want, (classes, dtype, 'composed'))


# ------------------------------------------------------------ availability --

@pytest.mark.parametrize('feed,hole', (('float32', -np.inf), ('bf16', -np.inf), ('int32', -1), ('int64', -1)))
def test_one_hole_zeroes_its_key_in_its_row_only(feed, hole):
  discrete = feed.startswith('int')
  mid = _k('b', feed, (5,), 4) if discrete else _k('b', 'float32', (5,), feed=feed)
  keys = (_k('a', 'float32', (3,)), mid, _k('c', 'float32', (2,)))
  clean = cases.inputs_of(keys, 9, 1.0, np.random.default_rng(1), holes=False)
  span = slice(3, 3 + (20 if discrete else 5))
  base = run(keys, clean)
  same_bits(base, exact(keys, clean, False, False))
  assert (base[:, span] != 0).any(-1).all()
  for row, element in ((0, 0), (4, 4), (8, 2)):                          # first element only, last only, one inside
    inp = {k: v.copy() for k, v in clean.items()}
    inp['b'][row, element] = hole
    for fused in (True, False):
      got = run(keys, inp, fused=fused)
      assert (got[row, span] == 0).all(), (row, element, fused)
      untouched = np.ones_like(got, bool)
      untouched[row, span] = False
      assert np.array_equal(got[untouched], base[untouched]), (row, element, fused)


def test_nan_is_kept_and_unsigned_and_bool_are_always_there():
  keys = (_k('a', 'float32', (4,)), _k('b', 'uint8', (3,), 255), _k('c', 'bool', (2,), 2), _k('d', 'float32', (2,), feed='bf16'))
  inp = cases.inputs_of(keys, 5, 1.0, np.random.default_rng(2), holes=False)
  inp['a'][1, 2] = np.nan
  inp['d'][3, 0] = np.nan
  inp['a'][2, 1] = np.inf                                                 # +inf is a value
  inp['b'][0] = 255                                                       # no class of 255, and no hole either
  inp['b'][1] = (254, 0, 255)
  inp['c'][:] = True
  for unit in (False, True):
    for fused in (True, False):
      got = run(keys, inp, unit=unit, fused=fused)
      assert np.argwhere(np.isnan(got)).tolist() == ([[1, 2], [3, 4 + 765 + 4]] if not unit else [[1, 2], [2, 1], [3, 4 + 765 + 4]])
      assert np.isnan(got[1, 2]) and (got[1, [0, 1, 3]] == inp['a'][1, [0, 1, 3]].clip(-1, 1) if unit else got[1, [0, 1, 3]] == inp['a'][1, [0, 1, 3]]).all()
      onehot = got[:, 4:4 + 765].reshape(5, 3, 255)
      assert (onehot[0] == 0).all() and onehot[1, 0, 254] == 1 and onehot[1, 1, 0] == 1 and (onehot[1, 2] == 0).all()
      assert onehot[1].sum() == 2 and (onehot[2:].sum(-1) == 1).all()
      assert (got[:, 4 + 765:4 + 765 + 4].reshape(5, 2, 2) == [0, 1]).all()
      if not unit:
        assert got[2, 1] == np.inf


def test_indices_out_of_range_give_zeros_and_touch_no_other_row():
  classes = 6
  for dtype, values in (('int32', (-2, classes, 2 ** 31 - 1, -2 ** 31)), ('int64', (-2, classes, 2 ** 31 - 1, 2 ** 32 + 1, -2 ** 63))):
    keys = (_k('a', 'float32', (3,)), _k('b', dtype, (2,), classes))
    clean = cases.inputs_of(keys, len(values) + 2, 1.0, np.random.default_rng(3), holes=False)
    base = run(keys, clean)
    inp = {k: v.copy() for k, v in clean.items()}
    for row, value in enumerate(values):
      inp['b'][row + 1, row % 2] = value
    got = run(keys, inp)
    for row, value in enumerate(values):
      element = row % 2
      assert (got[row + 1, 3 + element * classes:3 + (element + 1) * classes] == 0).all(), (dtype, value)
      other = 1 - element
      assert np.array_equal(got[row + 1, 3 + other * classes:3 + (other + 1) * classes],
                            base[row + 1, 3 + other * classes:3 + (other + 1) * classes])
      assert np.array_equal(got[row + 1, :3], base[row + 1, :3])
    assert np.array_equal(got[[0, -1]], base[[0, -1]])
    same_bits(got, cases.restate(keys, inp, None, False, np.float32), dtype)
    if dtype == 'int32':                                                  # composed is the definition there too
      same_bits(run(keys, inp, fused=False), got, 'composed')


# ------------------------------------------------------- reset, unit, out --

@pytest.mark.parametrize('as_bool', (True, False))
def test_reset_rows(as_bool):
  keys = mixed_keys(21)
  rows = 17
  inp = cases.inputs_of(keys, rows, 1.0, np.random.default_rng(4), holes=False)
  base = run(keys, inp, reset=None)
  assert (base != 0).any(-1).all()
  for name, flags in (('first', np.arange(rows) == 0), ('last', np.arange(rows) == rows - 1),
                      ('alternating', np.arange(rows) % 2 == 1), ('all', np.ones(rows, bool)), ('none', np.zeros(rows, bool))):
    reset = flags if as_bool else flags.astype(np.uint8) * 255          # any byte that is not 0
    for fused in (True, False):
      for kind, dtype in DTYPES.items():
        got = run(keys, inp, dtype=dtype, reset=reset, fused=fused)
        want = cases.stored(np.where(flags[:, None], np.float32(0), base), kind == 'bf16')
        same_bits(got, want, (name, fused, kind))
        assert (got[flags] == 0).all() and not np.signbit(got[flags]).any()


def test_unit_is_round_then_divide_on_every_finite_value():
  """+inf is a value and gives NaN on both sides; -inf is the mark of an unavailable row, whose span is zeros."""
  one = np.float32(1)
  values = [0.5, 1.0, 1 + 2.0 ** -23, 1.004, 1.002, 1e4, 0.999, 1 - 2.0 ** -24, 0.99805, 3.0e38, 1e-40, 0.0]
  v = np.array([s * x for x in values for s in (1, -1)] + [np.inf], np.float32)
  keys = (_k('a', 'float32', (len(v),)), _k('b', 'int32', (), 3))
  gone = v.copy()
  gone[-1] = -np.inf
  inp = {'a': np.stack([v, v[::-1], gone]), 'b': np.array([2, 0, 1], np.int32)}
  for kind, dtype in DTYPES.items():
    want = exact(keys, inp, True, kind == 'bf16')
    finite = np.isfinite(inp['a'][:2])
    assert np.isnan(want[:2, :len(v)][~finite]).all() and np.isfinite(want[:2, :len(v)][finite]).all()
    assert (np.abs(want[:2, :len(v)][finite]) <= one).all() and (want[2, :len(v)] == 0).all()
    for fused in (True, False):
      same_bits(run(keys, inp, unit=True, dtype=dtype, fused=fused), want, (kind, fused))
    assert (want[:, len(v):] == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]).all()      # one-hot values pass


@pytest.mark.parametrize('kind', sorted(DTYPES))
def test_out_is_a_column_slice_off_16_bytes(kind):
  dtype = DTYPES[kind]
  for width in (7, 21, 70):
    keys = mixed_keys(width)
    inp = cases.inputs_of(keys, 17, 1.0, np.random.default_rng(width), reset=True)
    want = exact(keys, inp, True, kind == 'bf16')
    concat = nets.DictConcat(cases.spaces_of(keys), dtype=dtype)
    for start, total in ((1, width + 9), (3, width + 3), (0, width)):
      buffer = torch.full((17, total), 7.0, dtype=dtype, device='cuda')
      assert buffer.data_ptr() % 16 == 0
      view = buffer[:, start:start + width]
      got = concat(tensors(keys, inp), reset=torch.from_numpy(inp['reset']).cuda(), unit=True, out=view, fused=True)
      assert got is view
      whole = buffer.float().cpu().numpy()
      same_bits(whole[:, start:start + width], want, (width, start))
      assert (whole[:, :start] == 7).all() and (whole[:, start + width:] == 7).all()
      composed = torch.full((17, total), 7.0, dtype=dtype, device='cuda')
      concat(tensors(keys, inp), reset=torch.from_numpy(inp['reset']).cuda(), unit=True, out=composed[:, start:start + width], fused=False)
      assert torch.equal(composed.view(torch.int16 if kind == 'bf16' else torch.int32), buffer.view(torch.int16 if kind == 'bf16' else torch.int32))
  with pytest.raises(ValueError, match='needs'):
    concat(tensors(keys, inp), out=torch.zeros(17, width + 1, dtype=dtype, device='cuda'))
  with pytest.raises(ValueError, match='column stride'):
    concat(tensors(keys, inp), out=torch.zeros(17, 2 * width, dtype=dtype, device='cuda')[:, ::2])


# ---------------------------------------------------- launches and paths --

def test_launch_counts_determinism_and_grad():
  c = cases.CASES[2]
  inp = cases.inputs(2)
  concat = nets.DictConcat(cases.spaces_of(c.keys), dtype=torch.float32)
  xs = tensors(c.keys, inp)
  reset = torch.from_numpy(inp['reset']).cuda()
  before = nets.dict_concat_launches()
  first = concat(xs, reset=reset, unit=True, fused=True)
  assert nets.dict_concat_launches() == before + 1
  again = concat(xs, reset=reset, unit=True, fused=True)
  auto = concat(xs, reset=reset, unit=True)
  assert nets.dict_concat_launches() == before + 3                       # fused=None takes the kernel where it fits
  composed = concat(xs, reset=reset, unit=True, fused=False)
  assert nets.dict_concat_launches() == before + 3
  bits = lambda t: t.view(torch.int32)
  assert torch.equal(bits(first), bits(again)) and torch.equal(bits(first), bits(auto))
  same_bits(composed.cpu().numpy(), first.cpu().numpy())
  assert len(concat._tables) == 1                                          # one table for the four calls
  # the function is the class
  same_bits(nets.dict_concat(xs, cases.spaces_of(c.keys), dtype=torch.float32, reset=reset, unit=True).cpu().numpy(), first.cpu().numpy())
  # an input that requires grad: fused=None composes, fused=True raises; the result never requires grad
  xs['a_arm'] = xs['a_arm'].clone().requires_grad_()
  before = nets.dict_concat_launches()
  got = concat(xs, reset=reset, unit=True)
  assert nets.dict_concat_launches() == before and not got.requires_grad
  same_bits(got.cpu().numpy(), first.cpu().numpy())
  with pytest.raises(ValueError, match=r'dict_concat\(fused=True\): an input requires grad'):
    concat(xs, reset=reset, unit=True, fused=True)
  # a key that is not contiguous is made contiguous
  xs = tensors(c.keys, inp)
  wide = torch.zeros(9, 8, device='cuda')
  wide[:, ::2] = xs['a_arm']
  xs['a_arm'] = wide[:, ::2]
  assert not xs['a_arm'].is_contiguous()
  same_bits(concat(xs, reset=reset, unit=True, fused=True).cpu().numpy(), first.cpu().numpy())
  # no rows: nothing is launched
  before = nets.dict_concat_launches()
  empty = concat({k: v[:0] for k, v in tensors(c.keys, inp).items()})
  assert empty.shape == (0, concat.width) and nets.dict_concat_launches() == before
  # past the limits: composed, and the same answer
  keys = tuple(_k(f'k{i:02d}', 'float32', (1,)) for i in range(17))
  inp = cases.inputs_of(keys, 5, 1.0, np.random.default_rng(17))
  before = nets.dict_concat_launches()
  same_bits(run(keys, inp, fused=None), exact(keys, inp, False, False))
  assert nets.dict_concat_launches() == before
  with pytest.raises(ValueError, match=r'fused=True\): 17 keys'):
    run(keys, inp, fused=True)
  # fdims = 2: the reference's reshape keeps one more axis, composed only
  keys = (_k('a', 'float32', (2, 3)), _k('b', 'int32', (2,), 4))
  inp = cases.inputs_of(keys, 5, 1.0, np.random.default_rng(18), holes=False)
  got = nets.DictConcat(cases.spaces_of(keys), fdims=2, dtype=torch.float32)(tensors(keys, inp))
  assert got.shape == (5, 2, 7)
  want = np.concatenate([inp['a'], (inp['b'][:, :, None] == np.arange(4)).astype(np.float32)], -1)
  same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize('case', [i for i, c in enumerate(cases.CASES) if c.squish is None])
def test_fused_and_composed_agree_bit_for_bit(case):
  c = cases.CASES[case]
  inp = cases.inputs(case)
  for kind, dtype in DTYPES.items():
    same_bits(run(c.keys, inp, None, c.unit, dtype, True), run(c.keys, inp, None, c.unit, dtype, False), (c.name, kind))
