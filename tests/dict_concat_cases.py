"""Cases, seeded inputs and a numpy restatement of `nn.DictConcat`
(embodied/jax/nets.py:467-500) with the reset masks and the clamp around it
(dreamerv3/rssm.py:76-79, 137).

Shared by `tools/gen_dict_concat_golden.py` (which feeds the fixture's inputs to
the reference's own `DictConcat`), `tools/dict_concat_accuracy.py` and the tests.
`restate` is this project's own numpy code in one float type.  A bfloat16 input
is held here as the float32 array of its values (every one of them a bfloat16
number); the GPU test turns it into a bfloat16 tensor without rounding.
"""
import collections
import pathlib
import re

import numpy as np

from embodied_amd.space import Space
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32
ROOT = pathlib.Path(__file__).resolve().parent.parent

# The symlog bar, in float32 ulps of the float64 value.  Measured by
# tools/dict_concat_accuracy.py (profiles/dict_concat_accuracy.txt): over the
# fixture's symlog cases the reference's own float32 run is at most
# SYMLOG_REFERENCE_ULP from its float64 run.  The kernel gets twice that and not
# less than one ulp: the device log1p is another implementation than numpy's.
SYMLOG_REFERENCE_ULP = 1.0336
SYMLOG_BAR_ULP = max(2 * SYMLOG_REFERENCE_ULP, 1.0)

# A key: its name, the space (dtype, shape, classes of a discrete one) and the
# dtype of the input ('bf16' or a numpy dtype name).
Key = collections.namedtuple('Key', 'name dtype shape classes feed')
Case = collections.namedtuple('Case', 'name keys squish rows reset unit scale')


def _k(name, dtype, shape=(), classes=None, feed=None):
  return Key(name, dtype, tuple(shape), classes, feed or np.dtype(dtype).name)


CASES = (
    # the RSSM's action dicts: one discrete key of 18 classes; one float key of 6; two of each
    Case('disc18', (_k('action', 'int32', (), 18),), None, 5, False, False, 1.0),
    Case('float6', (_k('action', 'float32', (6,)),), None, 17, False, False, 1.0),
    Case('two_each', (_k('b_move', 'int32', (), 18), _k('d_pick', 'int64', (3,), 5),
                      _k('a_arm', 'float32', (4,)), _k('c_grip', 'float32', (2, 3), feed='bf16')), None, 9, True, True, 2.0),
    # the Encoder's vector input: symlog over float keys of mixed shapes and magnitudes
    Case('symlog8', tuple(_k(f'v{i}', 'float32', shape) for i, shape in
                          enumerate(((), (1,), (3,), (7,), (2, 3), (9,), (16,), (5,)))), 'symlog', 33, False, False, 50.0),
    Case('symlog_unit', (_k('x', 'float32', (9,)), _k('y', 'float32', (2,))), 'symlog', 9, True, True, 4.0),
    # all six input dtypes at once
    Case('six_dtypes', (_k('f', 'float32', (3,)), _k('h', 'float32', (2,), feed='bf16'), _k('i', 'int32', (2,), 4),
                        _k('l', 'int64', (), 7), _k('u', 'uint8', (3,), 255), _k('z', 'bool', (2,), 2)), None, 9, True, False, 3.0),
)


def tag(case):
  return f'c{case}_{CASES[case].name}'


def space_of(key):
  if key.classes is None:
    return Space(key.dtype, key.shape)
  if np.dtype(key.dtype) == bool:
    return Space(bool, key.shape)
  return Space(key.dtype, key.shape, 0, key.classes)


def spaces_of(keys):
  return {k.name: space_of(k) for k in keys}


def width_of(keys):
  return sum(int(np.prod(k.shape, dtype=np.int64)) * (k.classes or 1) for k in keys)


def inputs_of(keys, rows, scale, rng, holes=True, reset=False):
  """Seeded inputs of `rows` rows.  With `holes`, rows 1 and rows - 1 of every
  other key hold an unavailable element (first and last element in turn) and a
  float key a NaN in row 0; out-of-range indices are left to the GPU tests."""
  inp = {}
  for i, k in enumerate(sorted(keys, key=lambda k: k.name)):
    shape = (rows, *k.shape)
    if k.classes is None:
      x = (scale * rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(f32)
      if k.feed == 'bf16':
        x = bf16_round(x)
      if holes and rows > 2:
        flat = x.reshape(rows, -1)
        flat[0, -1] = np.nan
        if i % 2 == 0:
          flat[1, 0] = -np.inf
          flat[rows - 1, -1] = -np.inf
    elif np.dtype(k.dtype) == bool:
      x = rng.integers(0, 2, shape).astype(bool)
    else:
      x = rng.integers(0, k.classes, shape).astype(k.dtype)
      if holes and rows > 2 and np.dtype(k.dtype).kind == 'i' and i % 2 == 0:
        flat = x.reshape(rows, -1)
        flat[1, -1] = -1
        flat[rows - 1, 0] = -1
    inp[k.name] = x
  if reset:
    inp['reset'] = (np.arange(rows) % 3 == 2)
  return inp


def inputs(case):
  c = CASES[case]
  return inputs_of(c.keys, c.rows, c.scale, np.random.default_rng([case, c.rows, len(c.keys)]), reset=c.reset)


def symlog(x):
  return np.sign(x) * np.log1p(np.abs(x))


def restate(keys, inp, squish=None, unit=False, ftype=np.float64):
  """nets.py:476-500, rssm.py:76-79 and rssm.py:137 over (rows, ...) inputs, every
  float operation in `ftype`: (rows, width).  An index is compared as a 64-bit
  integer: an int64 beyond the int32 range matches no class."""
  ys = []
  with np.errstate(invalid='ignore'):
    for k in sorted(keys, key=lambda k: k.name):
      x = np.asarray(inp[k.name])
      rows = x.shape[0]
      x = x.reshape(rows, -1)
      if x.dtype.kind == 'f':
        there = (x != -np.inf).all(-1)
      elif x.dtype.kind == 'i':
        there = (x != -1).all(-1)
      else:
        there = np.ones(rows, bool)
      if k.classes is not None:
        y = (x.astype(np.int64)[:, :, None] == np.arange(k.classes)).reshape(rows, -1).astype(ftype)
      else:
        y = x.astype(ftype)
        if squish == 'symlog':
          y = symlog(y)
      ys.append(np.where(there[:, None], y, ftype(0)))
    y = np.concatenate(ys, -1)
    if inp.get('reset') is not None:
      y = np.where(np.asarray(inp['reset']).astype(bool)[:, None], ftype(0), y)
    if unit:
      y = y / np.maximum(ftype(1), np.abs(y))
  return y


def stored(values, bf16, unit=False):
  """What the reference holds for the exact kinds (identity, one-hot, masks,
  clamp) given its float32 values BEFORE the clamp: rounded to the compute dtype,
  then divided (rssm.py:137 runs on the rounded action)."""
  v = bf16_round(np.asarray(values, f32)) if bf16 else np.asarray(values, f32)
  if unit:
    with np.errstate(invalid='ignore'):
      v = (v / np.maximum(f32(1), np.abs(v))).astype(f32)
    v = bf16_round(v) if bf16 else v
  return v


def ulps(got, want64):
  """|got - want| in float32 ulps of the float64 value, elementwise; 0 where both are the same NaN or infinity."""
  got, want = np.asarray(got, np.float64), np.asarray(want64, np.float64)
  same = (np.isnan(got) & np.isnan(want)) | (got == want)
  with np.errstate(invalid='ignore', over='ignore'):
    spacing = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
    return np.where(same, 0.0, np.abs(got - want) / spacing)


def bf16_bar(want64):
  """Half a bfloat16 ulp of the float64 value plus the float32 bar, as an absolute error."""
  want = np.abs(np.asarray(want64, np.float64))
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    exponent = np.floor(np.log2(np.maximum(want, np.finfo(f32).tiny)))
    return 0.5 * 2.0 ** (exponent - 7) + SYMLOG_BAR_ULP * np.spacing(want.astype(f32)).astype(np.float64)


# ------------------------------------------------------------ the GPU sweep --

def header_constants():
  """The grid cap and the packing ladder as csrc/dict_concat.h spells them."""
  text = (ROOT / 'embodied_amd' / 'csrc' / 'dict_concat.h').read_text()
  def scalar(name):
    return int(re.search(r'constexpr\s+\w+\s+%s\s*=\s*(\d+)' % name, text).group(1))
  def array(name):
    return tuple(int(v) for v in re.search(r'%s\[[^\]]*\]\s*=\s*\{([^}]*)\}' % name, text).group(1).split(','))
  return {'block': scalar('kDictBlock'), 'max_blocks': scalar('kDictMaxBlocks'), 'wave': scalar('kDictWave'),
          'max_width': scalar('kDictMaxWidth'), 'max_classes': scalar('kDictMaxClasses'),
          'ladder_widths': array('kDictLadderWidths'), 'ladder_lanes': array('kDictLadderLanes')}


def lanes(width, k):
  for last, n in zip(k['ladder_widths'], k['ladder_lanes']):
    if width <= last:
      return n
  return k['ladder_lanes'][-1]


def pass_rows(width, k):
  """Rows one pass of the capped grid covers."""
  return k['max_blocks'] * (k['block'] // lanes(width, k))


# widths of the issue, and every step of the ladder -1, +0, +1
SWEEP_WIDTHS = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SWEEP_ROWS = (1, 3, 17)
# past one pass of the capped grid, on the narrowest and on the widest rung: (rows, width), tiled from DISTINCT rows
DISTINCT = 13
PAST_GRID = ((65536 + 5, 7), (8192 + 3, 129))
KEY_COUNTS = (1, 2, 3, 16)
CLASSES = (1, 2, 18, 255, 257)
SHAPED = ((1,), (3,), (9,), (2, 3))


def split_width(width, parts):
  """`parts` positive sizes that add up to `width`, the larger ones first."""
  parts = min(parts, width)
  base, extra = divmod(width, parts)
  return [base + (i < extra) for i in range(parts)]


def float_keys(width, parts=3, feed=None):
  """`width` columns as up to `parts` float32 keys."""
  return tuple(_k(f'k{i:02d}', 'float32', (n,), feed=feed) for i, n in enumerate(split_width(width, parts)))
