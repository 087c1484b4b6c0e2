"""Tables and helpers of the sweep over the paths of the norm + activation and
blocked GRU gate kernels (csrc/norm_act.hip, csrc/gru_gate.hip) that
tests/test_gpu_norm_act.py and tests/test_gpu_gru_gate.py leave untried.

Shared by tests/test_gpu_rssm_core_sweep.py (which runs the kernels at them) and
tests/test_rssm_core_sweep_host.py (which shows, without a GPU, that every table
does what it says against the kernels' own constants, read out of the source,
and that the float32 definition stays inside the bars at the inputs).  Plain
numpy.  Inputs, the float64 restatement and the bars are those of
tests/norm_act_cases.py and tests/gru_gate_cases.py, unchanged.

What the kernels do, as far as the tables need it (`K`, `G`, the two ladders):

  * Both launchers take 16-byte loads and stores where the width allows it
    (`units` / `h` a multiple of 16 / sizeof(T)) AND every pointer is a multiple
    of 16, and go element by element otherwise.  A_UNITS and B_SHAPES are widths
    that vectorise, run from views that do not start on 16 bytes.
  * The forward launch has at most kMaxBlocks workgroups, the gradient launch at
    most kNormActMaxPartials; up to kNormActWaveUnits a wave takes a row (kBlock /
    kWave rows per workgroup), beyond it a workgroup does.  `forward_pass` and
    `grad_pass` are the rows of one pass of the grid-stride loop; the C_* shapes
    need a second one.
  * Up to kHeldUnits the gradient holds its row in registers, beyond it streams it.
"""
import pathlib
import re

import numpy as np

from tests import gru_gate_cases as gates
from tests import norm_act_cases as norms

f32 = np.float32
CSRC = pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc'
NORM_SOURCE, NORM_HEADER, GATE_SOURCE = CSRC / 'norm_act.hip', CSRC / 'norm_act.h', CSRC / 'gru_gate.hip'
KINDS = ('f32', 'bf16')
EPS = 1e-4
SEED = 23


def _constants(path, names):
  """`constexpr int name = a;` or `= a * b;` as the source spells it."""
  text, found = path.read_text(), {}
  for name in names:
    m = re.search(r'constexpr int %s = (\d+)(?: \* (\d+))?;' % name, text)
    found[name] = int(m.group(1)) * int(m.group(2) or 1)
  return found


def norm_constants():
  return {**_constants(NORM_SOURCE, ('kWave', 'kBlock', 'kMaxBlocks', 'kHeldUnits')),
          **_constants(NORM_HEADER, ('kNormActMaxUnits', 'kNormActWaveUnits', 'kNormActMaxPartials'))}


def gate_constants():
  return _constants(GATE_SOURCE, ('kThreads', 'kMaxBlocks'))


def source_ladder(macro, last):
  """EMB_NORM_BY_WIDTH or EMB_NORM_HELD_BY_WIDTH as the source spells it:
  [(last width, threads per row, values per thread), ...], the closing `else`
  ending at `last`."""
  text = NORM_SOURCE.read_text()
  body = text[text.index('#define %s(' % macro):]
  body = body[:body.index('while (0)')]
  rungs = [tuple(map(int, m)) for m in re.findall(r'if \(\(u\) <= (\d+)\) \{ CALL\((\d+), (\d+)\); \}', body)]
  end = re.search(r'else \{ CALL\((\d+), (\d+)\); \}', body)
  return rungs + [(last, int(end.group(1)), int(end.group(2)))]


K = norm_constants()
G = gate_constants()
FORWARD_LADDER = source_ladder('EMB_NORM_BY_WIDTH', K['kNormActMaxUnits'])
HELD_LADDER = source_ladder('EMB_NORM_HELD_BY_WIDTH', K['kHeldUnits'])
WIDE = 'wide'                                      # norm_act_grad_wide_kernel: past kHeldUnits


def forward_kernel(units):
  """(threads per row, values per thread) of the forward instantiation that runs `units`."""
  assert 1 <= units <= K['kNormActMaxUnits'], units
  return next((tpr, per) for last, tpr, per in FORWARD_LADDER if units <= last)


def grad_kernel(units):
  """... of the gradient's, or WIDE."""
  assert 1 <= units <= K['kNormActMaxUnits'], units
  if units > K['kHeldUnits']:
    return WIDE
  return next((tpr, per) for last, tpr, per in HELD_LADDER if units <= last)


def rows_per_workgroup(units):
  return K['kBlock'] // K['kWave'] if units <= K['kNormActWaveUnits'] else 1


def forward_pass(units):
  """Rows of one pass of the forward's grid-stride loop."""
  return K['kMaxBlocks'] * rows_per_workgroup(units)


def grad_pass(units):
  return K['kNormActMaxPartials'] * rows_per_workgroup(units)


def partial_rows(rows, units):
  """norm_act_partials of csrc/norm_act.h: workgroups of the gradient launch."""
  return min(-(-rows // rows_per_workgroup(units)), K['kNormActMaxPartials'])


def vectorises(width, kind):
  """Whether a row (norm) or a block (gate) of `width` values is whole 16-byte chunks."""
  return width % (8 if kind == 'bf16' else 4) == 0


# --- A: off-alignment views, norm_act ------------------------------------------------
# one width per rung of both ladders that vectorises in both dtypes; 8200 is the
# streamed gradient and the forward's workgroup of 1024 with a ragged last chunk
A_UNITS = (8, 512, 1024, 2048, 4096, 8192, 8200, 16384)
A_ROWS = 9
NORM_POINTERS = ('x', 'out', 'scale', 'shift', 'gout', 'dx', 'partials')


def a_case(units, kind):
  """(impl, act) in turn: every width runs both impls (one per dtype), every impl every activation."""
  i = A_UNITS.index(units)
  return norms.IMPLS[(i + KINDS.index(kind)) % 2], norms.ACTS[(i // 2 + i) % 4]


# --- B: off-alignment views, gru_gate -------------------------------------------------
# (deter, blocks): h = 1; h = 4 and 12 (16 bytes of float32, not of bfloat16); h = 24
# (both, and no power of two: a 16-byte item must not straddle a block); the model's h = 8
B_SHAPES = ((8, 8), (16, 4), (48, 4), (48, 2), (64, 8))
B_H = (1, 4, 12, 24, 8)
B_VECTORISES = {'f32': (False, True, True, True, True), 'bf16': (False, False, False, True, True)}
B_ROWS = (1, 3, 37)
GATE_POINTERS = ('x', 'deter', 'out', 'gout', 'dx', 'ddeter')
B_STRIDED = gates.STRIDED                          # per-element from an x one element in: 2.1 M items

# --- C: past one pass of the grid, norm_act --------------------------------------------
DISTINCT = 304                                     # >= norms.SUM_ROWS: the small run's column sums are held too
# (2051, 4096) is the one rung, 16 values on each of 256 threads, that the others leave out
C_FORWARD = ((8195, 3), (8195, 512), (8195, 1024), (2051, 1025), (2051, 4096), (2051, 4097), (2051, 8192), (2051, 8193))
C_WAVE_GRAD = ((2051, 3), (2051, 512), (2051, 1024))
C_BLOCK_GRAD = ((1027, 1025), (1027, 8192), (1027, 8193), (1027, 16384))
C_SHAPES = C_FORWARD + C_WAVE_GRAD + C_BLOCK_GRAD  # every one runs forward and gradient in one call
# bfloat16 at one shape per kernel family: a wave per row (forward and gradient), a
# workgroup of 256 per row (forward; the gradient that holds its row, 5 rows per
# workgroup), the forward's workgroup of 1024 with the gradient that streams, and
# the held workgroup gradient at its widest with a third row
C_BF16 = ((8195, 512), (2051, 4097), (2051, 8193), (1027, 8192))


def c_case(rows, units):
  i = C_SHAPES.index((rows, units))
  return norms.IMPLS[i % 2], norms.ACTS[(i // 2 + i) % 4]


def c_kinds(rows, units):
  return KINDS if (rows, units) in C_BF16 else ('f32',)


def multiplicity(rows, distinct=DISTINCT):
  """How often distinct row r is among rows 0 .. rows - 1 of the tiled input (row i is i % distinct)."""
  return rows // distinct + (np.arange(distinct) < rows % distinct)


# --- D: null outputs --------------------------------------------------------------------
D_SHAPES = ((301, 65), (301, 1024), (515, 2048), (515, 8200))
D_GATE_SHAPES = ((12, 4), (64, 8))
D_GATE_ROWS = 37


def d_case(rows, units, impl, kind):
  return norms.ACTS[(D_SHAPES.index((rows, units)) + norms.IMPLS.index(impl) + 2 * KINDS.index(kind)) % 4]


# --- E: nothing else is written -----------------------------------------------------------
E_UNITS = (1, 7, 65, 1023, 1025, 2047, 4099, 8191, 8193, 12291, 16383)
# All of E_UNITS are odd and go element by element wherever they start.  The 16- and
# 32-byte stores of Map::store_part are behind `at < units`; these widths take them
# (from the aligned start) with a last chunk that is not the last thread's, one per
# rung, and 16 384 with none to spare.
E_UNITS_VEC = (8, 520, 1032, 2056, 4104, 8200, 16384)
E_ROWS = 3
E_MARGIN = 16                                      # elements on both sides of every output, at least
E_STARTS = (E_MARGIN, E_MARGIN + 1)                # a multiple of 16 bytes in both dtypes, and not
FILL = 7.0


def e_case(units):
  i = (E_UNITS + E_UNITS_VEC).index(units)
  return norms.IMPLS[i % 2], norms.ACTS[(i // 2 + i) % 4]


# --- inputs ---------------------------------------------------------------------------------
_INPUTS = {}


def _frozen(d):
  for a in d.values():
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return d


def norm_inputs(rows, units, impl, kind='f32'):
  """`norms.inputs_of` with scale and shift, x and gout bfloat16-rounded for
  kind 'bf16'; made once and left unchanged."""
  key = ('norm', rows, units, impl, kind)
  if key not in _INPUTS:
    rng = np.random.default_rng([SEED, rows, units, norms.IMPLS.index(impl)])
    inp = norms.inputs_of(rows, units, impl, True, 1.0, rng)
    if kind == 'bf16':
      inp = dict(inp, x=norms.bf16_round(inp['x']), gout=norms.bf16_round(inp['gout']))
    _INPUTS[key] = _frozen(inp)
  return _INPUTS[key]


def gate_inputs(rows, deter, blocks, kind='f32'):
  key = ('gate', rows, deter, blocks, kind)
  if key not in _INPUTS:
    inp = gates.inputs_of(rows, deter, 1.0, np.random.default_rng([SEED, rows, deter, blocks]))
    if kind == 'bf16':
      inp = {k: gates.bf16_round(v) for k, v in inp.items()}
    _INPUTS[key] = _frozen(inp)
  return _INPUTS[key]


def norm_reference(inp, impl, act):
  return norms.reference64(inp['x'], inp['scale'], inp['shift'], impl, act, EPS, inp['gout'])


def tiled_sums(inp, impl, act, rows):
  """The float64 column sums of the `rows`-row input whose row i is distinct row
  i % len(x): dscale, dshift and the sums of |terms| their bars are taken from.
  Every term is linear in its row's gout, and a float32 gout times a small
  integer is exact in float64, so the sums weighted by each distinct row's
  multiplicity are `reference64` of gout * multiplicity."""
  weight = multiplicity(rows, len(inp['x'])).astype(np.float64)[:, None]
  ref = norms.reference64(inp['x'], inp['scale'], inp['shift'], impl, act, EPS, inp['gout'].astype(np.float64) * weight)
  return {key: ref[key] for key in ('dscale', 'dshift', 'dscale_abs', 'dshift_abs')}


def norm_ratios(got, want, inp, bf16, sums=None):
  """Shares of the bars of tests/norm_act_cases.py: out, dx, and with `sums` (the
  float64 column sums to hold dscale and dshift to) those two."""
  s = norms.row_scale(inp['gout'], inp['scale'], want['rstd'])
  ratios = {'out': norms.out_ratio(got['out'], want['out'], bf16), 'dx': norms.grad_ratio(got['dx'], want['dx'], s, bf16)}
  if sums is not None:
    ratios['dscale'] = norms.sum_ratio(got['dscale'], sums['dscale'], sums['dscale_abs'])
    ratios['dshift'] = norms.sum_ratio(got['dshift'], sums['dshift'], sums['dshift_abs'])
  return ratios


def gate_ratios(got, want, inp, bf16):
  s = gates.row_scale(inp['gout'], inp['x'], inp['deter'])
  return {'out': gates.out_ratio(got['out'], want['out'], bf16), 'dx': gates.grad_ratio(got['dx'], want['dx'], s, bf16),
          'ddeter': gates.grad_ratio(got['ddeter'], want['ddeter'], s, bf16)}
