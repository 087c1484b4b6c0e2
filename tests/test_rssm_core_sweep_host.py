"""What tests/test_gpu_rssm_core_sweep.py relies on, shown without a GPU: the
tables of tests/rssm_core_sweep_cases.py reach the paths they name, by the
constants and width ladders of csrc/norm_act.hip, csrc/norm_act.h and
csrc/gru_gate.hip as the source spells them (a later change to one of them
fails here instead of quietly unsweeping a path); the multiplicity-weighted
float64 column sums are those of the tiled rows; and the float32 definition
stays inside every bar at every input the GPU tests hold to one.  CPU only."""
import numpy as np
import pytest

from embodied_amd import nets
from tests import gru_gate_cases as gates
from tests import norm_act_cases as norms
from tests import rssm_core_sweep_cases as sweep

K, G = sweep.K, sweep.G


def test_constants_and_ladders_are_the_ones_the_tables_were_made_for():
  assert K == {'kWave': 64, 'kBlock': 256, 'kMaxBlocks': 2048, 'kHeldUnits': 8192, 'kNormActMaxUnits': 16384,
               'kNormActWaveUnits': 1024, 'kNormActMaxPartials': 512}
  assert G == {'kThreads': 256, 'kMaxBlocks': 2048}
  assert sweep.FORWARD_LADDER == [(512, 64, 8), (1024, 64, 16), (2048, 256, 8), (4096, 256, 16), (8192, 256, 32),
                                  (16384, 1024, 16)]
  assert sweep.HELD_LADDER == sweep.FORWARD_LADDER[:5]
  for ladder in (sweep.FORWARD_LADDER, sweep.HELD_LADDER):
    for last, tpr, per in ladder:
      assert tpr * per >= last                       # the row fits the registers of its threads
      assert (tpr == K['kWave']) == (last <= K['kNormActWaveUnits'])
  assert (sweep.forward_pass(1024), sweep.forward_pass(1025)) == (8192, 2048)
  assert (sweep.grad_pass(1024), sweep.grad_pass(1025)) == (2048, 512)
  assert norms.MAX_UNITS == K['kNormActMaxUnits'] == nets.NORM_ACT_MAX_UNITS
  # the facade's count of partial sums is the model's
  for rows in (1, 3, 9, 301, 304, 515, 1027, 2051, 8195):
    for units in (1, 3, 1024, 1025, 8192, 8193, 16384):
      assert nets._partial_floats(rows, units) == 2 * sweep.partial_rows(rows, units) * units


def test_A_widths_vectorise_in_both_dtypes_on_every_rung():
  assert {sweep.forward_kernel(u) for u in sweep.A_UNITS} == {(tpr, per) for _, tpr, per in sweep.FORWARD_LADDER}
  assert {sweep.grad_kernel(u) for u in sweep.A_UNITS} == {(tpr, per) for _, tpr, per in sweep.HELD_LADDER} | {sweep.WIDE}
  for units in sweep.A_UNITS:
    assert units % 8 == 0 and all(sweep.vectorises(units, kind) for kind in sweep.KINDS)
  # 8200: the streamed gradient and the forward's workgroup of 1024, a last chunk that is not whole rounds of the threads
  assert sweep.grad_kernel(8200) == sweep.WIDE and sweep.forward_kernel(8200) == (1024, 16)
  assert 8200 % (1024 * 4) and 8200 % (K['kBlock'] * 4) and 8200 % (K['kBlock'] * 8)
  for kind in sweep.KINDS:                           # both impls at every width, every activation under every impl
    assert {sweep.a_case(u, kind)[0] for u in sweep.A_UNITS} == set(norms.IMPLS)
  for units in sweep.A_UNITS:
    assert {sweep.a_case(units, kind)[0] for kind in sweep.KINDS} == set(norms.IMPLS)
  for impl in norms.IMPLS:
    assert {a for u in sweep.A_UNITS for k in sweep.KINDS for i, a in [sweep.a_case(u, k)] if i == impl} == set(norms.ACTS)
  assert sweep.A_ROWS == 9 and sweep.NORM_POINTERS == ('x', 'out', 'scale', 'shift', 'gout', 'dx', 'partials')


def test_B_shapes_have_the_stated_h_and_vectorisation_split():
  assert sweep.B_SHAPES == ((8, 8), (16, 4), (48, 4), (48, 2), (64, 8)) and sweep.B_ROWS == (1, 3, 37)
  for i, (deter, blocks) in enumerate(sweep.B_SHAPES):
    assert deter % blocks == 0 and deter // blocks == sweep.B_H[i]
    for kind in sweep.KINDS:
      assert sweep.vectorises(deter // blocks, kind) == sweep.B_VECTORISES[kind][i], (deter, blocks, kind)
  assert sweep.B_H == (1, 4, 12, 24, 8)
  assert sweep.B_VECTORISES['f32'] == (False, True, True, True, True)
  assert sweep.B_VECTORISES['bf16'] == (False, False, False, True, True)
  assert 24 & 23                                     # h = 24 is no power of two
  # one element in, STRIDED goes element by element: an item is one output
  rows, deter, blocks = sweep.B_STRIDED
  per_pass = G['kMaxBlocks'] * G['kThreads']
  assert per_pass == 524288 and rows * deter == 2129920 > 4 * per_pass
  assert all(sweep.vectorises(deter // blocks, kind) for kind in sweep.KINDS)      # aligned, it does not
  assert set(sweep.D_GATE_SHAPES) == {(12, 4), (64, 8)} and sweep.D_GATE_ROWS == 37


def test_C_shapes_pass_one_sweep_of_the_kernel_they_name():
  assert sweep.DISTINCT == 304 >= norms.SUM_ROWS
  assert len(set(sweep.C_SHAPES)) == len(sweep.C_SHAPES) == 15
  for rows, units in sweep.C_FORWARD:
    assert rows > sweep.forward_pass(units), (rows, units)
  assert {sweep.forward_kernel(u) for _, u in sweep.C_FORWARD} == {(tpr, per) for _, tpr, per in sweep.FORWARD_LADDER}
  for rows, units in sweep.C_WAVE_GRAD:
    assert units <= K['kNormActWaveUnits'] and rows > sweep.grad_pass(units) == 2048, (rows, units)
    assert sweep.partial_rows(rows, units) == K['kNormActMaxPartials']
  assert {sweep.grad_kernel(u) for _, u in sweep.C_WAVE_GRAD} == {(64, 8), (64, 16)}
  for rows, units in sweep.C_BLOCK_GRAD:
    assert units > K['kNormActWaveUnits'] and sweep.partial_rows(rows, units) == K['kNormActMaxPartials']
    # workgroup b takes rows b, b + 512, b + 1024: the first three take a third
    assert rows == 1027 and -(-rows // sweep.grad_pass(units)) == 3 and rows - 2 * sweep.grad_pass(units) == 3
  assert {sweep.grad_kernel(u) for _, u in sweep.C_BLOCK_GRAD} == {(256, 8), (256, 32), sweep.WIDE}
  for rows, units in sweep.C_SHAPES:                 # and every shape's gradient takes a second row somewhere
    assert rows > sweep.grad_pass(units) and rows > sweep.DISTINCT
  # bfloat16: every kernel family
  assert set(sweep.C_BF16) <= set(sweep.C_SHAPES)
  assert {sweep.forward_kernel(u)[0] for _, u in sweep.C_BF16} == {64, 256, 1024}
  families = {sweep.grad_kernel(u) if sweep.grad_kernel(u) == sweep.WIDE else sweep.grad_kernel(u)[0] for _, u in sweep.C_BF16}
  assert families == {64, 256, sweep.WIDE}
  assert {sweep.c_case(*shape)[0] for shape in sweep.C_SHAPES} == set(norms.IMPLS)
  assert {sweep.c_case(*shape)[1] for shape in sweep.C_SHAPES} == set(norms.ACTS)
  for rows in (304, 305, 1027, 2051, 8195):
    m = sweep.multiplicity(rows)
    assert m.sum() == rows and np.array_equal(m, np.bincount(np.arange(rows) % sweep.DISTINCT, minlength=sweep.DISTINCT))


def test_D_and_E_tables():
  assert sweep.D_SHAPES == ((301, 65), (301, 1024), (515, 2048), (515, 8200))
  assert all(rows >= norms.SUM_ROWS for rows, _ in sweep.D_SHAPES)
  assert {sweep.grad_kernel(u) for _, u in sweep.D_SHAPES} == {(64, 8), (64, 16), (256, 8), sweep.WIDE}
  acts = {sweep.d_case(r, u, impl, kind) for r, u in sweep.D_SHAPES for impl in norms.IMPLS for kind in sweep.KINDS}
  assert acts == set(norms.ACTS)
  assert sweep.E_UNITS == (1, 7, 65, 1023, 1025, 2047, 4099, 8191, 8193, 12291, 16383) and sweep.E_ROWS == 3
  assert not any(sweep.vectorises(u, 'f32') for u in sweep.E_UNITS)
  assert all(sweep.vectorises(u, kind) for u in sweep.E_UNITS_VEC for kind in sweep.KINDS)
  assert {sweep.forward_kernel(u) for u in sweep.E_UNITS_VEC} == {(tpr, per) for _, tpr, per in sweep.FORWARD_LADDER}
  assert {sweep.forward_kernel(u) for u in sweep.E_UNITS} == {(64, 8), (64, 16), (256, 8), (256, 32), (1024, 16)}
  assert {sweep.grad_kernel(u) for u in sweep.E_UNITS_VEC} == {(tpr, per) for _, tpr, per in sweep.HELD_LADDER} | {sweep.WIDE}
  assert sweep.E_MARGIN >= 16 and min(sweep.E_STARTS) >= sweep.E_MARGIN
  for size in (4, 2):                                # one start on 16 bytes, one off it, float32 and bfloat16
    assert [start * size % 16 == 0 for start in sweep.E_STARTS] == [True, False]


def test_weighted_column_sums_are_the_sums_over_the_tiled_rows():
  for impl, act, rows in (('layer', 'gelu', 41), ('rms', 'silu', 23)):
    inp = sweep.norm_inputs(7, 65, impl)
    tiled = {k: (v[np.arange(rows) % 7] if k in ('x', 'gout') else v) for k, v in inp.items()}
    brute = sweep.norm_reference(tiled, impl, act)
    fast = sweep.tiled_sums(inp, impl, act, rows)
    for key in ('dscale', 'dshift', 'dscale_abs', 'dshift_abs'):
      assert np.allclose(fast[key], brute[key], rtol=1e-12, atol=1e-13), (impl, key)
    assert not np.allclose(fast['dscale'], sweep.tiled_sums(inp, impl, act, rows + 1)['dscale'])


def _float32(inp, impl, act):
  return norms.evaluate(inp['x'], inp['scale'], inp['shift'], impl, act, sweep.EPS, inp['gout'], dtype=np.float32)


def _float32_tiled_sums(inp, impl, act, rows):
  """dscale and dshift of the float32 definition, its terms row by row (a one-row
  column sum is the row's terms) tiled and summed in float32 over the tiled rows."""
  one = [norms.evaluate(inp['x'][r:r + 1], inp['scale'], inp['shift'], impl, act, sweep.EPS, inp['gout'][r:r + 1], np.float32)
         for r in range(len(inp['x']))]
  index = np.arange(rows) % len(inp['x'])
  sums = {}
  for key in ('dscale', 'dshift'):
    terms = np.stack([o[key] for o in one])
    assert terms.dtype == np.float32
    sums[key] = terms[index].sum(0, dtype=np.float32)
  return sums


@pytest.mark.parametrize('rows,units', sweep.C_SHAPES)
def test_float32_definition_sits_inside_all_four_bars_at_the_inputs_of_C(rows, units):
  impl, act = sweep.c_case(rows, units)
  for kind in sweep.c_kinds(rows, units):
    inp = sweep.norm_inputs(sweep.DISTINCT, units, impl, kind)
    want, got = sweep.norm_reference(inp, impl, act), _float32(inp, impl, act)
    small = sweep.norm_ratios(got, want, inp, False, sums=want)
    big = sweep.norm_ratios(dict(got, **_float32_tiled_sums(inp, impl, act, rows)), want, inp, False,
                            sums=sweep.tiled_sums(inp, impl, act, rows))
    print(f'{rows} x {units} {impl} {act} {kind}: the float32 definition, {sweep.DISTINCT} rows',
          {k: round(v, 4) for k, v in small.items()}, 'tiled', {k: round(big[k], 4) for k in ('dscale', 'dshift')})
    assert max(small.values()) <= 1.0 and max(big.values()) <= 1.0, (small, big)


@pytest.mark.parametrize('rows,units', sweep.D_SHAPES)
def test_float32_definition_sits_inside_all_four_bars_at_the_inputs_of_D(rows, units):
  for impl in norms.IMPLS:
    for kind in sweep.KINDS:
      act = sweep.d_case(rows, units, impl, kind)
      inp = sweep.norm_inputs(rows, units, impl, kind)
      want = sweep.norm_reference(inp, impl, act)
      ratios = sweep.norm_ratios(_float32(inp, impl, act), want, inp, False, sums=want)
      print(f'{rows} x {units} {impl} {act} {kind}: the float32 definition', {k: round(v, 4) for k, v in ratios.items()})
      assert max(ratios.values()) <= 1.0, ratios


def test_float32_definition_sits_inside_the_bars_at_the_inputs_of_A_B_and_E():
  """out and dx only: 9 and 3 rows are fewer than `norms.SUM_ROWS`."""
  worst = {}
  for units in sweep.A_UNITS + sweep.E_UNITS + sweep.E_UNITS_VEC:
    for kind in sweep.KINDS:
      rows, (impl, act) = (sweep.A_ROWS, sweep.a_case(units, kind)) if units in sweep.A_UNITS else (sweep.E_ROWS, sweep.e_case(units))
      inp = sweep.norm_inputs(rows, units, impl, kind)
      ratios = sweep.norm_ratios(_float32(inp, impl, act), sweep.norm_reference(inp, impl, act), inp, False)
      assert max(ratios.values()) <= 1.0, (units, kind, ratios)
      worst = {k: max(v, worst.get(k, 0.0)) for k, v in ratios.items()}
  for deter, blocks in sweep.B_SHAPES + sweep.D_GATE_SHAPES:
    for rows in sweep.B_ROWS:
      for kind in sweep.KINDS:
        inp = sweep.gate_inputs(rows, deter, blocks, kind)
        got = gates.evaluate(inp['x'], inp['deter'], blocks, inp['gout'], dtype=np.float32)
        ratios = sweep.gate_ratios(got, gates.reference64(inp['x'], inp['deter'], blocks, inp['gout']), inp, False)
        assert max(ratios.values()) <= 1.0, (deter, blocks, rows, kind, ratios)
        worst.update({'gate ' + k: max(v, worst.get('gate ' + k, 0.0)) for k, v in ratios.items()})
  print('the float32 definition, worst share of each bar:', {k: round(v, 4) for k, v in sorted(worst.items())})
