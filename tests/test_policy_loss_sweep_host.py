"""What tests/test_gpu_policy_loss_sweep.py relies on, shown without a GPU: the
sweep of tests/policy_loss_sweep_cases.py covers the kernels' ladder as the
source spells it, and the float32 definition stays inside the forward bar and
the gradient bar of tests/test_gpu_policy_loss.py at every one of its inputs
(so the bars leave room for another reduction order and no more).  CPU only."""
import numpy as np
import pytest
import torch

from tests import policy_loss_cases as cases
from tests import policy_loss_sweep_cases as sweep

RUNG_IDS = [f'W{W}x{nper}' for W, nper in sweep.RUNGS]


def test_width_is_the_ladder_of_the_source_and_the_sweep_covers_it():
  ladder = sweep.source_ladder()
  assert [(W, nper) for _, W, nper in ladder] == list(sweep.RUNGS) and len(ladder) == 8
  assert ladder[-1][0] == sweep.max_classes() == sweep.MAX_CLASSES == 256
  assert sweep.WAVE == 64 and sweep.K['kWaves'] == 4 and sweep.SWEEP == sweep.K['kMaxBlocks'] * 4 == 8192
  first = 1
  for last, W, nper in ladder:
    assert W * nper >= last and sweep.WAVE % W == 0
    for classes in range(first, last + 1):
      assert sweep.width(classes) == (W, nper), classes
    counts = sweep.CLASSES[W, nper]
    assert counts and list(counts) == sorted(set(counts)) and sweep.shapes((W, nper))       # every rung has shapes
    assert counts[0] == first and counts[-1] == last
    # where a slot j of NPER starts (lane 0 alone), where it is full, and the count before that
    for j in range(1, nper):
      assert W * j + 1 < first or W * j + 1 in counts, (W, nper, j)
      assert W * j < first or W * j in counts, (W, nper, j)
    assert nper == 1 or last - 1 in counts
    first = last + 1
  assert first == sweep.MAX_CLASSES + 1
  for classes in range(1, sweep.MAX_CLASSES + 1):                 # 1 .. 256, nothing else
    assert sweep.width(classes) in sweep.RUNGS
  for bad in (0, 257):
    with pytest.raises(AssertionError):
      sweep.width(bad)
  swept = sweep.all_shapes()
  assert len(swept) == len(set(swept))
  for rung in sweep.RUNGS:
    k = sweep.segments(rung)
    for classes in sweep.CLASSES[rung]:
      assert {1, k, k + 1, 2 * k + 1} <= {g for g, c in swept if c == classes}, classes
      assert (sweep.control_groups(classes), classes) in swept and sweep.control_groups(classes) % k == 1 % k
    assert (0, sweep.CLASSES[rung][0]) in swept                   # no group axis
  # what the suite did not run before: W = 16 whole, full segments, the rung edges, more than one
  # iteration of the g0 loop at W = 4, 8, 16
  for shape in ((5, 9), (5, 16), (17, 4), (33, 3), (9, 8), (17, 7), (9, 15), (3, 17), (5, 32), (2, 33), (2, 65), (2, 128),
                (2, 129), (2, 192), (2, 193), (2, 255), (65, 1)):
    assert shape in swept, shape
  assert sweep.GEOMETRIES == ((1, 2, 1), (5, 2, 1), (2, 4, 1), (5, 1, 0)) and sweep.ALONE in sweep.GEOMETRIES
  assert any(u == 0 and s >= 1 for u, s in sweep.SETTINGS) and any(u > 0 and s >= 1 for u, s in sweep.SETTINGS)
  for geometry in sweep.GEOMETRIES:                               # both layouts of weight, everywhere
    assert {sweep.cut_weight(*geometry, *setting) for setting in sweep.SETTINGS} == {False, True}
  for setting in sweep.SETTINGS:
    assert {sweep.cut_weight(*geometry, *setting) for geometry in sweep.GEOMETRIES} == {False, True}
  # past one pass of the capped grid, in the forward's rows and in the gradient's
  assert sweep.PAST_N * (sweep.PAST_T - sweep.PAST_DROP) > sweep.SWEEP and sweep.PAST_N * sweep.PAST_T > sweep.SWEEP
  assert {sweep.width(c) for _, c in sweep.PAST_SHAPES} == {(8, 1), (64, 2)}


def test_the_inputs_are_what_the_sweep_says():
  d = sweep.data(3, 5, 5, 2, 1, 1.0)
  assert d['logits'].shape == (5, 2, 3, 5) and d['act'].shape == (5, 2, 3) and d['act'].dtype == np.int32
  assert d['adv'].shape == d['gout'].shape == (5, 1) and d['weight'].shape == (5, 2)
  assert list(d['act'].reshape(-1)[:4]) == [0, 4, -1, 5]
  assert (d['weight'] == 0).any() and (d['weight'] != 0).any()           # some weights are 0
  assert sweep.data(0, 5, 5, 2, 1, 1.0)['logits'].shape == (5, 2, 5)
  rounded = sweep.data(3, 5, 5, 2, 1, 1.0, 'bf16')['logits']
  assert np.array_equal(rounded, cases.bf16_round(rounded)) and not np.array_equal(rounded, d['logits'])
  assert sweep.data(3, 5, 5, 2, 1, 1.0) is d and not d['logits'].flags.writeable
  for classes in (1, 5, 65, 256):
    h = sweep.hit_data(classes, 1.0)
    groups = sweep.control_groups(classes)
    assert h['logits'].shape == (classes + 2, 1, groups, classes) and h['act'].shape == (classes + 2, 1, groups)
    assert (h['act'] == (np.arange(classes + 2) - 1)[:, None, None]).all() and (h['weight'] != 0).all()


@pytest.mark.parametrize('rung', sweep.RUNGS, ids=RUNG_IDS)
def test_float32_definition_sits_inside_both_bars_at_every_sweep_input(rung):
  """Every shape of the rung, every geometry, float32 and bfloat16-rounded
  logits, every (unimix, scale) of the sweep, and the hit-lane inputs: the
  restated arithmetic in float32 on the CPU against float64, as shares of the
  forward bar 1e-5 + 1e-5 |want| and the gradient bar 1e-5 (s + |want|)."""
  worst = [0.0, 0.0]
  count = 0
  for groups, classes in sweep.shapes(rung):
    assert sweep.width(classes) == rung
    for n, t, drop in sweep.GEOMETRIES:
      for kind in sweep.KINDS:
        for unimix, scale in sweep.SETTINGS:
          d = sweep.data(groups, classes, n, t, drop, scale, kind)
          got = cases.restate(d['logits'], d['act'], d['adv'], d['weight'], sweep.ACTENT, unimix, d['dims'], drop,
                              d['gout'], dtype=torch.float32)
          pair = sweep.ratios(d, got, got['grad'], sweep.reference(d, unimix))
          assert max(pair) <= 1.0, (groups, classes, n, t, drop, kind, unimix, scale, pair)
          worst = [max(a, b) for a, b in zip(worst, pair)]
          count += 1
  for classes in sweep.CLASSES[rung]:
    for unimix in (0.01, 0.0):
      d = sweep.hit_data(classes, 1.0)
      got = cases.restate(d['logits'], d['act'], d['adv'], d['weight'], sweep.ACTENT, unimix, 1, 0, d['gout'],
                          dtype=torch.float32)
      pair = sweep.ratios(d, got, got['grad'], sweep.reference(d, unimix))
      assert max(pair) <= 1.0, ('hit', classes, unimix, pair)
      worst = [max(a, b) for a, b in zip(worst, pair)]
      count += 1
  print(f'W = {rung[0]}, NPER = {rung[1]}: the float32 definition is {worst[0]:.3g} of the forward bar and '
        f'{worst[1]:.3g} of the gradient bar over {count} inputs')


def test_float32_definition_past_one_sweep_of_the_grid():
  unimix, scale = sweep.PAST_SETTING
  for groups, classes in sweep.PAST_SHAPES:
    for kind in sweep.KINDS:
      d = sweep.data(groups, classes, sweep.PAST_N, sweep.PAST_T, sweep.PAST_DROP, scale, kind)
      got = cases.restate(d['logits'], d['act'], d['adv'], d['weight'], sweep.ACTENT, unimix, 1, sweep.PAST_DROP, d['gout'],
                          dtype=torch.float32)
      pair = sweep.ratios(d, got, got['grad'], sweep.reference(d, unimix))
      print(f'{groups}x{classes} {kind}, N = {sweep.PAST_N}: the float32 definition is {pair[0]:.3g} of the forward bar '
            f'and {pair[1]:.3g} of the gradient bar')
      assert max(pair) <= 1.0, (groups, classes, kind, pair)
