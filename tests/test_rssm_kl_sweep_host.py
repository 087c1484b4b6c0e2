"""What tests/test_gpu_rssm_kl_sweep.py relies on, shown without a GPU: the
sweep of tests/rssm_kl_sweep_cases.py covers the kernels' ladder as the source
spells it, the float32 definition stays inside both bars at every one of its
inputs (so the bars leave room for another reduction order and no more), and
no row's kl sits so close to free_nats that float32 could put the maximum's
gradient on the other side.  CPU only."""
import numpy as np
import pytest
import torch

from tests import rssm_kl_cases as cases
from tests import rssm_kl_sweep_cases as sweep

RUNG_IDS = [f'W{W}x{nper}' for W, nper in sweep.RUNGS]


def test_width_is_the_ladder_of_the_source_and_the_sweep_covers_it():
  ladder = sweep.source_ladder()
  assert [(W, nper) for _, W, nper in ladder] == list(sweep.RUNGS)
  assert ladder[-1][0] == sweep.MAX_CLASSES == 256 and sweep.WAVE == 64 and sweep.K['kWaves'] == 4
  first = 1
  for last, W, nper in ladder:
    assert W * nper >= last and sweep.WAVE % W == 0
    for classes in range(first, last + 1):
      assert sweep.width(classes) == (W, nper), classes
    # the rung's first class count, its last (here or in FUSED_SHAPES) and nothing of another rung
    counts = sweep.CLASSES[W, nper]
    older = [c for _, c in cases.FUSED_SHAPES]
    assert all(first <= c <= last for c in counts) and list(counts) == sorted(set(counts))
    assert counts[0] == first or first in older
    assert counts[-1] == last or last in older and counts[-1] == last - 1
    # where a slot j of NPER starts (lane 0 alone) and where it is full
    for j in range(1, nper):
      assert W * j + 1 < first or W * j + 1 in counts, (W, nper, j)
      assert W * j < first or W * j in counts, (W, nper, j)
    first = last + 1
  assert first == sweep.MAX_CLASSES + 1
  for classes in range(1, sweep.MAX_CLASSES + 1):                 # 1 .. 256, nothing else
    assert sweep.width(classes) in sweep.RUNGS
  for bad in (0, 257):
    with pytest.raises(AssertionError):
      sweep.width(bad)
  swept = sweep.all_shapes()
  assert len(swept) == len(set(swept))
  for classes in sweep.SHIPPED_CLASSES:
    assert (sweep.SHIPPED_STOCH, classes) in swept, classes
  for rung in sweep.RUNGS:
    k = sweep.segments(rung)
    for classes in sweep.CLASSES[rung]:
      assert {1, k, k + 1, 2 * k + 1} <= {s for s, c in swept if c == classes}, classes
      assert (sweep.control_stoch(classes), classes) in swept and sweep.control_stoch(classes) % k == 1 % k
  # what the suite did not run before: W = 16 whole, 48 classes, the NPER tails, one class
  for shape in ((32, 16), (5, 9), (5, 15), (32, 48), (33, 1), (2, 65), (2, 129), (2, 192), (2, 193)):
    assert shape in swept, shape
  assert sweep.ROWS == (1, 5) and sweep.FREE_NATS == (1.0, 0.0)
  assert sweep.SETTINGS == ((0.01, 1.0), (0.01, 5.0), (0.0, 0.1), (0.0, 1.0))


@pytest.mark.parametrize('rung', sweep.RUNGS, ids=RUNG_IDS)
def test_float32_definition_sits_inside_both_bars_at_every_sweep_input(rung):
  """Every shape of the rung, rows 1 and 5, float32 and bfloat16-rounded
  inputs, every (unimix, scale) of the sweep, free_nats 1 and 0: the composed
  arithmetic in float32 on the CPU against float64, as shares of the forward
  bar 1e-5 + 1e-5 |want| and the gradient bar 1e-5 |g| (1 + |want|); and no
  row's float64 kl within FREE_MARGIN of free_nats = 1."""
  worst = [0.0, 0.0]
  nearest = np.inf
  below = above = 0
  for stoch, classes in sweep.shapes(rung):
    for rows in sweep.ROWS:
      for kind in sweep.KINDS:
        for unimix, scale in sweep.SETTINGS:
          d = sweep.data(stoch, classes, rows, scale, kind)
          for free in sweep.FREE_NATS:
            want = cases.reference64(d['post'], d['prior'], unimix, free, d['g_dyn'], d['g_rep'])
            got = cases.restate(d['post'], d['prior'], unimix, free, d['g_dyn'], d['g_rep'], torch.float32)
            forward = max(cases.forward_ratio(got[k], want[k]) for k in ('kl', 'dyn', 'rep', 'ent_post', 'ent_prior'))
            grad = max(cases.grad_ratio(got['grad_post'], want['grad_post'], d['g_rep']),
                       cases.grad_ratio(got['grad_prior'], want['grad_prior'], d['g_dyn']))
            assert forward <= 1.0 and grad <= 1.0, (stoch, classes, rows, kind, unimix, scale, free, forward, grad)
            worst = [max(worst[0], forward), max(worst[1], grad)]
          gap = np.abs(want['kl'] - 1.0)
          assert (gap > sweep.FREE_MARGIN).all(), (stoch, classes, rows, kind, unimix, scale, want['kl'])
          nearest = min(nearest, float(gap.min()))
          below += int((want['kl'] < 1.0).sum())
          above += int((want['kl'] > 1.0).sum())
  print(f'W = {rung[0]}, NPER = {rung[1]}: the float32 definition is {worst[0]:.3g} of the forward bar and '
        f'{worst[1]:.3g} of the gradient bar; the kl nearest to free_nats = 1 is {nearest:.3g} away; '
        f'{below} rows below it, {above} above')
  assert below and above                            # the maximum's gradient is taken on both sides
