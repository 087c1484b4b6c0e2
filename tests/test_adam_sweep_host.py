"""The lists of tests/adam_sweep_cases.py as far as they go without a GPU: the
loops they are about exist in csrc/optim.hip, the lists exceed the kernels'
constants, the clip regime sits where a kernel that stopped after its first pass
would decide the other way, the mixed list mixes, and the definition holds on
them: float32 inside every bar, float64 equal to `torch.optim.AdamW`.  CPU only."""
import numpy as np
import pytest
import torch

from tests import adam_cases as cases
from tests import adam_sweep_cases as sweep
from tests.optim_sweep_cases import SOURCE
from tests.test_adam_host import adamw_run_over

CASE_IDS = [sweep.tag(case) for case in sweep.CASES]


def _body(text, name):
  """The body of the kernel `name`, braces included, out of the source."""
  start = text.index(f'void {name}(')
  opened = text.index('{', text.index(')', start))
  depth = 0
  for at in range(opened, len(text)):
    depth += {'{': 1, '}': -1}.get(text[at], 0)
    if depth == 0:
      return text[opened:at + 1]
  raise AssertionError(name)


def test_the_loops_are_in_the_kernels_the_lists_are_about():
  text = SOURCE.read_text()
  for loop in ('chunk += gridDim.x', 'k += kThreads', 'k += kMetricThreads'):
    assert loop in text, loop
  adam = _body(text, 'optim_adam_update_kernel')
  assert 'optim_update_kernel' not in adam and 'adam_chunk<true>' in adam     # that kernel's body and no other
  assert 'k < n_chunks; k += kThreads' in adam                                # the global-norm sum: ALL chunks
  assert 'chunk < n_chunks; chunk += gridDim.x' in adam
  norms = _body(text, 'optim_norms_kernel')
  assert 'chunk < n_chunks; chunk += gridDim.x' in norms and 'norms_chunk<true, PARAMS>' in norms
  assert 'k < n_chunks; k += kMetricThreads' in _body(text, 'optim_metrics_kernel')
  assert 'optim_norms_kernel<false>' in text                                  # Adam's instantiation


def test_the_lists_exceed_the_constants_they_are_about():
  k, c = sweep.K, cases.C
  many, deep = sweep.LISTS['many'], sweep.LISTS['deep']
  assert len(many) == 2 * k['kMaxBlocks'] + 3 and all(1 <= int(np.prod(s.shape)) <= 5 for s in many)
  assert sweep.chunks(many) == len(many) > max(k['kMaxBlocks'], k['kMetricThreads'], k['kThreads'])
  assert {len(s.shape) for s in many} == {1, 2} and set(cases.mask_of(many)) == {False, True}
  sizes = [int(np.prod(s.shape)) for s in deep]
  assert sizes == [sweep.DEEP, 3, sweep.DEEP] and -(-sweep.DEEP // c) == k['kThreads'] + 2
  assert sweep.DEEP % c == 7                                               # a ragged last chunk
  assert (deep[0].poff, deep[0].goff, deep[1].poff) == (None, None, None)
  assert (deep[2].poff, deep[2].goff) == (1, 1)                            # head = 3: vectors behind scalars
  assert sweep.chunks(deep) == 2 * (k['kThreads'] + 2) + 1 > k['kThreads']
  assert set(cases.mask_of(deep)) == {False}
  assert sweep.STEPS == {'many': 4, 'deep': 2} and sweep.HYPERS['many'] == cases.COVER
  assert sweep.HYPERS['deep'] == (cases.Hyper(1e-2, 10.0, 0.1, 0, False), cases.Hyper(1e-2, 10.0, 0.1, 0, True))
  assert len(sweep.CASES) == 6 and sweep.EXEMPT == () and sweep.worst_ratios is cases.worst_ratios
  for name in sweep.LISTS:
    for bf16 in (False, True):
      inp = sweep.inputs(name, bf16)
      assert inp is sweep.inputs(name, bf16) and len(inp['g']) == sweep.STEPS[name]
      assert [x.shape for x in inp['p']] == [s.shape for s in sweep.LISTS[name]]
      assert all(x.dtype == np.float32 and not x.flags.writeable for x in inp['p'] + [x for g in inp['g'] for x in g])
      assert len(inp['bf16']) == len(sweep.LISTS[name])
  assert sweep.reference(sweep.CASES[-1]) is sweep.reference(sweep.CASES[-1])


def test_the_clip_regime_sits_on_the_later_loop_iterations():
  """From float64, per dtype variant: on every step of every case with the clip
  on the whole norm is at least MARGIN from the bound; on the clipped steps the
  part in the first pass alone (chunks < kMaxBlocks of `many`, chunks < kThreads
  of `deep`) is BELOW the bound by at least MARGIN, so a sum that lost the later
  iterations would not clip; both regimes occur in each list."""
  for name in sweep.LISTS:
    seen = set()
    clipped_steps = 0
    for h in sweep.HYPERS[name]:
      inp = sweep.inputs(name, h.bf16)
      for step, grads in enumerate(inp['g']):
        side, gap = cases.regime(grads, h.clip)
        assert (side == 'off') == (h.clip == 0.0)
        if side == 'off':
          continue
        assert gap >= cases.MARGIN, (name, h, step, side, gap)
        seen.add(side)
        if side == 'above':
          part = cases.global_norm(sweep.first_pass(name, grads))
          assert part < h.clip and (h.clip - part) / h.clip >= cases.MARGIN, (name, h, step, part)
          assert part > 0.0
          clipped_steps += 1
    assert seen == {'below', 'above'}, (name, seen)
    assert clipped_steps >= sum(1 for h in sweep.HYPERS[name] if h.clip)
  # the norms are the ones the lists state, to 3e-4 after the rounding to bfloat16
  for name in sweep.LISTS:
    for bf16 in (False, True):
      for grads, (whole, part) in zip(sweep.inputs(name, bf16)['g'], sweep.NORMS[name]):
        assert abs(cases.global_norm(grads) / whole - 1) < 3e-4
        assert part is None or abs(cases.global_norm(sweep.first_pass(name, grads)) / part - 1) < 3e-4
  first = sweep.first_pass('many', sweep.inputs('many', False)['g'][0])
  assert len(first) == sweep.BLOCKS
  assert sweep.first_pass('deep', sweep.inputs('deep', False)['g'][0])[0].size == sweep.K['kThreads'] * cases.C


def test_the_mixed_list_mixes_within_a_workgroup():
  blocks = sweep.BLOCKS
  flags = sweep.inputs('many', True)['bf16']
  assert flags == tuple(i % 3 == 0 for i in range(2 * blocks + 3)) and set(flags) == {False, True}
  differ = sum(flags[i] != flags[i + blocks] for i in range(blocks))
  assert differ > blocks // 2, differ
  assert set(sweep.inputs('many', False)['bf16']) == {False} and set(sweep.inputs('deep', False)['bf16']) == {False}
  assert set(sweep.inputs('deep', True)['bf16']) == {True}
  for name in sweep.LISTS:
    inp = sweep.inputs(name, True)
    for grads in inp['g']:
      rounded = [np.array_equal(g, cases.bf16_round(g).reshape(g.shape)) for g in grads]
      assert all(same for flag, same in zip(inp['bf16'], rounded) if flag)
      assert not any(same for flag, same in zip(inp['bf16'], rounded) if not flag)
  # the float32 tensors of the mixed list are the ones of the float32 list
  for step in range(sweep.STEPS['many']):
    plain, mixed = sweep.inputs('many', False)['g'][step], sweep.inputs('many', True)['g'][step]
    assert all(np.array_equal(a, b) for a, b, flag in zip(plain, mixed, flags) if not flag)


@pytest.mark.parametrize('case', sweep.CASES, ids=CASE_IDS)
def test_float32_definition_against_the_bars_on_the_sweep_lists(case):
  """`restate` in float32 on the CPU against its float64 run: the worst ratio
  per quantity, printed.  A (list, quantity) that misses must be in
  `sweep.EXEMPT`, which is empty."""
  name, i = case
  h = sweep.HYPERS[name][i]
  want = sweep.reference(case)
  got = cases.restate(sweep.inputs(name, h.bf16), h, sweep.LISTS[name], torch.float32)
  assert len(got) == len(want) == sweep.STEPS[name]
  worst = sweep.worst_ratios(got, want)
  for key in sorted(worst):
    print(f'float32 restated, {sweep.tag(case)}, {key}: {worst[key]:.3g} of its bar')
  missed = {(name, key) for key, value in worst.items() if value > 1.0}
  assert missed <= {entry[:2] for entry in sweep.EXEMPT}, worst


@pytest.mark.parametrize('case', sweep.CASES, ids=CASE_IDS)
def test_the_restatement_equals_an_independent_implementation_on_the_sweep_lists(case):
  """`restate` in float64 against torch's AdamW over hand-clipped gradients, p
  after every step, to 1e-12: the tie of tests/test_adam_host.py on these lists."""
  name, i = case
  h = sweep.HYPERS[name][i]
  want = adamw_run_over(sweep.inputs(name, h.bf16), sweep.LISTS[name], h)
  mine = sweep.reference(case)
  assert len(mine) == len(want) == sweep.STEPS[name]
  for step in range(sweep.STEPS[name]):
    assert len(mine[step]['p']) == len(want[step]) == len(sweep.LISTS[name])
    for i, (a, b) in enumerate(zip(mine[step]['p'], want[step])):
      assert a.dtype == np.float64 and a.shape == b.shape
      assert np.allclose(a, b, rtol=1e-12, atol=1e-12), (sweep.tag(case), step, i, float(np.abs(a - b).max(initial=0)))
