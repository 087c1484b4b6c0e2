"""tools/pathbench.py, the measuring protocol of the family benches, without a
GPU: the timer is injected.  The order of the calls it issues, the sizing of a
round, the verdict rules, the report's text -- and the row formatters of three
benches held against the rows of the committed profiles, so that a file written
from the same timer readings is the file the benches wrote before they shared
this module."""
import argparse
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools import bench_conv_stage, bench_normal_policy, bench_policy_loss, pathbench  # noqa: E402

FAMILY = ('twohot', 'policy_loss', 'normal_policy', 'onehot_sample', 'recon_loss', 'rssm_kl', 'rssm_core', 'stat_metrics',
          'conv_stage', 'optim', 'adam', 'slow_model', 'ppo_targets', 'dreamer_targets', 'normalize')
CELL = re.compile(r'([\d.]+) \[([\d.]+) \.\. ([\d.]+)\] \((\d+)\)')


class FakeTimer:
  """Records (path, calls); every path's value is scripted.  The paths of these tests are their own names."""

  def __init__(self, values):
    self.values, self.log = values, []

  def __call__(self, call, calls):
    self.log.append((call, calls))
    return self.values[call]


def paths_of(*names):
  return {name: name for name in names}


# ---------------------------------------------------------------- the order of the protocol

def test_measure_warms_up_sizes_then_alternates():
  timer = FakeTimer({'composed': 1000.0, 'fused': 250.0})        # 0.1e6 / estimate: 100 and 400 calls
  got = pathbench.measure(paths_of('composed', 'fused'), 1000, 3, timer=timer)
  assert timer.log == [('composed', 3), ('composed', 5), ('fused', 3), ('fused', 5)] + [('composed', 100), ('fused', 400)] * 3
  assert list(got) == ['composed', 'fused']
  assert got['composed'].values == [1000.0] * 3 and got['composed'].calls == 100
  assert got['fused'].values == [250.0] * 3 and got['fused'].calls == 400 and got['fused'].median == 250.0
  assert got['fused'].cell == '    250.0 [250.0 .. 250.0] (400)'


def test_measure_with_the_optimizer_benches_warmup():
  timer = FakeTimer({'composed': 1000.0, 'fused': 250.0})
  pathbench.measure(paths_of('composed', 'fused'), 1000, 2, warmup=(2, 3), floor=3, timer=timer)
  assert timer.log == [('composed', 2), ('composed', 3), ('fused', 2), ('fused', 3)] + [('composed', 100), ('fused', 400)] * 2


def test_after_round_runs_once_per_round_with_the_calls():
  timer, seen = FakeTimer({'composed': 1000.0, 'fused': 250.0}), []
  pathbench.measure(paths_of('composed', 'fused'), 1000, 3, timer=timer,
                    after_round=lambda calls: seen.append((len(timer.log), dict(calls))))
  assert seen == [(4 + 2 * r, {'composed': 100, 'fused': 400}) for r in (1, 2, 3)]


def test_run_rounds_takes_one_number_for_all_paths():
  timer = FakeTimer({'old': 12.0, 'new': 3.0})
  got = pathbench.run_rounds(paths_of('old', 'new'), 50, 2, timer=timer)
  assert timer.log == [('old', 50), ('new', 50)] * 2
  assert got['old'].calls == got['new'].calls == 50


# ---------------------------------------------------------------- the sizing of a round

# calls = int(min(cap, max(floor, budget / estimate))), cap 1000; estimates of 10, 300 and 50 000 us
@pytest.mark.parametrize('floor, budget, want', [
    (5, 0.1e6, {10.0: 1000, 300.0: 333, 50000.0: 5}),
    (5, 0.2e6, {10.0: 1000, 300.0: 666, 50000.0: 5}),
    (3, 0.1e6, {10.0: 1000, 300.0: 333, 50000.0: 3}),
])
def test_sizing(floor, budget, want):
  for estimate, calls in want.items():
    assert calls == int(min(1000, max(floor, budget / estimate)))        # the table above is the formula's
    timer = FakeTimer({'path': estimate})
    assert pathbench.sized('path', 1000, floor=floor, budget_us=budget, timer=timer) == calls
    got = pathbench.measure(paths_of('path'), 1000, 1, floor=floor, budget_us=budget, timer=timer)
    assert got['path'].calls == calls and timer.log[-1] == ('path', calls)


# ---------------------------------------------------------------- rows of the committed profiles

def committed(name, number):
  return (ROOT / 'profiles' / name).read_text().splitlines()[number - 1]


def cells_of(line):
  """The Rounds of every 'median [min .. max] (calls)' cell of a row.  Three values with that median, minimum and
  maximum: an odd number of rounds leaves the others open."""
  found = [tuple(map(float, m.groups()[:3])) + (int(m.group(4)),) for m in CELL.finditer(line)]
  return [pathbench.rounds_of([low, median, high], calls) for median, low, high, calls in found]


def test_policy_loss_row_is_the_committed_one():
  composed = pathbench.rounds_of([119.4, 121.6, 122.0], 776)
  fused = pathbench.rounds_of([23.1, 23.3, 24.7], 1000)
  line = bench_policy_loss.row('1024x16x6 f32', 'forward', composed, fused, (19.0, 1.0), 1024 * 16 * 6 * 4)
  assert line == committed('policy_loss_bench.txt', 8)
  assert line.endswith('17 = 0.00 of the ceiling')


def test_conv_stage_row_is_the_committed_one():
  want = committed('conv_stage_bench.txt', 12)               # three paths, and cells wider than their columns
  assert want.startswith('  pool 1024x64x64x128 f32           fwd+bwd  ')
  composed, parent, fused = cells_of(want)
  moved = 3.5 * 1024 * 64 * 64 * 128 * 4
  got = {'composed': composed, 'parent': parent, 'fused': fused}
  assert bench_conv_stage.row('pool 1024x64x64x128 f32', 'fwd+bwd', got, moved) == want


def test_normal_policy_row_is_the_committed_one():
  want = committed('normal_policy_bench.txt', 9)             # with the enqueue column, marked `host`
  assert want.startswith('  1024x16x1 f32         forward   ')
  composed, fused = cells_of(want)
  enqueue, mark, ops = re.search(r'\)\s+([\d.]+) (host)?\s+([\d.]+ / [\d.]+)', want).groups()
  count = 1024 * 16 * 1
  moved = 2 * 4 * count + 4 * count                          # both raw inputs and the actions, float32
  counts = tuple(float(n) for n in ops.split(' / '))
  assert mark == 'host'
  assert bench_normal_policy.row('1024x16x1 f32', 'forward', composed, fused, float(enqueue), counts, moved) == want
  # the mark goes where the fused figure is more than 15 % above the enqueue time
  assert ' host' not in bench_normal_policy.row('1024x16x1 f32', 'forward', composed, fused, 19.9, counts, moved)


# ---------------------------------------------------------------- verdicts and the closing lines

def test_median_below():
  low, high = pathbench.rounds_of([1.0, 2.0, 9.0]), pathbench.rounds_of([1.5, 2.5, 3.0])
  assert pathbench.median_below(low, high)
  assert not pathbench.median_below(high, low)
  assert not pathbench.median_below(low, low)                # equal is not below


def test_median_below_both_rivals():
  fused, composed = pathbench.rounds_of([2.0, 2.0, 2.0]), pathbench.rounds_of([5.0, 5.0, 5.0])
  assert pathbench.median_below(fused, composed, pathbench.rounds_of([3.0, 3.0, 3.0]))
  assert not pathbench.median_below(fused, composed, pathbench.rounds_of([1.0, 1.0, 1.0]))     # below one rival only


def test_every_round_below_every_round():
  fused = pathbench.rounds_of([1.0, 2.0, 3.0])
  assert pathbench.every_round_below(fused, pathbench.rounds_of([3.1, 4.0, 5.0]))
  assert not pathbench.every_round_below(fused, pathbench.rounds_of([2.9, 4.0, 5.0]))          # the medians alone would pass


def report_of(tmp_path, capsys, device='# a device (gfx950), torch 2'):
  args = argparse.Namespace(calls=20, rounds=2, out=str(tmp_path / 'deep' / 'bench.txt'))
  report = pathbench.Report('bench_policy_loss.py', args, device, ['# a header line'])
  return report, capsys.readouterr().out


def test_report_header_rows_closing_and_file(tmp_path, capsys):
  report, printed = report_of(tmp_path, capsys)
  assert printed == '# tools/bench_policy_loss.py --calls 20 --rounds 2\n# a device (gfx950), torch 2\n# a header line\n'
  report.add('  row one', '  row two')
  assert capsys.readouterr().out == '  row one\n  row two\n'        # printed as they are added
  report.verdict('row one', True)
  report.verdict('row two', False)
  report.verdict('row three', True)
  report.closing()
  closing = ('# fused median below composed median at: row one, row three\n'
             '# fused median not below composed median at: row two\n')
  assert capsys.readouterr().out == closing
  report.write()
  assert (tmp_path / 'deep' / 'bench.txt').read_text() == printed + '  row one\n  row two\n' + closing


def test_closing_with_no_row_in_the_bench_s_own_words(tmp_path, capsys):
  report, _ = report_of(tmp_path, capsys)
  report.closing()
  report.closing('fused median below both rivals at', 'fused median not below both rivals at')
  report.closing('fused beats composed, every round of one below every round of the other, at',
                 'fused does not beat composed in every round at', none='no measured shape')
  report.closing('update() median below the composed median at', 'not at', wins=['small'], losses=[])
  assert report.lines[3:] == [
      '# fused median below composed median at: no measured row',
      '# fused median not below composed median at: no measured row',
      '# fused median below both rivals at: no measured row',
      '# fused median not below both rivals at: no measured row',
      '# fused beats composed, every round of one below every round of the other, at: no measured shape',
      '# fused does not beat composed in every round at: no measured shape',
      '# update() median below the composed median at: small',
      '# not at: no measured row',
  ]


def test_report_whose_device_comes_later(tmp_path, capsys):
  report, printed = report_of(tmp_path, capsys, device=None)
  assert printed == ''
  report.lines[1] = '# the first child process\'s device'
  report.write()
  assert (tmp_path / 'deep' / 'bench.txt').read_text().splitlines()[1] == '# the first child process\'s device'


# ---------------------------------------------------------------- a profiler window that fails

def test_unmeasured_operation_count(monkeypatch, capsys):
  import torch

  def refuse():
    raise RuntimeError('no device')
  monkeypatch.setattr(torch.cuda, 'synchronize', refuse)
  assert pathbench.device_ops(lambda: None) is None
  assert '# torch.profiler window failed: RuntimeError' in capsys.readouterr().err
  assert pathbench.count(None) == 'not measured' and pathbench.count(19.0) == '19.0'
  fused = pathbench.rounds_of([23.1, 23.3, 24.7], 1000)
  assert 'not measured / not measured' in bench_policy_loss.row('1024x16x6 f32', 'forward', fused, fused, (None, None), 4)


# ---------------------------------------------------------------- one home for the protocol, read as text

def test_benches_import_the_protocol_and_nothing_from_each_other():
  borrowed = []
  for path in sorted((ROOT / 'tools').glob('bench_*.py')):
    text = path.read_text()
    borrowed += [(path.name, m.group(1), m.group(2).strip()) for m in
                 re.finditer(r'^\s*from tools\.(bench_\w+) import ([^#\n]+)', text, re.M)]
    assert not re.search(r'^\s*(import tools\.bench_|from tools import .*\bbench_|import bench_|from bench_)', text, re.M), path.name
  assert borrowed == [('bench_adam.py', 'bench_optim', 'parameter_sets'), ('bench_slow_model.py', 'bench_optim', 'parameter_sets')]
  for name in FAMILY:
    text = (ROOT / 'tools' / f'bench_{name}.py').read_text()
    assert re.search(r'^from tools import pathbench\b', text, re.M), name
  assert 'bench_' not in re.sub(r'bench_\*|_bench\.txt', '', (ROOT / 'tools' / 'pathbench.py').read_text())


def test_timers_are_defined_once():
  sources = {path.name: path.read_text() for path in (ROOT / 'tools').glob('*.py')}
  for timer in ('device_us', 'host_us', 'device_ops'):
    assert [name for name, text in sources.items() if re.search(rf'^\s*def {timer}\(', text, re.M)] == ['pathbench.py'], timer
  for name in FAMILY:                                          # and no host clock or event pair of a bench's own
    text = sources[f'bench_{name}.py']
    assert not re.search(r'^\s*def (timed|enqueue_us)\(|perf_counter|cuda\.Event|import time\b', text, re.M), name
