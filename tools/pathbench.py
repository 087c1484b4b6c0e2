"""The measuring protocol of the family benches (tools/bench_*.py that write
profiles/*_bench.txt): the timers, the rounds, the verdict rules and the report.

A bench is a script with its own inputs, paths, equality asserts and row text.
What it shares with the others is here, and what it varies is an argument at
its call site:

  timers    `device_us` (an event pair), `host_us` (the host clock, with or
            without the closing synchronise inside it), `device_ops` (a
            torch.profiler window of its own).
  rounds    `sized` warms a path up, estimates one call and sets the calls of
            a round: int(min(cap, max(floor, budget_us / estimate))).
            `run_rounds` runs the rounds, the paths alternating inside each.
            `measure` is the two together.
  verdicts  `median_below` and `every_round_below`.
  report    `Report`: the header, every line printed as it is added, the rows
            won and lost, the closing pair and the file.
"""
import collections
import pathlib
import statistics
import sys

import torch

COPY_CEILING_GBS = 6290.0       # the copy ceiling of this part, read + write bytes

# One path's rounds: the value of every round (us per call), the calls of a round, the median, the cell of a row.
Rounds = collections.namedtuple('Rounds', 'values calls median cell')


def device_us(call, calls):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for _ in range(calls):
    call()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) * 1e3 / calls


def host_us(call, calls, sync=True):
  """Host clock per call from a drained device.  `sync=True`: the clock runs
  until the device has finished.  `sync=False`: it stops after the last enqueue
  and the device is waited for outside it."""
  import time
  torch.cuda.synchronize()
  start = time.perf_counter()
  for _ in range(calls):
    call()
  if sync:
    torch.cuda.synchronize()
  spent = time.perf_counter() - start
  torch.cuda.synchronize()
  return spent * 1e6 / calls


def device_ops(call, calls=3, skip=None):
  """Device-side events per call as torch.profiler sees them (None: no
  profiler).  `skip`: the start of the name of events that are no operation,
  such as the annotation `Optimizer.step` runs inside."""
  try:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      for _ in range(calls):
        call()
      torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
              and not (skip and e.name.startswith(skip))]
    return len(events) / calls
  except Exception as e:      # a figure that was not measured is reported as such
    print(f'# torch.profiler window failed: {e!r}', file=sys.stderr)
    return None


def count(ops):
  return 'not measured' if ops is None else f'{ops:.1f}'


def cell(values, calls=None, width=9, unit=''):
  """'   median [min .. max] (calls)'; without `calls`, without the bracket."""
  text = f'{statistics.median(values):{width}.1f}{unit} [{min(values):.1f} .. {max(values):.1f}]'
  return text if calls is None else f'{text} ({calls})'


def rounds_of(values, calls=None):
  return Rounds(list(values), calls, statistics.median(values), cell(values, calls))


def sized(call, cap, warmup=(3, 5), floor=5, budget_us=0.1e6, timer=device_us):
  """Warm `call` up, estimate one call, and return the calls of one round."""
  timer(call, warmup[0])
  estimate = timer(call, warmup[1])
  return int(min(cap, max(floor, budget_us / estimate)))


def run_rounds(paths, calls, rounds, timer=device_us, after_round=None):
  """`rounds` rounds, the paths alternating inside each: {name: Rounds}.
  `calls`: the calls of a round per path, or one number for all.
  `after_round(calls)`: a sample of the bench's own, once per round."""
  if not isinstance(calls, dict):
    calls = dict.fromkeys(paths, calls)
  values = {name: [] for name in paths}
  for _ in range(rounds):
    for name, call in paths.items():
      values[name].append(timer(call, calls[name]))
    if after_round:
      after_round(calls)
  return {name: rounds_of(values[name], calls[name]) for name in paths}


def measure(paths, cap, rounds, *, warmup=(3, 5), floor=5, budget_us=0.1e6, timer=device_us, after_round=None):
  """The round protocol over `paths`, an ordered mapping of name to callable:
  every path warmed up and sized in turn, then the rounds."""
  calls = {name: sized(call, cap, warmup, floor, budget_us, timer) for name, call in paths.items()}
  return run_rounds(paths, calls, rounds, timer, after_round)


def median_below(mine, *rivals):
  return all(mine.median < rival.median for rival in rivals)


def every_round_below(mine, rival):
  return max(mine.values) < min(rival.values)


def device_line(arch=True):
  props = f' ({torch.cuda.get_device_properties(0).gcnArchName})' if arch else ''
  return f'# {torch.cuda.get_device_name(0)}{props}, torch {torch.__version__}'


class Report:
  """The lines of one profile file.  `device`: its second line (`device_line()`
  and what the bench adds to it); None where it is not known yet, and then the
  header is not printed and the bench sets `lines[1]` itself."""

  def __init__(self, script, args, device, header=()):
    self.lines = [f'# tools/{script} --calls {args.calls} --rounds {args.rounds}', device, *header]
    self.out, self.wins, self.losses = args.out, [], []
    if device is not None:
      print('\n'.join(self.lines), flush=True)

  def add(self, *lines):
    for line in lines:
      self.lines.append(line)
      print(line, flush=True)

  def verdict(self, row, won):
    (self.wins if won else self.losses).append(row)

  def closing(self, won='fused median below composed median at', lost='fused median not below composed median at',
              none='no measured row', wins=None, losses=None):
    """'# <won>: <rows>' and '# <lost>: <rows>', of this report's rows or of the lists given."""
    wins, losses = (self.wins if wins is None else wins), (self.losses if losses is None else losses)
    self.add(f'# {won}: ' + (', '.join(wins) or none), f'# {lost}: ' + (', '.join(losses) or none))

  def write(self):
    out = pathlib.Path(self.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(line for line in self.lines if line is not None) + '\n')
