"""Cost of `embodied_amd.optim.SlowModel`: the stand-alone launch of csrc/optim.hip
against the composed torch ops of the same class and against what a torch user
writes, `torch._foreach_lerp_`; and an optimizer step followed by `update()`
against the step of an optimizer the slow model is attached to.

    python tools/bench_slow_model.py [--calls 200] [--rounds 5] [--out profiles/slow_model_bench.txt]

Four sets of float32 tensors.  Three are the reference's `value` MLP
(dreamerv3/configs.yaml:101: 3 layers of `units` with a kernel, a bias and an
RMS-norm scale each, then the 255-bin head, on a feature of deter + 32 * classes)
at its smallest, default and largest model size; the fourth is the optimizer
bench's small set:
  value1m    size1m:   feature 640, units 64
  value200m  size200m: feature 10240, units 1024 (the default)
  value400m  size400m: feature 15360, units 1536
  small      about 1 M parameters in 40 tensors (tools/bench_optim.py)

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up; the paths alternate inside
            every round; median of the rounds [min .. max].
  host us   wall time of the same calls up to the last enqueue, per call, measured
            from a drained device.
  composed  `dst.mul_(omm).add_(src * mix)` per tensor: the definition.
  lerp      `torch._foreach_lerp_(dst, src, rate)`: not the same expression, not
            bit-comparable; the rival.
  fused     `SlowModel.update()`: one launch, 12 bytes per parameter (reads src and
            dst, writes dst) over its median as a share of the copy ceiling that
            DESIGN.md quotes.
  step+update / attached, for `LaProp` and for `Adam` over the same tensors with
            float32 gradients: the two launches of `step()` and the launch of
            `update()`, against the two launches of `step()` with the slow model
            attached (40 bytes per parameter: the step's 32 and 8 for the copy).

Every set is measured in a process of its own under its own time limit; the tool
stops at the first one that fails or runs out of time and writes no file.  The
last lines name the rows at which each fused median is below its rival's: what
`SlowModel`'s `fused=None` is set from.  Needs a GPU: there is no CPU fallback
and no figure without one.
"""
import argparse
import math
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools import pathbench  # noqa: E402
from tools.pathbench import COPY_CEILING_GBS  # noqa: E402

LIMIT = 300                                               # seconds per set, start-up included
RATE = 0.02                                               # configs.yaml:110, slowvalue
VALUE_SIZES = {'value1m': (512, 4, 64), 'value200m': (8192, 64, 1024), 'value400m': (12288, 96, 1536)}   # deter, classes, units


def value_shapes(deter, classes, units, stoch=32, layers=3, bins=255):
  shapes, width = [], deter + stoch * classes
  for _ in range(layers):
    shapes += [(width, units), (units,), (units,)]
    width = units
  return shapes + [(width, bins), (bins,)]


def shapes_of(name):
  if name in VALUE_SIZES:
    return value_shapes(*VALUE_SIZES[name])
  from tools.bench_optim import parameter_sets
  return dict(parameter_sets())[name]


def measure(name, args):
  """One set, in this process: prints its rows and its `verdict` lines."""
  import torch
  from embodied_amd import optim
  assert torch.cuda.is_available(), 'bench_slow_model needs a GPU'
  shapes = shapes_of(name)
  count = sum(math.prod(s) for s in shapes)
  torch.manual_seed(0)

  def tensors(scale):
    return [torch.randn(s, device='cuda') * scale for s in shapes]

  calls = {}
  src = tensors(0.05)
  slows = {k: optim.SlowModel(tensors(1.0), src, rate=RATE, fused=k == 'fused') for k in ('fused', 'composed')}
  calls['composed'] = slows['composed'].update
  lerp_dst = tensors(1.0)
  calls['lerp'] = lambda: torch._foreach_lerp_(lerp_dst, src, RATE)
  calls['fused'] = slows['fused'].update
  for title, cls in (('laprop', optim.LaProp), ('adam', optim.Adam)):
    for kind in ('step+update', 'attached'):
      params = tensors(0.05)
      for p in params:
        p.grad = torch.randn(p.shape, device='cuda') * 0.01
      opt = cls(params, fused=True)
      slow = optim.SlowModel(tensors(1.0), params, rate=RATE, fused=True)
      if kind == 'attached':
        slow.attach(opt)
        calls[f'{title} attached'] = opt.step
      else:
        calls[f'{title} step+update'] = lambda opt=opt, slow=slow: (opt.step(), slow.update())
  got = pathbench.measure(calls, args.calls, args.rounds, warmup=(2, 3), floor=3)
  host = {k: statistics.median(pathbench.host_us(call, got[k].calls, sync=False) for _ in range(3))
          for k, call in calls.items()}
  assert slows['fused'].table_uploads == 1
  median = {k: v.median for k, v in got.items()}
  print('device: ' + pathbench.device_line()[2:])
  print(f'row:   {name}: {count} parameters in {len(shapes)} tensors, {slows["fused"]._plan["n_chunks"]} chunks of '
        f'{optim.CHUNK}')
  for k in calls:
    print(f'row:     {k:<20}{pathbench.cell(got[k].values, got[k].calls, 10, " us")}'
          f'   host {host[k]:8.1f} us')
  for k, per in (('fused', 12), ('laprop attached', 40), ('adam attached', 40)):
    rate = per * count / median[k] / 1e3
    print(f'row:     {k}: {per} bytes per parameter, {rate:.0f} GB/s = {rate / COPY_CEILING_GBS:.2f} of the copy ceiling '
          f'({COPY_CEILING_GBS:.0f} GB/s)')
  for what, mine, rival in (('composed', 'fused', 'composed'), ('lerp', 'fused', 'lerp'),
                            ('laprop', 'laprop attached', 'laprop step+update'),
                            ('adam', 'adam attached', 'adam step+update')):
    print(f'verdict: {name}|{what}|{"below" if median[mine] < median[rival] else "not below"}', flush=True)


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=200)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'slow_model_bench.txt'))
  parser.add_argument('--sets', default='value1m,value200m,value400m,small')
  parser.add_argument('--child', metavar='SET', help='measure one set in this process')
  args = parser.parse_args()
  if args.child:
    measure(args.child, args)
    return
  report = pathbench.Report('bench_slow_model.py', args, None, [      # the device: from the first set
      f'# SlowModel(rate={RATE:g}, every=1); LaProp() and Adam() at their defaults, float32 gradients',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# host us: wall time up to the last enqueue, per call',
      '# lerp: torch._foreach_lerp_(dst, src, rate) at the same commit, on tensors of its own; another expression',
  ])
  verdicts = []
  for name in args.sets.split(','):
    command = [sys.executable, str(pathlib.Path(__file__).resolve()), '--child', name, '--calls', str(args.calls),
               '--rounds', str(args.rounds)]
    try:
      done = subprocess.run(command, capture_output=True, text=True, timeout=LIMIT, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
      sys.exit(f'bench_slow_model: {name} ran past its {LIMIT} s; stopping, nothing written')
    if done.returncode != 0:
      sys.stderr.write(done.stderr[-4000:])
      sys.exit(f'bench_slow_model: {name} failed with status {done.returncode}; stopping, nothing written')
    for line in done.stdout.splitlines():
      if line.startswith('device: ') and report.lines[1] is None:
        report.lines[1] = '# ' + line[len('device: '):]
      elif line.startswith('row: '):
        report.add(line[len('row: '):])
      elif line.startswith('verdict: '):
        verdicts.append(line[len('verdict: '):].split('|'))
  for what, title in (('composed', 'update() median below the composed median'),
                      ('lerp', 'update() median below the _foreach_lerp_ median'),
                      ('laprop', 'LaProp attached step median below step() + update()'),
                      ('adam', 'Adam attached step median below step() + update()')):
    report.closing(f'{title} at', 'not at', wins=[v[0] for v in verdicts if v[1] == what and v[2] == 'below'],
                   losses=[v[0] for v in verdicts if v[1] == what and v[2] == 'not below'])
  report.write()


if __name__ == '__main__':
  main()
