"""Cost of the scalar book-keeping of one DreamerV3 train step: the metrics of
imag_loss (dreamerv3/agent.py:424-442, `scans.imag_metrics`) and the loss means
and their total (dreamerv3/agent.py:239-240, `outs.total_loss`), the composed
torch ops against the kernels of csrc/stat_rows.hip.

    python tools/bench_stat_metrics.py [--calls 1000] [--rounds 5] [--out profiles/stat_metrics_bench.txt]

  imag_metrics  (N, T) with two action keys, both with entropy limits, a 'perc'
                retnorm stepped by `dreamer_targets` and float vstats: 12 entries.
                (16, 16), the workload's (1024, 16), (1024, 17) -- the most
                returns `dreamer_targets` fuses -- and (4096, 16), past 16 384.
  total_loss    K = 10 losses of (B, T) each, forward, and forward + backward
                (`loss.backward()`, the `.grad`s dropped between calls).

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  enqueue   for the fused call: host time per call of issuing the same calls
            without waiting for the device (median of the rounds).  Where the
            device-event figure is within 15 % of it the row is marked `host`.
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `scans._imag_metrics_path` and
`outs._total_loss_path` are set from.  The comparison is against the composed
path of the same commit and nothing else.  Needs a GPU: there is no CPU fallback
and no figure without one.
"""
import argparse
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402

IMAG_SHAPES = [(16, 16), (1024, 16), (1024, 17), (4096, 16)]
LOSS_SHAPES = [(10, 16, 64), (10, 64, 64)]
ENTLIMITS = {'move': (0.0, 1.6094379124341003), 'arm': (-3.5, 4.25)}


def imag_pieces(n, t, gen):
  from embodied_amd import DeviceNormalize, scans
  f = lambda shape: torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda()
  rew, pred, slow = f((n, t)), f((n, t)), f((n, t))
  con = torch.from_numpy((0.9 + 0.1 * gen.random((n, t))).astype(np.float32)).cuda()
  ents = {'move': f((n, t)).abs(), 'arm': f((n, t))}
  retnorm = DeviceNormalize('perc')
  none = DeviceNormalize('none')
  if n * (t - 1) <= 16384:
    targets = scans.dreamer_targets(rew, con, slow, retnorm, none, none)
  else:                              # past what one launch of dreamer_targets holds: arrays of the same shapes
    retnorm(f((1024, 15)))
    targets = scans.DreamerTargets(f((n, t - 1)), con.clone(), f((n, t - 1)), f((n, t - 1)), f((n, t)))
  call = lambda fused: scans.imag_metrics(targets, rew, con, pred, slow, retnorm, (0.25, 1.5), ents, ENTLIMITS, fused=fused)
  a, b = call(False), call(True)
  for key in a:
    assert torch.allclose(a[key], b[key], rtol=1e-5, atol=1e-5), ((n, t), key, a[key], b[key])
  return {'forward': {fused: (lambda fused=fused: call(fused)) for fused in (False, True)}}


def loss_pieces(count, b, t, gen):
  from embodied_amd import outs
  names = [f'loss{k}' for k in range(count)]
  losses = {k: torch.from_numpy(gen.standard_normal((b, t)).astype(np.float32)).cuda().requires_grad_() for k in names}
  scales = {k: 0.1 + 0.3 * i for i, k in enumerate(names)}
  forward = {fused: (lambda fused=fused: outs.total_loss(losses, scales, fused=fused)) for fused in (False, True)}

  def both(fused):
    for v in losses.values():
      v.grad = None
    forward[fused]()[0].backward()

  grads = []
  for fused in (False, True):
    both(fused)
    grads.append([v.grad.clone() for v in losses.values()])
  for x, y in zip(*grads):
    assert torch.allclose(x, y, rtol=1e-6, atol=0), (count, b, t)
  assert torch.allclose(forward[False]()[0], forward[True]()[0], rtol=1e-5, atol=1e-6)
  return {'forward': forward, 'fwd+bwd': {fused: (lambda fused=fused: both(fused)) for fused in (False, True)}}


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'stat_metrics_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_stat_metrics needs a GPU'
  device = (pathbench.device_line()
            + '; scans.imag_metrics (two action keys with limits, perc retnorm, float vstats) and outs.total_loss')
  report = pathbench.Report('bench_stat_metrics.py', args, device, [
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# enqueue: host time per fused call without waiting for the device; `host`: the fused us is the enqueue time',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# {"call":<28}{"piece":<10}{"composed us":<34}{"fused us":<34}{"enqueue us":<14}ops composed / fused',
  ])
  gen = np.random.default_rng(0)
  jobs = [(f'imag_metrics {n}x{t}', imag_pieces(n, t, gen)) for n, t in IMAG_SHAPES]
  jobs += [(f'total_loss K={k} {b}x{t}', loss_pieces(k, b, t, gen)) for k, b, t in LOSS_SHAPES]
  for name, pieces in jobs:
    for piece, paths in pieces.items():
      issue = []
      enqueue = lambda calls: issue.append(pathbench.host_us(paths[True], calls[True], sync=False))
      got = pathbench.measure(paths, args.calls, args.rounds, after_round=enqueue)
      ops = {f: None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths}
      report.verdict(f'{name} {piece}', pathbench.median_below(got[True], got[False]))
      enqueued = statistics.median(issue)
      bound = f'{enqueued:.1f}' + (' host' if got[True].median <= 1.15 * enqueued else '')
      report.add(f'  {name:<28}{piece:<10}{got[False].cell:<34}{got[True].cell:<34}{bound:<14}'
                 f'{pathbench.count(ops[False])} / {pathbench.count(ops[True])}')
  report.closing()
  report.write()


if __name__ == '__main__':
  main()
