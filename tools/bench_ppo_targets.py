"""Cost of the PPO targets of one train step, composed against fused.

    python tools/bench_ppo_targets.py [--calls 5000] [--rounds 5] [--out profiles/ppo_targets_bench.txt]

For every shape `scans.ppo_targets` runs the same call -- update on, `out=` given,
contiguous float32 inputs, both normalisers 'meanstd' -- on its two paths:
composed (`gae`, two `DeviceNormalize.normalize` launches and torch's multiply-add,
copy, clip and pad) and fused (one `emb_ppo_targets` launch of one workgroup).

  us/call    host clock around `calls` back-to-back calls that end in a device
             synchronise, after a warm-up of the same shape (a hundredth as many
             calls beyond 65 536 values, where a call takes 0.1 ms and up); the
             two paths alternate inside every round, the figure is the median
             round (min .. max in brackets).  Back-to-back calls cost the larger
             of the host's enqueue time and the device's time.
  launches   device operations (kernels, copies) per call in a torch.profiler
             window of its own; "lib": what the library's launch counters say
             (emb_ppo_targets + emb_normalize; gae has no counter).

The last line names the largest shape at which the fused path still wins: the
crossover `scans.PPO_TARGETS_FUSED_MAX` is set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402
from tools.pathbench import host_us  # noqa: E402

SHAPES = [(16, 64), (64, 64), (1024, 16), (16, 1024), (4096, 64), (65536, 64)]


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=5000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'ppo_targets_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_ppo_targets needs a GPU'
  import embodied_amd as emb
  from embodied_amd import normalize as normlib
  from embodied_amd import scans

  device = (pathbench.device_line(arch=False) + '; scans.ppo_targets(update=True, out=...), '
            'meanstd normalisers, float32 contiguous inputs')
  report = pathbench.Report('bench_ppo_targets.py', args, device, [
      '# us/call: median of rounds [min .. max], host clock over back-to-back calls + synchronise',
      '# launches: device operations per call (torch.profiler window); "lib": emb_ppo_targets + emb_normalize counters',
      f'# {"shape":<12}{"values":<10}{"composed us/call":<30}{"fused us/call":<30}{"ratio":<8}'
      f'{"composed launches":<24}{"fused launches"}',
  ])
  gen = np.random.default_rng(0)
  wins = []
  for B, T in SHAPES:
    inputs = [torch.from_numpy(gen.standard_normal((B, T)).astype(np.float32)).cuda() for _ in range(2)]
    inputs += [torch.from_numpy(gen.random((B, T)) < p).cuda() for p in (0.05, 0.03)]
    calls = args.calls if B * T <= 1 << 16 else max(args.calls // 100, 10)
    paths = {}
    for name, fused in (('composed', False), ('fused', True)):
      norms = emb.DeviceNormalize('meanstd'), emb.DeviceNormalize('meanstd')
      out = tuple(torch.empty(shape, device='cuda') for shape in ((B, T - 1), (B, T - 1), (B, T), (B, T - 1)))
      paths[name] = (lambda norms=norms, out=out, fused=fused:
                     scans.ppo_targets(*inputs, *norms, out=out, fused=fused)), norms, out
    for call, _, _ in paths.values():               # warm-up of this shape
      host_us(call, max(calls // 10, 10))
    # the same results from both after the same number of steps
    for a, b in zip(paths['composed'][2], paths['fused'][2]):
      assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), (B, T)
    got = pathbench.run_rounds({name: path[0] for name, path in paths.items()}, calls, args.rounds, timer=host_us)
    counted = {}
    for name in got:
      before = scans.ppo_targets_launches() + normlib.launches()
      host_us(paths[name][0], 10)
      counted[name] = (scans.ppo_targets_launches() + normlib.launches() - before) / 10
    seen = {name: None if args.no_profiler else pathbench.device_ops(paths[name][0], 20) for name in got}
    cell = lambda name: pathbench.cell(got[name].values)
    count = lambda name: f'{pathbench.count(seen[name])} (lib {counted[name]:.1f})'
    ratio = got['composed'].median / got['fused'].median
    if ratio > 1.0:
      wins.append((B, T))
    report.add(f'  {f"{B}x{T}":<12}{B * T:<10}{cell("composed"):<30}{cell("fused"):<30}'
               f'{ratio:<8.2f}{count("composed"):<24}{count("fused")}')
  largest = max(wins, key=lambda shape: shape[0] * shape[1]) if wins else None
  report.add('# fused wins (ratio > 1) at: ' + (', '.join(f'{b}x{t}' for b, t in wins) or 'no measured shape')
             + (f'; largest: {largest[0]}x{largest[1]} = {largest[0] * largest[1]} values' if largest else ''))
  report.write()


if __name__ == '__main__':
  main()
