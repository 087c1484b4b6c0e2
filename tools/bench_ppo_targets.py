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
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(16, 64), (64, 64), (1024, 16), (16, 1024), (4096, 64), (65536, 64)]


def timed(call, calls):
  torch.cuda.synchronize()
  start = time.perf_counter()
  for _ in range(calls):
    call()
  torch.cuda.synchronize()
  return (time.perf_counter() - start) / calls * 1e6


def device_ops(call, calls=20):
  """Device-side events per call as torch.profiler sees them (None: no profiler)."""
  try:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      for _ in range(calls):
        call()
      torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(events) / calls
  except Exception as e:      # a figure that was not measured is reported as such
    print(f'# torch.profiler window failed: {e!r}', file=sys.stderr)
    return None


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

  lines = [
      f'# tools/bench_ppo_targets.py --calls {args.calls} --rounds {args.rounds}',
      f'# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; scans.ppo_targets(update=True, out=...), '
      'meanstd normalisers, float32 contiguous inputs',
      '# us/call: median of rounds [min .. max], host clock over back-to-back calls + synchronise',
      '# launches: device operations per call (torch.profiler window); "lib": emb_ppo_targets + emb_normalize counters',
      f'# {"shape":<12}{"values":<10}{"composed us/call":<30}{"fused us/call":<30}{"ratio":<8}'
      f'{"composed launches":<24}{"fused launches"}',
  ]
  print('\n'.join(lines), flush=True)
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
      timed(call, max(calls // 10, 10))
    # the same results from both after the same number of steps
    for a, b in zip(paths['composed'][2], paths['fused'][2]):
      assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), (B, T)
    rounds = {'composed': [], 'fused': []}
    for _ in range(args.rounds):
      for name in rounds:
        rounds[name].append(timed(paths[name][0], calls))
    counted = {}
    for name in rounds:
      before = scans.ppo_targets_launches() + normlib.launches()
      timed(paths[name][0], 10)
      counted[name] = (scans.ppo_targets_launches() + normlib.launches() - before) / 10
    seen = {name: None if args.no_profiler else device_ops(paths[name][0]) for name in rounds}

    def cell(values):
      return f'{statistics.median(values):9.1f} [{min(values):.1f} .. {max(values):.1f}]'

    def count(name):
      ops = 'not measured' if seen[name] is None else f'{seen[name]:.1f}'
      return f'{ops} (lib {counted[name]:.1f})'

    ratio = statistics.median(rounds['composed']) / statistics.median(rounds['fused'])
    if ratio > 1.0:
      wins.append((B, T))
    line = (f'  {f"{B}x{T}":<12}{B * T:<10}{cell(rounds["composed"]):<30}{cell(rounds["fused"]):<30}'
            f'{ratio:<8.2f}{count("composed"):<24}{count("fused")}')
    lines.append(line)
    print(line, flush=True)
  largest = max(wins, key=lambda shape: shape[0] * shape[1]) if wins else None
  lines.append('# fused wins (ratio > 1) at: ' + (', '.join(f'{b}x{t}' for b, t in wins) or 'no measured shape')
               + (f'; largest: {largest[0]}x{largest[1]} = {largest[0] * largest[1]} values' if largest else ''))
  print(lines[-1], flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
