"""Cost of one return-normaliser call, torch ops against the HIP kernel.

    python tools/bench_normalize.py [--calls 20000] [--rounds 5] [--out profiles/normalize_bench.txt]

For every shape and impl: `distributed.Normalize` (torch: quantile / reductions
and a chain of 0-d ops) and `DeviceNormalize` (one `emb_normalize` launch) run
the same call, `norm(x)` with update, on the same input.

  us/call    host clock around `calls` back-to-back calls that end in a device
             synchronise (20000 calls of 10 us or more: windows of 0.2 s and
             up; a tenth as many calls at 1 M values, which take 100 us and
             up), after a warm-up of the same shape; the two classes alternate inside every round, the figure is the median round
             (min .. max in brackets).  Back-to-back calls cost the larger of
             the host's enqueue time and the device's time.
  launches   device operations (kernels, copies) per call in a torch.profiler
             window of its own; for DeviceNormalize also what the library's
             launch counter says.

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

SHAPES = [(16, 64), (1024, 15), (16, 64, 16), (1 << 20,)]


def timed(norm, x, calls):
  torch.cuda.synchronize()
  start = time.perf_counter()
  for _ in range(calls):
    norm(x)
  torch.cuda.synchronize()
  return (time.perf_counter() - start) / calls * 1e6


def device_ops(norm, x, calls=20):
  """Device-side events per call as torch.profiler sees them (None: no profiler)."""
  try:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      for _ in range(calls):
        norm(x)
      torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(events) / calls
  except Exception as e:      # a figure that was not measured is reported as such
    print(f'# torch.profiler window failed: {e!r}', file=sys.stderr)
    return None


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=20000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'normalize_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_normalize needs a GPU'
  import embodied_amd as emb
  from embodied_amd import distributed as D
  from embodied_amd import normalize as normlib

  lines = [
      f'# tools/bench_normalize.py --calls {args.calls} --rounds {args.rounds}',
      f'# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; norm(x) with update, float32 contiguous input',
      '# us/call: median of rounds [min .. max], host clock over back-to-back calls + synchronise',
      '# launches: device operations per call (torch.profiler window); "lib": emb_normalize launch counter',
      f'# {"shape":<14}{"impl":<9}{"torch us/call":<28}{"device us/call":<28}{"ratio":<8}'
      f'{"torch launches":<16}{"device launches"}',
  ]
  print('\n'.join(lines), flush=True)
  gen = np.random.default_rng(0)
  for shape in SHAPES:
    x = torch.from_numpy(gen.standard_normal(shape).astype(np.float32) * 30 - 4).cuda()
    calls = args.calls if x.numel() <= 1 << 16 else max(args.calls // 10, 20)
    for impl in ('meanstd', 'perc'):
      old, new = D.Normalize(impl), emb.DeviceNormalize(impl)
      for norm in (old, new):               # warm-up of this shape
        timed(norm, x, max(calls // 10, 10))
      # same statistics from both after the same number of updates
      a, b = [float(v) for v in old.stats()], [float(v) for v in new.stats()]
      assert np.allclose(a, b, rtol=1e-5, atol=1e-5), (shape, impl, a, b)
      rounds = {'old': [], 'new': []}
      for _ in range(args.rounds):
        rounds['old'].append(timed(old, x, calls))
        rounds['new'].append(timed(new, x, calls))
      before = normlib.launches()
      timed(new, x, 10)
      counted = (normlib.launches() - before) / 10
      seen = (None, None) if args.no_profiler else (device_ops(old, x), device_ops(new, x))

      def cell(values):
        return f'{statistics.median(values):8.1f} [{min(values):.1f} .. {max(values):.1f}]'

      def count(value):
        return 'not measured' if value is None else f'{value:.1f}'

      ratio = statistics.median(rounds['old']) / statistics.median(rounds['new'])
      line = (f'  {"x".join(map(str, shape)):<14}{impl:<9}{cell(rounds["old"]):<28}{cell(rounds["new"]):<28}'
              f'{ratio:<8.2f}{count(seen[0]):<16}{count(seen[1])} (lib {counted:.1f})')
      lines.append(line)
      print(line, flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
