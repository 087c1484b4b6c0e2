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
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402
from tools.pathbench import host_us  # noqa: E402

SHAPES = [(16, 64), (1024, 15), (16, 64, 16), (1 << 20,)]


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

  device = pathbench.device_line(arch=False) + '; norm(x) with update, float32 contiguous input'
  report = pathbench.Report('bench_normalize.py', args, device, [
      '# us/call: median of rounds [min .. max], host clock over back-to-back calls + synchronise',
      '# launches: device operations per call (torch.profiler window); "lib": emb_normalize launch counter',
      f'# {"shape":<14}{"impl":<9}{"torch us/call":<28}{"device us/call":<28}{"ratio":<8}'
      f'{"torch launches":<16}{"device launches"}',
  ])
  gen = np.random.default_rng(0)
  for shape in SHAPES:
    x = torch.from_numpy(gen.standard_normal(shape).astype(np.float32) * 30 - 4).cuda()
    calls = args.calls if x.numel() <= 1 << 16 else max(args.calls // 10, 20)
    for impl in ('meanstd', 'perc'):
      old, new = D.Normalize(impl), emb.DeviceNormalize(impl)
      paths = {'old': lambda: old(x), 'new': lambda: new(x)}
      for call in paths.values():           # warm-up of this shape
        host_us(call, max(calls // 10, 10))
      # same statistics from both after the same number of updates
      a, b = [float(v) for v in old.stats()], [float(v) for v in new.stats()]
      assert np.allclose(a, b, rtol=1e-5, atol=1e-5), (shape, impl, a, b)
      got = pathbench.run_rounds(paths, calls, args.rounds, timer=host_us)
      before = normlib.launches()
      host_us(paths['new'], 10)
      counted = (normlib.launches() - before) / 10
      seen = [None if args.no_profiler else pathbench.device_ops(call, 20) for call in paths.values()]
      cell = lambda name: pathbench.cell(got[name].values, width=8)
      ratio = got['old'].median / got['new'].median
      report.add(f'  {"x".join(map(str, shape)):<14}{impl:<9}{cell("old"):<28}{cell("new"):<28}'
                 f'{ratio:<8.2f}{pathbench.count(seen[0]):<16}{pathbench.count(seen[1])} (lib {counted:.1f})')
  report.write()


if __name__ == '__main__':
  main()
