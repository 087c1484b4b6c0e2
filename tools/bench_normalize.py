"""Cost of one return-normaliser call, torch ops against the HIP kernel.

    python tools/bench_normalize.py [--calls 20000] [--rounds 5] [--out profiles/normalize_bench.txt]
                                    [--parent-lib libembodied_hip.so of the commit before the chain]
                                    [--chain-lib libembodied_hip.so of this tree with kNormGridMin = 16385]

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

The second table is what kNormGridMin (csrc/normalize.h) is set from: for every
n above one workgroup's LDS and impl, `update` and `update + out`, three columns
-- the one-workgroup kernel (`emb_normalize` of `--parent-lib`, a library built
from the commit before the chain; "not measured" without it), torch composed,
and the chain of launches of csrc/normalize_grid.hip (`emb_normalize` of
`--chain-lib`, this tree built with kNormGridMin = 16385 so that every row takes
the chain; without it, this build).  Its closing line names the smallest
measured n at which the chain's median is below the one-workgroup median for
both impls and both calls: kNormGridMin.

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
GRID_SIZES = [16385, 32768, 61440, 131072, 262144, 1 << 20]


def library_call(path, impl, x, out):
  """`emb_normalize` of the library at `path` as a call on x (and out), with a
  state of its own (`call.state`) and that library's launch counter (`call.launches`)."""
  import ctypes as C
  from embodied_amd import _lib
  lib = C.CDLL(str(path))
  lib.emb_normalize.argtypes, lib.emb_normalize.restype = _lib.SIGNATURES['emb_normalize'], C.c_int32
  config = _lib.NormalizeConfig({'meanstd': _lib.NORM_MEANSTD, 'perc': _lib.NORM_PERC}[impl], 1, 0.01, 1e-8, 5.0, 95.0)
  state = torch.zeros(5, dtype=torch.float32, device=x.device)
  stream = _lib.raw_stream(x.device)

  def call():
    status = lib.emb_normalize(C.byref(config), x.data_ptr(), x.numel(), state.data_ptr(), 1, None,
                               None if out is None else out.data_ptr(), stream)
    assert status == 0, status

  def launches():
    count = C.c_int64(0)
    lib.emb_normalize_launches(C.byref(count))
    return count.value
  call.state, call.launches = state, launches
  return call


def grid_rows(report, args):
  """The three-column table over GRID_SIZES and the threshold it gives."""
  from embodied_amd import _lib
  from embodied_amd import distributed as D
  chain_lib = args.chain_lib or _lib.PATH
  report.add(
      '# one workgroup (--parent-lib: the kernel of the commit before the chain) | torch composed | the chain of launches',
      '# (--chain-lib: this tree built with kNormGridMin = 16385, so that every row takes the chain)' if args.chain_lib
      else '# (the chain column is this build: rows below its kNormGridMin take the one-workgroup kernel)',
      f'# {"n":<10}{"impl":<9}{"call":<13}{"one workgroup us/call":<34}{"torch us/call":<34}{"chain us/call":<34}{"chain launches"}')
  gen = np.random.default_rng(1)
  below = {}
  for n in GRID_SIZES:
    x = torch.from_numpy(gen.standard_normal(n).astype(np.float32) * 30 - 4).cuda()
    out = torch.empty_like(x)
    for impl in ('meanstd', 'perc'):
      for mode in ('update', 'update+out'):
        old = D.Normalize(impl)
        target = out if mode == 'update+out' else None
        chain = library_call(chain_lib, impl, x, target)
        parent = library_call(args.parent_lib, impl, x, target) if args.parent_lib else None

        def torch_call():
          offset, scale = old(x)
          return (x - offset) / scale if target is not None else None
        paths = {'parent': parent, 'torch': torch_call, 'chain': chain}
        paths = {name: call for name, call in paths.items() if call}
        if parent:      # the same statistics after one update from the same state
          chain(), parent()
          a, b = parent.state.cpu().numpy(), chain.state.cpu().numpy()
          assert np.allclose(a, b, rtol=1e-6, atol=0), (n, impl, mode, a, b)
        got = pathbench.measure(paths, args.calls, args.rounds, timer=host_us)
        before = chain.launches()
        host_us(chain, 10)
        counted = (chain.launches() - before) / 10
        cell = lambda name: got[name].cell if name in got else 'not measured'
        report.add(f'  {n:<10}{impl:<9}{mode:<13}{cell("parent"):<34}{cell("torch"):<34}{cell("chain"):<34}{counted:.1f}')
        if parent:
          below[n] = below.get(n, True) and pathbench.median_below(got['chain'], got['parent'])
  wins = [n for n in GRID_SIZES if below.get(n)]
  report.add('# chain median below the one-workgroup median, both impls and both calls, at n = '
             + (', '.join(map(str, wins)) or 'no measured n') + f'; kNormGridMin: {wins[0] if wins else "not measured"}')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=20000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'normalize_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  parser.add_argument('--parent-lib', default=None)
  parser.add_argument('--chain-lib', default=None)
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
  grid_rows(report, args)
  report.write()


if __name__ == '__main__':
  main()
