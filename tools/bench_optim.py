"""Cost of one optimizer step: the kernels of csrc/optim.hip against the composed
torch ops of `embodied_amd.optim.LaProp`, and `torch.optim.Adam(fused=True)` as
context only (it does less work: no per-tensor norms, no clipping).

    python tools/bench_optim.py [--calls 200] [--rounds 5] [--out profiles/optim_bench.txt]

Three parameter sets, each with float32 and with bfloat16 gradients:
  small    about 1 M parameters in 40 tensors
  ppo      the counted PPO model (tools/count_params.py), 12.2 M parameters
  dreamer  the 200M DreamerV3 model, its tensors' shapes from the same walk

  us        time between two device events around `calls` back-to-back `step()`s
            ending in a synchronise, after a warm-up; the paths alternate inside
            every round; median of the rounds [min .. max].
  host us   wall time of the same calls up to the last enqueue, per step, measured
            from a drained device: what the host spends per step (for the fused
            path: gathering the addresses, comparing them with the table, two calls).
  ops       device operations (kernels, copies) per step in a torch.profiler
            window of its own, the annotation around `Optimizer.step` left out.
  ceiling   the fused step's algorithmic bytes per parameter -- the norms launch
            reads g and p, the update launch reads g, p, nu, mu and writes p, nu,
            mu: 36 with float32 gradients, 32 with bfloat16 ones -- over its median
            time, as a share of the copy ceiling that DESIGN.md quotes.
  norms     the norms launch alone (through the C ABI, the optimizer's tables) and
            its read rate; a rate above the copy ceiling says its reads were served
            from the Infinity Cache (g and p of the small sets fit; written by the
            backward pass and the previous update, they are there in a learner too).

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `optim._path` is set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import math
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from tools import count_params  # noqa: E402
from tools import pathbench  # noqa: E402
from tools.pathbench import COPY_CEILING_GBS, device_us, host_us  # noqa: E402


class Counted(int):
  """A parameter count that remembers the tensors it counts: the walk of
  tools/count_params.py, run with these, yields the shapes as well."""

  def __new__(cls, value, shapes=()):
    self = int.__new__(cls, value)
    self.shapes = tuple(shapes)
    return self

  @staticmethod
  def _shapes(other):
    return other.shapes if isinstance(other, Counted) else (((int(other),),) if other else ())   # a bare vector

  def __add__(self, other):
    return Counted(int(self) + int(other), self.shapes + self._shapes(other))

  def __radd__(self, other):
    return Counted(int(other) + int(self), self._shapes(other) + self.shapes)

  def __mul__(self, times):
    return Counted(int(self) * int(times), self.shapes * int(times))

  __rmul__ = __mul__


def walked_shapes(walk, *args):
  """The tensors of `count_params.ppo` / `.dreamer`: (shapes, total)."""
  saved = {name: getattr(count_params, name) for name in ('linear', 'block_linear', 'conv', 'norm')}
  try:
    count_params.linear = lambda i, o: Counted(i * o + o, ((i, o), (o,)))
    count_params.block_linear = lambda i, o, g: Counted(g * (i // g) * (o // g) + o, ((g, i // g, o // g), (o,)))
    count_params.conv = lambda k, i, o: Counted(k * k * i * o + o, ((k, k, i, o), (o,)))
    count_params.norm = lambda kind, n: Counted({'none': 0, 'rms': n, 'layer': 2 * n}[kind],
                                                {'none': (), 'rms': ((n,),), 'layer': ((n,), (n,))}[kind])
    parts = walk(*args)
  finally:
    for name, fn in saved.items():
      setattr(count_params, name, fn)
  total = sum(parts.values(), Counted(0))
  shapes = [s for s in total.shapes if math.prod(s)]
  assert sum(math.prod(s) for s in shapes) == int(total) == sum(int(v) for v in walk(*args).values())
  return shapes, int(total)


def parameter_sets():
  small = [(160, 160)] * 38 + [(160,)] * 2                                   # 973 120 parameters, 40 tensors
  ppo, _ = walked_shapes(count_params.ppo, count_params.PPO_AGENT, (84, 84, 4), 6)       # bench.py's shapes
  dreamer, _ = walked_shapes(count_params.dreamer, count_params.DREAMER_AGENT, (64, 64, 3), 0, 17)     # crafter
  return (('small', small), ('ppo', ppo), ('dreamer', dreamer))


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=200)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'optim_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  parser.add_argument('--sets', default='small,ppo,dreamer')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_optim needs a GPU'
  from embodied_amd import _lib, optim

  device = pathbench.device_line() + '; LaProp(lr=4e-5, agc=0.3, wd=0), one step()'
  report = pathbench.Report('bench_optim.py', args, device, [
      '# us: time between device events over back-to-back steps, per step: median of rounds [min .. max] (steps per round)',
      '# host us: wall time up to the last enqueue, per step; ops: device operations per step (torch.profiler window)',
      f'# ceiling: 36 (float32 gradients) or 32 (bfloat16) bytes per parameter / the fused median; copy ceiling '
      f'{COPY_CEILING_GBS:.0f} GB/s (read + write)',
      '# norms: the norms launch alone, 8 (6) bytes per parameter read; above the copy ceiling = served from the Infinity Cache',
      '# Adam: torch.optim.Adam(fused=True), context only (float32 gradients only: it takes no others)',
  ])
  torch.manual_seed(0)
  for name, shapes in parameter_sets():
    if name not in args.sets.split(','):
      continue
    count = sum(math.prod(s) for s in shapes)
    params = [torch.randn(s, device='cuda') * 0.05 for s in shapes]
    for kind in ('f32', 'bf16'):
      dtype = torch.float32 if kind == 'f32' else torch.bfloat16
      for p in params:
        p.grad_dtype = None
        p.grad = (torch.randn(p.shape, device='cuda') * 0.01).to(dtype)
      opts = {'composed': optim.LaProp(params, fused=False), 'fused': optim.LaProp(params, fused=True)}
      if kind == 'f32':
        opts['Adam'] = torch.optim.Adam(params, lr=4e-5, fused=True)
      steps = {k: opt.step for k, opt in opts.items()}
      got = pathbench.measure(steps, args.calls, args.rounds, warmup=(2, 3), floor=3)
      host = {k: statistics.median(host_us(step, got[k].calls, sync=False) for _ in range(3)) for k, step in steps.items()}
      ops = {k: None if args.no_profiler else pathbench.device_ops(step, skip='Optimizer.step')
             for k, step in steps.items()}
      plan = opts['fused']._plan
      norms = lambda: _lib.api.emb_optim_norms(plan['table'].data_ptr(), plan['chunks'].data_ptr(), plan['n_chunks'],
                                               plan['partials'].data_ptr(), _lib.raw_stream(plan['device']))
      device_us(norms, 3)
      norms_us = statistics.median(device_us(norms, max(10, got['fused'].calls)) for _ in range(args.rounds))
      assert opts['fused'].table_uploads == 1
      row = f'{name} {kind}'
      report.add(f'  {row}: {count} parameters in {len(shapes)} tensors, {plan["n_chunks"]} chunks of {optim.CHUNK}')
      for k in opts:
        report.add(f'    {k:<10}{pathbench.cell(got[k].values, got[k].calls, 10, " us")}'
                   f'   host {host[k]:8.1f} us   ops {pathbench.count(ops[k])}')
      per = 36 if kind == 'f32' else 32
      rate = per * count / got['fused'].median / 1e3
      read = (8 if kind == 'f32' else 6) * count / norms_us / 1e3
      report.add(f'    fused: {rate:.0f} GB/s = {rate / COPY_CEILING_GBS:.2f} of the ceiling; norms launch alone '
                 f'{norms_us:.1f} us = {read:.0f} GB/s read'
                 f' ({"above the copy ceiling: from the Infinity Cache" if read > COPY_CEILING_GBS else "below the copy ceiling"})')
      report.verdict(row, pathbench.median_below(got['fused'], got['composed']))
      del opts, steps, plan, norms
    for p in params:
      p.grad = None
    del params
    torch.cuda.empty_cache()
  report.closing()
  report.write()


if __name__ == '__main__':
  main()
