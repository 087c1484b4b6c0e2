"""Cost of the actor's loss of one train step (dreamerv3/agent.py:411-415) for a
continuous action key, and of its draw: the composed torch ops against the
kernels of csrc/normal_policy.hip.

    python tools/bench_normal_policy.py [--calls 1000] [--rounds 5] [--out profiles/normal_policy_bench.txt]

Per shape (N, T, A) and dtype three pieces, each on both paths at identical
inputs (`bounded`, minstd 0.1, maxstd 1, actent 3e-4, drop_last, weight (N, T)):

  forward   `normal_policy_loss(mean_raw, std_raw, act, adv, weight)` under
            autograd: the three outputs.
  fwd+bwd   the same and `(loss * gout).sum().backward()`, the `.grad`s dropped
            between calls.
  sample    `Normal(mean_raw, std_raw).sample(seed, offset)`.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  enqueue   for the fused call: host time per call of issuing the same calls
            without waiting for the device (median of the rounds).  Where the
            device-event figure is within 15 % of it the row is marked `host`:
            the figure is what the host needs to enqueue a call, not what the
            kernel takes.
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.
  GB/s      for the fused call: the bytes it must move (forward: both raw inputs
            and the actions once; fwd+bwd: those twice and both gradients once;
            sample: both raw inputs read, the actions written) over the median
            time, as a share of the copy ceiling that DESIGN.md quotes.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `outs._normal_path` is set from.  The
comparison is against the composed path of the same commit and nothing else.
Needs a GPU: there is no CPU fallback and no figure without one.
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
from tools.pathbench import COPY_CEILING_GBS  # noqa: E402

SHAPES = [(n, 16, actions, kind) for n in (1024, 16384) for actions in (1, 6, 21, 38) for kind in ('f32', 'bf16')]
KIND, MINSTD, MAXSTD, ACTENT = 'bounded', 0.1, 1.0, 3e-4


def row(name, piece, composed, fused, enqueue, ops, moved):
  """One line of the file: the two paths' `pathbench.Rounds`, the fused call's enqueue time (median of the rounds),
  the operation counts, the bytes the fused call moves."""
  rate = moved / fused.median / 1e3
  bound = f'{enqueue:.1f}' + (' host' if fused.median <= 1.15 * enqueue else '')
  counts = pathbench.count(ops[0]) + ' / ' + pathbench.count(ops[1])
  return (f'  {name:<22}{piece:<10}{composed.cell:<34}{fused.cell:<34}{bound:<14}'
          f'{counts:<22}{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'normal_policy_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_normal_policy needs a GPU'
  from embodied_amd import outs

  device = (pathbench.device_line() + f'; outs.normal_policy_loss / Normal.sample, {KIND} ({MINSTD}, {MAXSTD}), '
            f'actent {ACTENT}, drop_last, weight (N, T)')
  report = pathbench.Report('bench_normal_policy.py', args, device, [
      '# shape: N x T x A',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# enqueue: host time per fused call without waiting for the device; `host`: the fused us is the enqueue time',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<22}{"piece":<10}{"composed us":<34}{"fused us":<34}{"enqueue us":<14}{"ops composed / fused":<22}fused GB/s',
  ])
  gen = np.random.default_rng(0)
  for n, t, actions, kind in SHAPES:
    dtype = torch.float32 if kind == 'f32' else torch.bfloat16
    shape = (n, t, actions)
    raw = lambda: torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda().to(dtype).requires_grad_()
    mean_raw, std_raw = raw(), raw()
    act = torch.from_numpy(gen.uniform(-1, 1, shape).astype(np.float32)).cuda()
    adv, gout = (torch.from_numpy(gen.standard_normal((n, t - 1)).astype(np.float32)).cuda() for _ in range(2))
    weight = torch.from_numpy(np.cumprod(0.997 * (gen.random((n, t)) > 0.01), 1).astype(np.float32)).cuda()
    count = mean_raw.numel()
    inputs = 2 * mean_raw.element_size() * count
    pieces = {}
    for fused in (False, True):
      forward = lambda fused=fused: outs.normal_policy_loss(
          mean_raw, std_raw, act, adv, weight, ACTENT, KIND, MINSTD, MAXSTD, fused=fused)

      def both(forward=forward):
        mean_raw.grad = std_raw.grad = None
        (forward()['loss'] * gout).sum().backward()

      sample = lambda fused=fused: outs.Normal(mean_raw, std_raw, KIND, MINSTD, MAXSTD, fused=fused).sample(7, 11)
      pieces[fused] = {'forward': forward, 'fwd+bwd': both, 'sample': sample}
    # the same values from both paths before anything is timed
    a, b = pieces[False]['forward'](), pieces[True]['forward']()
    for key in a:
      assert torch.allclose(a[key], b[key], rtol=2e-5, atol=2e-4), (shape, kind, key)
    grads = []
    for f in (False, True):
      pieces[f]['fwd+bwd']()
      grads.append((mean_raw.grad.float().clone(), std_raw.grad.float().clone()))
    for x, y in zip(*grads):
      assert torch.allclose(x, y, rtol=1e-4 if kind == 'f32' else 2.0 ** -6, atol=1e-5), (shape, kind, 'grad')
    assert torch.allclose(pieces[False]['sample'](), pieces[True]['sample'](), rtol=1e-6, atol=1e-6), (shape, kind)
    name = 'x'.join(str(s) for s in shape) + ' ' + kind
    moves = (('forward', inputs + 4 * count), ('fwd+bwd', 2 * (inputs + 4 * count) + inputs), ('sample', inputs + 4 * count))
    for piece, moved in moves:
      paths, issue = {f: pieces[f][piece] for f in (False, True)}, []
      enqueue = lambda calls: issue.append(pathbench.host_us(paths[True], calls[True], sync=False))
      got = pathbench.measure(paths, args.calls, args.rounds, after_round=enqueue)
      ops = [None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths]
      report.verdict(f'{name} {piece}', pathbench.median_below(got[True], got[False]))
      report.add(row(name, piece, got[False], got[True], statistics.median(issue), ops, moved))
  report.closing()
  report.write()


if __name__ == '__main__':
  main()
