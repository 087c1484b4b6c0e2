"""Cost of the actor's loss of one train step (dreamerv3/agent.py:411-415): the
composed torch ops against the kernels of csrc/policy_loss.hip.

    python tools/bench_policy_loss.py [--calls 1000] [--rounds 5] [--out profiles/policy_loss_bench.txt]

Per shape (N, T, [groups,] classes) and dtype two pieces, each on both paths of
`outs.policy_loss` (unimix 0, actent 3e-4, drop_last, weight (N, T)):

  forward   `policy_loss(logits, act, adv, weight)` under autograd: the three outputs.
  fwd+bwd   the same and `(loss * gout).sum().backward()`, the `.grad` dropped
            between calls.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.
  GB/s      for the fused call: the bytes it must move (forward: the logits
            once; fwd+bwd: the logits twice and the gradient once) over the median
            time, as a share of the copy ceiling that DESIGN.md quotes.  The call
            includes the facade's host work, so at small shapes this is the
            host's rate, not the kernel's.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `outs._policy_path` is set from.
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
from tools.pathbench import COPY_CEILING_GBS  # noqa: E402

SHAPES = [(n, 16, groups, classes, kind) for n in (1024, 16384) for classes in (6, 18, 256) for groups in (0, 4)
          for kind in ('f32', 'bf16')]
UNIMIX, ACTENT = 0.0, 3e-4


def row(name, piece, composed, fused, ops, moved):
  """One line of the file: the two paths' `pathbench.Rounds`, their operation counts, the bytes the fused call moves."""
  rate = moved / fused.median / 1e3
  counts = pathbench.count(ops[0]) + ' / ' + pathbench.count(ops[1])
  return (f'  {name:<26}{piece:<10}{composed.cell:<34}{fused.cell:<34}{counts:<22}'
          f'{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'policy_loss_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_policy_loss needs a GPU'
  from embodied_amd import outs

  device = pathbench.device_line() + f'; outs.policy_loss, unimix {UNIMIX}, actent {ACTENT}, drop_last, weight (N, T)'
  report = pathbench.Report('bench_policy_loss.py', args, device, [
      '# shape: N x T x [groups x] classes',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<26}{"piece":<10}{"composed us":<34}{"fused us":<34}{"ops composed / fused":<22}fused GB/s',
  ])
  gen = np.random.default_rng(0)
  for n, t, groups, classes, kind in SHAPES:
    dtype = torch.float32 if kind == 'f32' else torch.bfloat16
    shape = (n, t, groups, classes) if groups else (n, t, classes)
    logits = torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda().to(dtype).requires_grad_()
    act = torch.from_numpy(gen.integers(0, classes, shape[:-1]).astype(np.int32)).cuda()
    adv, gout = (torch.from_numpy(gen.standard_normal((n, t - 1)).astype(np.float32)).cuda() for _ in range(2))
    weight = torch.from_numpy(np.cumprod(0.997 * (gen.random((n, t)) > 0.01), 1).astype(np.float32)).cuda()
    size = logits.element_size() * logits.numel()
    pieces = {}
    for fused in (False, True):
      forward = lambda fused=fused: outs.policy_loss(
          logits, act, adv, weight, actent=ACTENT, unimix=UNIMIX, dims=1 if groups else 0, fused=fused)

      def both(forward=forward):
        logits.grad = None
        (forward()['loss'] * gout).sum().backward()
      pieces[fused] = {'forward': forward, 'fwd+bwd': both}
    # the same values from both paths before anything is timed
    a, b = pieces[False]['forward'](), pieces[True]['forward']()
    for key in a:
      assert torch.allclose(a[key], b[key], rtol=2e-5, atol=2e-5), (shape, kind, key)
    grads = []
    for f in (False, True):
      pieces[f]['fwd+bwd']()
      grads.append(logits.grad.float().clone())
    assert torch.allclose(*grads, rtol=1e-4 if kind == 'f32' else 2.0 ** -6, atol=1e-5), (shape, kind, 'grad')
    name = 'x'.join(str(s) for s in shape) + ' ' + kind
    for piece, moved in (('forward', size), ('fwd+bwd', 3 * size)):
      paths = {f: pieces[f][piece] for f in (False, True)}
      got = pathbench.measure(paths, args.calls, args.rounds)
      ops = [None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths]
      report.verdict(f'{name} {piece}', pathbench.median_below(got[True], got[False]))
      report.add(row(name, piece, got[False], got[True], ops, moved))
  report.closing()
  report.write()


if __name__ == '__main__':
  main()
