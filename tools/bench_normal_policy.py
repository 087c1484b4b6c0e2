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
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_twohot import COPY_CEILING_GBS, device_ops, device_us  # noqa: E402

SHAPES = [(n, 16, actions, kind) for n in (1024, 16384) for actions in (1, 6, 21, 38) for kind in ('f32', 'bf16')]
KIND, MINSTD, MAXSTD, ACTENT = 'bounded', 0.1, 1.0, 3e-4


def enqueue_us(fn, calls):
  """Host time per call of issuing `calls` calls; the device is waited for outside the clock."""
  torch.cuda.synchronize()
  start = time.perf_counter()
  for _ in range(calls):
    fn()
  stop = time.perf_counter()
  torch.cuda.synchronize()
  return (stop - start) * 1e6 / calls


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'normal_policy_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_normal_policy needs a GPU'
  from embodied_amd import outs

  lines = [
      f'# tools/bench_normal_policy.py --calls {args.calls} --rounds {args.rounds}',
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}'
      f'; outs.normal_policy_loss / Normal.sample, {KIND} ({MINSTD}, {MAXSTD}), actent {ACTENT}, drop_last, weight (N, T)',
      '# shape: N x T x A',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# enqueue: host time per fused call without waiting for the device; `host`: the fused us is the enqueue time',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<22}{"piece":<10}{"composed us":<34}{"fused us":<34}{"enqueue us":<14}{"ops composed / fused":<22}fused GB/s',
  ]
  print('\n'.join(lines), flush=True)
  gen = np.random.default_rng(0)
  wins, losses = [], []
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
      def timed(fused, calls):
        return device_us(pieces[fused][piece], calls)
      calls, rounds, issue = {}, {False: [], True: []}, []
      for fused in rounds:                             # warm-up of this shape; sizes the rounds
        timed(fused, 3)
        estimate = timed(fused, 5)
        calls[fused] = int(min(args.calls, max(5, 0.1e6 / estimate)))
      for _ in range(args.rounds):
        for fused in rounds:
          rounds[fused].append(timed(fused, calls[fused]))
        issue.append(enqueue_us(pieces[True][piece], calls[True]))
      ops = {f: None if args.no_profiler else device_ops(pieces[f][piece]) for f in rounds}
      median = {f: statistics.median(rounds[f]) for f in rounds}
      enqueue = statistics.median(issue)
      cell = lambda f: f'{median[f]:9.1f} [{min(rounds[f]):.1f} .. {max(rounds[f]):.1f}] ({calls[f]})'
      number = lambda f: 'not measured' if ops[f] is None else f'{ops[f]:.1f}'
      (wins if median[True] < median[False] else losses).append(f'{name} {piece}')
      rate = moved / median[True] / 1e3
      bound = f'{enqueue:.1f}' + (' host' if median[True] <= 1.15 * enqueue else '')
      line = (f'  {name:<22}{piece:<10}{cell(False):<34}{cell(True):<34}{bound:<14}'
              f'{number(False) + " / " + number(True):<22}{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')
      lines.append(line)
      print(line, flush=True)
  lines.append('# fused median below composed median at: ' + (', '.join(wins) or 'no measured row'))
  lines.append('# fused median not below composed median at: ' + (', '.join(losses) or 'no measured row'))
  print('\n'.join(lines[-2:]), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
