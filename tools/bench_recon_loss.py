"""Cost of the reconstruction terms of the world-model loss
(dreamerv3/agent.py:170-182): the kernels of csrc/recon_loss.hip against the
composed path of the same module.

    python tools/bench_recon_loss.py [--calls 1000] [--rounds 5] [--out profiles/recon_loss_bench.txt]

Per row two pieces:

  forward   the head's `.loss(target, dims)` under autograd.
  fwd+bwd   the same and `(loss * gout).sum().backward()`, the `.grad` dropped
            between calls.

on two paths, `fused=False` (torch ops restating the reference) and `fused=True`
(one launch forward, one backward):

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.
  GB/s      the bytes the fused call must move (forward: x and the target read
            once; backward: both read again and the gradient written) / its
            median time, and its share of the copy ceiling, 6290 GB/s.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `outs._recon_path` is set from.
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

# (head, shape of x, dims, dtype of x)
ROWS = [
    ('image', (1024, 64, 64, 3), 3, 'bf16'), ('image', (1024, 64, 64, 3), 3, 'f32'),
    ('image', (4096, 64, 64, 3), 3, 'bf16'), ('image', (4096, 64, 64, 3), 3, 'f32'),
    ('image', (1024, 96, 96, 3), 3, 'bf16'),
    ('symlog', (1024, 1024), 1, 'f32'), ('symlog', (1024, 7), 1, 'f32'),
    ('con', (1024,), 0, 'f32'), ('con', (16384,), 0, 'f32'),
]
PATHS = ('composed', 'fused')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'recon_loss_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_recon_loss needs a GPU'
  from embodied_amd import outs

  device = pathbench.device_line() + '; outs.ImageMSE (uint8 frames), outs.MSE(symlog), outs.Binary (uint8 labels)'
  report = pathbench.Report('bench_recon_loss.py', args, device, [
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"row":<30}{"piece":<10}{"composed us":<32}{"fused us":<32}{"ops":<16}fused GB/s',
  ])
  gen = np.random.default_rng(0)
  for head, shape, dims, kind in ROWS:
    dtype = torch.float32 if kind == 'f32' else torch.bfloat16
    x = torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda().to(dtype).requires_grad_()
    lead = shape[:len(shape) - dims]
    gout = torch.from_numpy(gen.standard_normal(lead).astype(np.float32)).cuda()
    if head == 'image':
      target = torch.from_numpy(gen.integers(0, 256, shape).astype(np.uint8)).cuda()
      make = lambda fused: outs.ImageMSE(x, fused=fused).loss(target, dims)
    elif head == 'symlog':
      target = torch.from_numpy((3 * gen.standard_normal(shape)).astype(np.float32)).cuda()
      make = lambda fused: outs.MSE(x, 'symlog', fused=fused).loss(target, dims)
    else:
      target = torch.from_numpy(gen.integers(0, 2, shape).astype(np.uint8)).cuda()
      make = lambda fused: outs.Binary(x, fused=fused).loss(target, dims)
    count = int(np.prod(shape))
    read = count * (x.element_size() + target.element_size())
    moved = {'forward': read + 4 * int(np.prod(lead)), 'fwd+bwd': 2 * read + count * x.element_size() + 8 * int(np.prod(lead))}
    pieces = {}
    for path in PATHS:
      forward = lambda fused=path == 'fused': make(fused)

      def both(forward=forward):
        x.grad = None
        (forward() * gout).sum().backward()
      pieces[path] = {'forward': forward, 'fwd+bwd': both}
    a, b = make(False), make(True)                                  # the same loss from both paths before anything is timed
    assert torch.allclose(a, b, rtol=1e-2 if kind == 'bf16' else 1e-4), (head, shape, kind)
    name = f'{head} ' + 'x'.join(str(s) for s in shape) + f' {kind}'
    for piece in ('forward', 'fwd+bwd'):
      paths = {path: pieces[path][piece] for path in PATHS}
      got = pathbench.measure(paths, args.calls, args.rounds)
      opcount = ' / '.join(pathbench.count(None if args.no_profiler else pathbench.device_ops(paths[p])) for p in PATHS)
      report.verdict(f'{name} {piece}', pathbench.median_below(got['fused'], got['composed']))
      rate = moved[piece] / got['fused'].median * 1e-3
      report.add(f'  {name:<30}{piece:<10}{got["composed"].cell:<32}{got["fused"].cell:<32}{opcount:<16}'
                 f'{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling ({moved[piece] / 1e6:.1f} MB)')
  report.closing()
  report.write()


if __name__ == '__main__':
  main()
