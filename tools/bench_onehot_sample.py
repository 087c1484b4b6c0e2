"""Cost of the draw of a one-hot latent or an action (dreamerv3/rssm.py:87, 100,
dreamerv3/agent.py:18, 126, 192): the kernels of csrc/onehot_sample.hip against
the composed path of the same module and against a `torch.multinomial`
composition.

    python tools/bench_onehot_sample.py [--calls 1000] [--rounds 5] [--out profiles/onehot_sample_bench.txt]

Per shape (rows, groups, classes) and dtype two pieces (unimix 0.01, a new
offset every call):

  forward   `OneHot(logits, unimix).sample(seed, offset)` under autograd.
  fwd+bwd   the same and `(onehot * gout).sum().backward()`, the `.grad` dropped
            between calls.

on three paths:
  composed     `fused=False`: softmax, blend, log, `emb_philox_uniform`, cumsum,
               the comparison, argmax, one_hot and the straight-through expression.
  fused        `fused=True`: one launch forward, one backward.
  multinomial  softmax, blend, `torch.multinomial(probs, 1)`, one_hot and the
               straight-through expression: what a port without this library writes.
  entry        the forward's C entry point alone, buffers made once: what the
               fused call costs without the facade's host work.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused / multinomial.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `outs._sample_path` is set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import itertools
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402

# the RSSM's observe step, its imagination step, a large batch, the actor's head, and
# the switch-over from one segment of 64 lanes to two values per lane (64 | 65 classes)
SHAPES = [(16, 32, 32), (16, 32, 64), (1024, 32, 32), (1024, 32, 64), (16384, 32, 64), (1024, 1, 18), (1024, 32, 65)]
UNIMIX, SEED = 0.01, 0x9e3779b97f4a7c15
PATHS = ('composed', 'fused', 'multinomial')


def multinomial_sample(logits, unimix):
  x = logits.to(torch.float32)
  probs = torch.softmax(x, -1)
  probs = (1 - unimix) * probs + unimix / probs.shape[-1]
  with torch.no_grad():
    index = torch.multinomial(probs.view(-1, probs.shape[-1]), 1).view(probs.shape[:-1])
    onehot = torch.nn.functional.one_hot(index, probs.shape[-1]).to(torch.float32)
  return (onehot + (probs - probs.detach())).to(logits.dtype)


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'onehot_sample_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_onehot_sample needs a GPU'
  from embodied_amd import _lib, outs

  device = pathbench.device_line() + f'; outs.OneHot.sample, unimix {UNIMIX}, a new offset every call'
  report = pathbench.Report('bench_onehot_sample.py', args, device, [
      '# shape: rows x groups x classes',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# entry: emb_onehot_sample alone through the binding, buffers made once (forward rows only)',
      '# ops: device operations per call (torch.profiler window), composed / fused / multinomial',
      f'# {"shape":<22}{"piece":<10}{"composed us":<32}{"fused us":<32}{"multinomial us":<32}{"entry us":<10}ops',
  ])
  gen = np.random.default_rng(0)
  medians = {}
  for rows, groups, classes in SHAPES:
    for kind in ('f32', 'bf16'):
      dtype = torch.float32 if kind == 'f32' else torch.bfloat16
      shape = (rows, groups, classes)
      logits = torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda().to(dtype).requires_grad_()
      gout = torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).cuda().to(dtype)
      offsets = itertools.count()
      pieces = {}
      for path in PATHS:
        if path == 'multinomial':
          forward = lambda: multinomial_sample(logits, UNIMIX)
        else:
          forward = lambda fused=path == 'fused': outs.OneHot(logits, UNIMIX, fused=fused).sample(SEED, next(offsets))

        def both(forward=forward):
          logits.grad = None
          (forward() * gout).sum().backward()
        pieces[path] = {'forward': forward, 'fwd+bwd': both}
      # the same draw from both paths of the module before anything is timed (apart from draws on a boundary)
      a = outs.OneHot(logits, UNIMIX, fused=False).sample(SEED, 1)
      b = outs.OneHot(logits, UNIMIX, fused=True).sample(SEED, 1)
      assert (a != b).any(-1).float().mean().item() < 1e-3, (shape, kind)
      index, onehot = torch.empty(rows * groups, dtype=torch.int32, device='cuda'), torch.empty_like(logits)
      stream, x = _lib.raw_stream(logits.device), logits.detach()
      entry = lambda: _lib.api.emb_onehot_sample(
          x.data_ptr(), _lib.F32 if kind == 'f32' else _lib.BF16, rows, groups, classes, UNIMIX, 0, SEED, next(offsets),
          None, None, onehot.data_ptr(), stream)
      name = 'x'.join(str(s) for s in shape) + ' ' + kind
      for piece in ('forward', 'fwd+bwd'):
        paths = {path: pieces[path][piece] for path in PATHS}
        if piece == 'forward':
          paths['entry'] = entry
        got = pathbench.measure(paths, args.calls, args.rounds)
        ops = [None if args.no_profiler else pathbench.device_ops(paths[p]) for p in PATHS]
        median = medians[name, piece] = {p: got[p].median for p in paths}
        report.verdict(f'{name} {piece}', pathbench.median_below(got['fused'], got['composed']))
        alone = f'{median["entry"]:.1f}' if 'entry' in median else '-'
        report.add(f'  {name:<22}{piece:<10}{got["composed"].cell:<32}{got["fused"].cell:<32}{got["multinomial"].cell:<32}'
                   f'{alone:<10}{" / ".join(pathbench.count(n) for n in ops)}')
  report.closing()
  small, large = medians['16x32x32 f32', 'forward'], medians['1024x32x32 f32', 'forward']
  bound = small['fused'] > 2 * small['entry'] and small['fused'] > 0.8 * large['fused']
  report.add(
      f'# 16 rows against 1024 at 32 x 32 f32, forward: fused {small["fused"]:.1f} / {large["fused"]:.1f} us, the entry '
      f'point alone {small["entry"]:.1f} / {large["entry"]:.1f} us: the fused call at 16 rows is '
      + ('bound by the host\'s enqueue (the facade and the launch), not by the kernel' if bound else
         'not bound by the host\'s enqueue by this measure'))
  a, b = medians['1024x32x64 f32', 'forward'], medians['1024x32x65 f32', 'forward']
  report.add(f'# the switch-over at 64 | 65 classes (one segment | two values per lane), 1024 x 32, f32 forward: '
             f'fused {a["fused"]:.1f} | {b["fused"]:.1f} us, entry {a["entry"]:.1f} | {b["entry"]:.1f} us; '
             'the narrower switch-overs (2 .. 32 lanes) were not measured')
  report.write()


if __name__ == '__main__':
  main()
