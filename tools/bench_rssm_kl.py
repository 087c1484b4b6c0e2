"""Cost of the RSSM's KL block of one train step (dreamerv3/rssm.py:123-132):
the composed torch ops against the kernels of csrc/onehot_kl.hip, and the
kernels' worst error against float64.

    python tools/bench_rssm_kl.py [--calls 1000] [--rounds 5] [--out profiles/rssm_kl_bench.txt]
                                  [--accuracy profiles/rssm_kl_accuracy.txt]

Per shape and dtype two pieces, each on both paths of `outs.rssm_kl`
(unimix 0.01, free_nats 1):

  forward   `rssm_kl(post, prior)` under autograd: the four outputs.
  fwd+bwd   the same and `(dyn * g_dyn + rep * g_rep).sum().backward()`, the
            `.grad`s dropped between calls.
and, for the kernels alone, `emb_onehot_kl` and `emb_onehot_kl_grad` called
through the C ABI on buffers made once (`fwd kernel`, `grad kernel`): the
facade's pieces above cost the larger of the host's enqueue time and the
device's time.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own.
  GB/s      for the two kernel rows: the bytes the kernel must move (forward:
            both tensors once; grad: both once and both gradients once) over the
            median time, beside the copy ceiling that DESIGN.md quotes.

The last lines name the shapes at which the kernels' median is below the
composed one, and those where it is not: what `outs._kl_path` is set from.
The accuracy file holds, per shape, dtype and unimix, the worst error of both
paths as a share of the bars of tests/test_gpu_rssm_kl.py: the shapes of that
test, then those of the sweep over every segment width
(tests/rssm_kl_sweep_cases.py).
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
from tools.pathbench import COPY_CEILING_GBS, device_us  # noqa: E402

SHAPES = [(rows, stoch, classes, kind) for rows in (1024, 16384) for stoch, classes in ((32, 32), (32, 64), (32, 96))
          for kind in ('f32', 'bf16')]
UNIMIX, FREE_NATS = 0.01, 1.0


def kernel_calls(post, prior, g_dyn, g_rep):
  """`emb_onehot_kl` and `emb_onehot_kl_grad` through the C ABI, buffers made once."""
  from embodied_amd import _lib
  from embodied_amd import outs
  x, y = post.detach(), prior.detach()
  rows, stoch, classes = x.shape
  dtype = outs._DTYPES[x.dtype]
  rowwise = torch.empty(5, rows, device=x.device)
  grads = torch.empty_like(x), torch.empty_like(y)
  stream = _lib.raw_stream(x.device)
  forward = lambda: _lib.api.emb_onehot_kl(
      x.data_ptr(), y.data_ptr(), dtype, rows, stoch, classes, UNIMIX, FREE_NATS, *[r.data_ptr() for r in rowwise],
      stream)
  backward = lambda: _lib.api.emb_onehot_kl_grad(
      x.data_ptr(), y.data_ptr(), dtype, rows, stoch, classes, UNIMIX, FREE_NATS, rowwise[0].data_ptr(),
      g_rep.data_ptr(), g_dyn.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), stream)
  forward()
  return forward, backward


def accuracy(outs, lines):
  from tests import rssm_kl_cases as cases
  from tests import rssm_kl_sweep_cases as sweep
  lines += ['# tools/bench_rssm_kl.py: worst error against float64 (tests.rssm_kl_cases.reference64) as a share of the bars',
            '# forward: |got - want| / (1e-5 + 1e-5 |want|) over dyn, rep and both entropies, free_nats 1 and 0;',
            '# gradient: |got - want| / (1e-5 |g| (1 + |want|)) per element (bf16: + 2^-8 |want|); rows 37, logit scales '
            + ', '.join(f'{s:g}' for s in cases.SCALES),
            '# unimix 0: gradients at scales 0.1 and 1 only (the float32 definition misses the bar beyond)',
            '# shapes: tests.rssm_kl_cases.FUSED_SHAPES, then every (stoch, classes) of tests.rssm_kl_sweep_cases, rung by rung',
            f'# {"shape":<12}{"dtype":<7}{"unimix":<8}{"fused fwd":<12}{"fused grad":<12}{"composed fwd":<14}composed grad']
  worst_all = {True: [0.0, 0.0], False: [0.0, 0.0]}
  shapes = list(cases.FUSED_SHAPES)
  shapes += [shape for shape in sweep.all_shapes() if shape not in shapes]
  for stoch, classes in shapes:
    for kind in ('f32', 'bf16'):
      for unimix in cases.UNIMIX:
        worst = {True: [0.0, 0.0], False: [0.0, 0.0]}
        for scale in cases.SCALES:
          rng = np.random.default_rng([stoch, classes, int(scale * 10)])
          post, prior = cases.logits_of(cases.ROWS, stoch, classes, scale, rng)
          if kind == 'bf16':
            post, prior = cases.bf16_round(post), cases.bf16_round(prior)
          g_dyn, g_rep = rng.standard_normal((2, cases.ROWS)).astype(np.float32)
          for free in cases.FREE_NATS:
            ref = cases.reference64(post, prior, unimix, free, g_dyn, g_rep)
            for fused in (True, False):
              dtype = torch.float32 if kind == 'f32' else torch.bfloat16
              p = torch.from_numpy(post).cuda().to(dtype).requires_grad_()
              q = torch.from_numpy(prior).cuda().to(dtype).requires_grad_()
              out = outs.rssm_kl(p, q, unimix=unimix, free_nats=free, fused=fused)
              (out['dyn'] * torch.from_numpy(g_dyn).cuda() + out['rep'] * torch.from_numpy(g_rep).cuda()).sum().backward()
              host = lambda t: t.detach().float().cpu().numpy()
              forward = max(cases.forward_ratio(host(out[a]), ref[b]) for a, b in (
                  ('dyn', 'dyn'), ('rep', 'rep'), ('dyn_ent', 'ent_prior'), ('rep_ent', 'ent_post')))
              worst[fused][0] = max(worst[fused][0], forward)
              if unimix or scale in cases.GRAD_SCALES_NO_UNIMIX:
                grad = max(cases.grad_ratio(host(p.grad), ref['grad_post'], g_rep, kind == 'bf16'),
                           cases.grad_ratio(host(q.grad), ref['grad_prior'], g_dyn, kind == 'bf16'))
                worst[fused][1] = max(worst[fused][1], grad)
        lines.append(f'  {f"{stoch}x{classes}":<12}{kind:<7}{unimix:<8g}{worst[True][0]:<12.3f}{worst[True][1]:<12.3f}'
                     f'{worst[False][0]:<14.3f}{worst[False][1]:.3f}')
        for fused in worst:
          worst_all[fused] = [max(a, b) for a, b in zip(worst_all[fused], worst[fused])]
  lines.append(f'# worst: fused forward {worst_all[True][0]:.3f}, gradient {worst_all[True][1]:.3f}; '
               f'composed forward {worst_all[False][0]:.3f}, gradient {worst_all[False][1]:.3f}')
  return lines


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'rssm_kl_bench.txt'))
  parser.add_argument('--accuracy', default=str(ROOT / 'profiles' / 'rssm_kl_accuracy.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_rssm_kl needs a GPU'
  from embodied_amd import outs

  device = pathbench.device_line()
  acc = accuracy(outs, [device])
  print('\n'.join(acc), flush=True)
  path = pathlib.Path(args.accuracy)
  path.parent.mkdir(parents=True, exist_ok=True)
  path.write_text('\n'.join(acc) + '\n')

  report = pathbench.Report('bench_rssm_kl.py', args, device + f'; outs.rssm_kl, unimix {UNIMIX}, free_nats {FREE_NATS}', [
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window); the kernel rows: the C entry point alone',
      f'# GB/s: bytes the kernel must move / median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<22}{"piece":<12}{"composed us":<34}{"fused us":<34}{"ops composed / fused":<22}fused GB/s',
  ])
  gen = np.random.default_rng(0)
  for rows, stoch, classes, kind in SHAPES:
    dtype = torch.float32 if kind == 'f32' else torch.bfloat16
    make = lambda: torch.from_numpy(gen.standard_normal((rows, stoch, classes)).astype(np.float32)).cuda().to(dtype)
    post, prior = make().requires_grad_(), make().requires_grad_()
    g_dyn, g_rep = (torch.from_numpy(gen.standard_normal(rows).astype(np.float32)).cuda() for _ in range(2))
    size = post.element_size() * post.numel()
    pieces = {}
    for fused in (False, True):
      forward = lambda fused=fused: outs.rssm_kl(post, prior, UNIMIX, FREE_NATS, fused=fused)

      def both(forward=forward):
        post.grad = prior.grad = None
        out = forward()
        (out['dyn'] * g_dyn + out['rep'] * g_rep).sum().backward()
      pieces[fused] = {'forward': forward, 'fwd+bwd': both}
    # the same values from both paths before anything is timed
    a, b = pieces[False]['forward'](), pieces[True]['forward']()
    for key in a:
      assert torch.allclose(a[key], b[key], rtol=2e-5, atol=2e-5), (rows, stoch, classes, kind, key)
    grads = []
    for f in (False, True):
      pieces[f]['fwd+bwd']()
      grads.append((post.grad.float().clone(), prior.grad.float().clone()))
    tol = 1e-4 if kind == 'f32' else 2.0 ** -6
    for x, y in zip(*grads):
      assert torch.allclose(x, y, rtol=tol, atol=1e-5), (rows, stoch, classes, kind, 'grad')
    name = f'{rows}x{stoch}x{classes} {kind}'
    for piece in ('forward', 'fwd+bwd'):
      paths = {f: pieces[f][piece] for f in (False, True)}
      got = pathbench.measure(paths, args.calls, args.rounds)
      ops = {f: None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths}
      report.verdict(f'{name} {piece}', pathbench.median_below(got[True], got[False]))
      report.add(f'  {name:<22}{piece:<12}{got[False].cell:<34}{got[True].cell:<34}'
                 f'{pathbench.count(ops[False]) + " / " + pathbench.count(ops[True]):<22}-')
    for piece, call, moved in zip(('fwd kernel', 'grad kernel'), kernel_calls(post, prior, g_dyn, g_rep),
                                  (2 * size, 4 * size)):
      device_us(call, 50)
      alone = pathbench.run_rounds({piece: call}, args.calls, args.rounds)[piece]
      rate = moved / alone.median / 1e3
      report.add(f'  {name:<22}{piece:<12}{"":<34}{alone.cell:<34}'
                 f'{"- / 1.0":<22}{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')
  report.closing(none='no measured shape')
  report.write()


if __name__ == '__main__':
  main()
