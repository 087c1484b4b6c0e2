"""Cost of the RSSM's norm + activation and of its blocked GRU gate
(embodied/jax/nets.py:361-399, nets.py:26-39, dreamerv3/rssm.py:152-159): the
composed torch ops against the kernels of csrc/norm_act.hip and csrc/gru_gate.hip.

    python tools/bench_rssm_core.py [--calls 1000] [--rounds 5] [--out profiles/rssm_core_bench.txt]

Per shape and dtype two pieces, each on both paths of `nets.norm_act` (rms, silu,
a `scale` that takes a gradient) and `nets.gru_gate`:

  forward   the call under autograd.
  fwd+bwd   the same and `.backward(gout)`, the `.grad`s dropped between calls.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.
  GB/s      for the fused call: the bytes it must move (norm forward: x and out;
            fwd+bwd: x twice, out, gout and dx; gate forward: x, deter and out;
            fwd+bwd: x and deter twice, out, gout, dx and ddeter) over the median
            time, as a share of the copy ceiling that DESIGN.md quotes.  The call
            includes the facade's host work, so at small shapes this is the
            host's rate, not the kernel's.
The norm also gets a row for `torch.nn.functional.rms_norm` + `silu` where that
function exists (in the `composed` column, named `F.rms_norm`).

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `nets._norm_path` / `_gate_path` are set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from tools import pathbench  # noqa: E402
from tools.pathbench import COPY_CEILING_GBS  # noqa: E402

NORM_SHAPES = [(16, 1024), (1024, 1024), (16384, 1024), (16, 8192), (1024, 8192)]
GATE_SHAPES = [(16, 8192, 8), (1024, 8192, 8), (4096, 8192, 8), (1024, 512, 8)]


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'rssm_core_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_rssm_core needs a GPU'
  from embodied_amd import nets

  device = pathbench.device_line() + '; nets.norm_act (rms, silu, scale with a gradient) and nets.gru_gate'
  report = pathbench.Report('bench_rssm_core.py', args, device, [
      '# shape: norm rows x units; gate rows x deter / blocks',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<40}{"piece":<10}{"composed us":<34}{"fused us":<34}{"ops composed / fused":<22}fused GB/s',
  ])
  gen = torch.Generator(device='cuda').manual_seed(0)

  def measure(name, pieces, moved, baseline='composed'):
    for piece in ('forward', 'fwd+bwd'):
      paths = {f: pieces[f][piece] for f in (False, True)}
      got = pathbench.measure(paths, args.calls, args.rounds)
      ops = {f: None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths}
      if baseline == 'composed':
        report.verdict(f'{name} {piece}', pathbench.median_below(got[True], got[False]))
      rate = moved[piece] / got[True].median / 1e3
      label = name if baseline == 'composed' else f'{name} vs {baseline}'
      report.add(f'  {label:<40}{piece:<10}{got[False].cell:<34}{got[True].cell:<34}'
                 f'{pathbench.count(ops[False]) + " / " + pathbench.count(ops[True]):<22}'
                 f'{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')

  for rows, units in NORM_SHAPES:
    for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
      x = torch.randn(rows, units, device='cuda', generator=gen).to(dtype).requires_grad_()
      gout = torch.randn(rows, units, device='cuda', generator=gen).to(dtype)
      scale = (1 + 0.3 * torch.randn(units, device='cuda', generator=gen)).requires_grad_()
      size = x.element_size() * x.numel()
      pieces = {}
      for fused in (False, True):
        forward = lambda fused=fused: nets.norm_act(x, scale, None, 'rms', 'silu', fused=fused)

        def both(forward=forward):
          x.grad = scale.grad = None
          forward().backward(gout)
        pieces[fused] = {'forward': forward, 'fwd+bwd': both}
      a, b = pieces[False]['forward'](), pieces[True]['forward']()
      # bfloat16: the composed path rounds after the norm and after every operation of the activation, a few ulps of 2^-8
      assert torch.allclose(a.float(), b.float(), rtol=2e-5 if kind == 'f32' else 2.0 ** -5, atol=2e-5 if kind == 'f32' else 2.0 ** -6), (rows, units, kind)
      moved = {'forward': 2 * size, 'fwd+bwd': 5 * size}
      name = f'norm {rows}x{units} {kind}'
      measure(name, pieces, moved)
      if hasattr(torch.nn.functional, 'rms_norm'):
        F = torch.nn.functional
        library = lambda: F.silu(F.rms_norm(x, (units,), scale.to(x.dtype), 1e-4))

        def library_both():
          x.grad = scale.grad = None
          library().backward(gout)
        measure(name, {False: {'forward': library, 'fwd+bwd': library_both}, True: pieces[True]}, moved, 'F.rms_norm')

  for rows, deter, blocks in GATE_SHAPES:
    for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
      x = torch.randn(rows, 3 * deter, device='cuda', generator=gen).to(dtype).requires_grad_()
      d = torch.randn(rows, deter, device='cuda', generator=gen).to(dtype).requires_grad_()
      gout = torch.randn(rows, deter, device='cuda', generator=gen).to(dtype)
      size = d.element_size() * d.numel()
      pieces = {}
      for fused in (False, True):
        forward = lambda fused=fused: nets.gru_gate(x, d, blocks, fused=fused)

        def both(forward=forward):
          x.grad = d.grad = None
          forward().backward(gout)
        pieces[fused] = {'forward': forward, 'fwd+bwd': both}
      a, b = pieces[False]['forward'](), pieces[True]['forward']()
      assert torch.allclose(a.float(), b.float(), rtol=2e-5 if kind == 'f32' else 2.0 ** -5, atol=2e-5 if kind == 'f32' else 2.0 ** -6)
      measure(f'gate {rows}x{deter}/{blocks} {kind}', pieces, {'forward': 5 * size, 'fwd+bwd': 14 * size})

  report.closing()
  report.write()


if __name__ == '__main__':
  main()
