"""Cost of the tails of DreamerV3's convolution stages (dreamerv3/rssm.py:238-241 and
:327, 336-338, 346): the kernels of csrc/conv_stage.hip against the two things a
user could write without them.

    python tools/bench_conv_stage.py [--calls 1000] [--rounds 5] [--out profiles/conv_stage_bench.txt]

Per shape of x (the reference's own stages at depth 64, mults (2, 3, 4, 4), 64 x 64
frames, N = 16 and N = 1024 frames) and dtype, three paths of `nets.pool_norm_act`
/ `nets.norm_act_upsample` (rms, silu, a `scale` that takes a gradient):

  composed  `fused=False`: the definition, torch ops all the way.
  parent    what the library offered before these kernels: `amax` over the
            windows, then `nets.norm_act(fused=True)`; or `nets.norm_act(fused=True)`,
            then `repeat_interleave` twice.
  fused     `fused=True`: one launch forward, two backward (dx, then the sum of
            the partial column sums).

  forward   the call under autograd.
  fwd+bwd   the same and `.backward(gout)`, the `.grad`s dropped between calls.

  us        time between two device events around back-to-back calls ending in a
            synchronise, after a warm-up of the same shape; the paths alternate
            inside every round; median of the rounds [min .. max] (calls per round).
  GB/s      for the fused call: the bytes it must move over the median time, as
            a share of the copy ceiling that DESIGN.md quotes.  With S the bytes
            of x -- pool forward: x and the pooled result, 1.25 S; fwd+bwd: that,
            x again, gout and dx, 3.5 S; upsample forward: x and four copies,
            5 S; fwd+bwd: that, x again, gout and dx, 11 S.  The call includes the
            facade's host work, so at small shapes this is the host's rate.

The last lines name the rows at which the fused median is below both rivals',
and those where it is not: what `nets._pool_path` / `_upsample_path` are set from.
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

POOL_SHAPES = [(64, 64, 128), (32, 32, 192), (16, 16, 256), (8, 8, 256), (64, 64, 32)]
UPSAMPLE_SHAPES = [(4, 4, 256), (8, 8, 256), (16, 16, 192), (32, 32, 128)]
FRAMES = (16, 1024)
PATHS = ('composed', 'parent', 'fused')


def row(name, piece, got, moved):
  """One line of the file: the `pathbench.Rounds` of every path, the bytes the fused call moves."""
  rate = moved / got['fused'].median / 1e3
  return (f'  {name:<34}{piece:<9}{got["composed"].cell:<32}{got["parent"].cell:<32}{got["fused"].cell:<32}'
          f'{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'conv_stage_bench.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_conv_stage needs a GPU'
  from embodied_amd import nets

  device = pathbench.device_line() + '; nets.pool_norm_act and nets.norm_act_upsample (rms, silu, scale with a gradient)'
  report = pathbench.Report('bench_conv_stage.py', args, device, [
      '# shape: x as N x H x W x C; parent: amax + norm_act(fused=True), norm_act(fused=True) + repeat_interleave',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      f'# GB/s: bytes the fused call must move / its median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<34}{"piece":<9}{"composed us":<32}{"parent us":<32}{"fused us":<32}fused GB/s',
  ])
  gen = torch.Generator(device='cuda').manual_seed(0)

  def measure(name, pieces, moved):
    for piece in ('forward', 'fwd+bwd'):
      got = pathbench.measure({path: pieces[path][piece] for path in PATHS}, args.calls, args.rounds)
      report.verdict(f'{name} {piece}', pathbench.median_below(got['fused'], got['composed'], got['parent']))
      report.add(row(name, piece, got, moved[piece]))

  for stage, shapes in (('pool', POOL_SHAPES), ('upsample', UPSAMPLE_SHAPES)):
    call = nets.pool_norm_act if stage == 'pool' else nets.norm_act_upsample
    for height, width, units in shapes:
      for frames in FRAMES:
        for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
          x = torch.randn(frames, height, width, units, device='cuda', generator=gen).to(dtype).requires_grad_()
          scale = (1 + 0.3 * torch.randn(units, device='cuda', generator=gen)).requires_grad_()

          def parent():
            if stage == 'pool':
              pooled = x.reshape(frames, height // 2, 2, width // 2, 2, units).amax((2, 4))
              return nets.norm_act(pooled, scale, None, 'rms', 'silu', fused=True)
            return nets.norm_act(x, scale, None, 'rms', 'silu', fused=True).repeat_interleave(2, -2).repeat_interleave(2, -3)

          forwards = {'composed': lambda: call(x, scale, None, 'rms', 'silu', fused=False), 'parent': parent,
                      'fused': lambda: call(x, scale, None, 'rms', 'silu', fused=True)}
          results = {path: forward().detach() for path, forward in forwards.items()}
          gout = torch.randn(results['fused'].shape, device='cuda', generator=gen).to(dtype)
          # bfloat16: the composed path rounds after the norm and after every operation of the activation, a few ulps of 2^-8
          close = dict(rtol=2e-5, atol=2e-5) if kind == 'f32' else dict(rtol=2.0 ** -5, atol=2.0 ** -6)
          for path in ('composed', 'parent'):
            assert torch.allclose(results[path].float(), results['fused'].float(), **close), (stage, path, kind)
          del results
          pieces = {}
          for path, forward in forwards.items():
            def both(forward=forward):
              x.grad = scale.grad = None
              forward().backward(gout)
            pieces[path] = {'forward': forward, 'fwd+bwd': both}
          size = x.element_size() * x.numel()
          moved = ({'forward': 1.25 * size, 'fwd+bwd': 3.5 * size} if stage == 'pool' else
                   {'forward': 5 * size, 'fwd+bwd': 11 * size})
          measure(f'{stage} {frames}x{height}x{width}x{units} {kind}', pieces, moved)
          x.grad = scale.grad = None
          del x, gout, pieces, forwards
          torch.cuda.empty_cache()

  report.closing('fused median below both rivals at', 'fused median not below both rivals at')
  report.write()


if __name__ == '__main__':
  main()
