"""How far `nets.pool_norm_act` / `nets.norm_act_upsample` sit from the float64
restatement of tests/conv_stage_cases.py, as the worst share of each bar of
tests/norm_act_cases.py (out, dx, dscale, dshift; 1.0 is the bar), per stage,
path and dtype, over every width of the tests at 310 Norm rows, both impls and
the four activations.

    python tools/conv_stage_accuracy.py [--out profiles/conv_stage_accuracy.txt]

bfloat16 on the composed path is listed for the record: it rounds between norm
and activation as the reference does, the difference `norm_act` documents, and
is not held to the bars.  Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import conv_stage_cases as stages  # noqa: E402


def run(call, inp, impl, act, kind, fused):
  dtype = torch.float32 if kind == 'f32' else torch.bfloat16
  dev = lambda a, t=torch.float32: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().to(t)
  x, scale, shift = dev(inp['x'], dtype).requires_grad_(), dev(inp['scale']).requires_grad_(), dev(inp['shift'])
  if shift is not None:
    shift.requires_grad_()
  out = call(x, scale, shift, impl, act, 1e-4, fused=fused)
  out.backward(dev(inp['gout'], dtype))
  host = lambda t: None if t is None else t.detach().float().cpu().numpy()
  return host(out), host(x.grad), host(scale.grad), None if shift is None else host(shift.grad)


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'conv_stage_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'conv_stage_accuracy needs a GPU'
  from embodied_amd import nets
  lines = ['# tools/conv_stage_accuracy.py',
           f'# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; worst share of each bar of tests/norm_act_cases.py',
           f'# over C in {stages.UNITS}, 310 Norm rows, impl rms / layer, act none / silu / gelu / relu, affine',
           f'# {"stage":<10}{"path":<10}{"dtype":<7}{"out":<10}{"dx":<10}{"dscale":<10}dshift']
  for stage in stages.STAGES:
    call = nets.pool_norm_act if stage == 'pool' else nets.norm_act_upsample
    height, width = (10, 62) if stage == 'pool' else (5, 31)
    for fused in (True, False):
      for kind in ('f32', 'bf16'):
        worst = {}
        for step, units in enumerate(stages.UNITS):
          for k, impl in enumerate(stages.IMPLS):
            act = stages.ACTS[(step + k) % 4]
            inp = stages.inputs_of(stage, 2, height, width, units, impl, True, 1.0, np.random.default_rng([units, k]))
            if kind == 'bf16':
              inp = dict(inp, x=stages.bf16_round(inp['x']), gout=stages.bf16_round(inp['gout']))
            want = stages.reference(stage, inp['x'], inp['scale'], inp['shift'], impl, act, 1e-4, inp['gout'])
            found = stages.ratios(stage, want, *run(call, inp, impl, act, kind, fused), kind == 'bf16', True)
            for key, ratio in found.items():
              worst[key] = max(worst.get(key, 0.0), ratio)
        cells = ''.join(f'{worst.get(key, float("nan")):<10.3g}' for key in ('out', 'dx', 'dscale', 'dshift'))
        note = '   (not held: the documented rounding difference)' if kind == 'bf16' and not fused else ''
        lines.append(f'  {stage:<10}{"fused" if fused else "composed":<10}{kind:<7}{cells}{note}')
        print(lines[-1], flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
