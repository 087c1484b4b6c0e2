"""Worst error of `nets.norm_act` and `nets.gru_gate` on the kernels against
float64 (tests.norm_act_cases.reference64, tests.gru_gate_cases.reference64), as
a share of the bars of tests/test_gpu_norm_act.py and tests/test_gpu_gru_gate.py.

    python tools/rssm_core_accuracy.py [--out profiles/rssm_core_accuracy.txt]

norm_act, per shape of the tests' width ladder (cases.LADDER), impl and dtype,
the worst over the four activations:
  out      |got - want| / (1e-5 + 1e-5 |want|)                (bf16: + 2^-8 |want|)
  dx       |got - want| / (1e-5 s (1 + |want| / s)), s = rstd max |gout scale|  (bf16: + 2^-8 |want|)
  dscale, dshift   |got - want| / (1e-5 sum |terms|)
gru_gate, per shape and dtype over the input scales 1, 5 and 30: out, dx and
ddeter with s = max |gout| max(1, max |x|, max |deter|).
Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'rssm_core_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'rssm_core_accuracy needs a GPU'
  from embodied_amd import nets
  from tests import gru_gate_cases as gates
  from tests import norm_act_cases as norms

  lines = [
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
      '# tools/rssm_core_accuracy.py: worst error of the kernels against float64 as a share of the bars',
      '# norm_act: tests.norm_act_cases.LADDER, eps 1e-4, scale and shift given, the worst over none / silu / gelu / relu',
      f'# {"rows x units":<16}{"impl":<7}{"dtype":<7}{"out":<10}{"dx":<10}{"dscale":<10}dshift']
  host = lambda t: t.detach().float().cpu().numpy()
  dev = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)
  top = {}
  for rows, units in norms.LADDER:
    for impl in norms.IMPLS:
      for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        worst = dict(out=0.0, dx=0.0, dscale=0.0, dshift=0.0)
        for act in norms.ACTS:
          inp = norms.inputs_of(rows, units, impl, True, 1.0, np.random.default_rng([rows, units, len(act)]))
          if kind == 'bf16':
            inp = dict(inp, x=norms.bf16_round(inp['x']), gout=norms.bf16_round(inp['gout']))
          want = norms.reference64(inp['x'], inp['scale'], inp['shift'], impl, act, 1e-4, inp['gout'])
          x, scale = dev(inp['x'], dtype).requires_grad_(), dev(inp['scale']).requires_grad_()
          shift = None if inp['shift'] is None else dev(inp['shift']).requires_grad_()
          out = nets.norm_act(x, scale, shift, impl, act, 1e-4, fused=True)
          out.backward(dev(inp['gout'], dtype))
          s = norms.row_scale(inp['gout'], inp['scale'], want['rstd'])
          bf16 = kind == 'bf16'
          got = dict(out=norms.out_ratio(host(out), want['out'], bf16), dx=norms.grad_ratio(host(x.grad), want['dx'], s, bf16),
                     dscale=norms.sum_ratio(host(scale.grad), want['dscale'], want['dscale_abs']))
          if shift is not None:
            got['dshift'] = norms.sum_ratio(host(shift.grad), want['dshift'], want['dshift_abs'])
          worst = {k: max(v, got.get(k, 0.0)) for k, v in worst.items()}
        top = {k: max(v, top.get('norm ' + k, 0.0)) for k, v in (('norm ' + k, v) for k, v in worst.items())} | {
            k: v for k, v in top.items() if not k.startswith('norm ')}
        lines.append(f'  {f"{rows} x {units}":<16}{impl:<7}{kind:<7}{worst["out"]:<10.3f}{worst["dx"]:<10.3f}'
                     f'{worst["dscale"]:<10.3f}{worst["dshift"]:.3f}')
  lines += ['# gru_gate: rows x deter / blocks, the worst over the input scales 1, 5 and 30',
            f'# {"shape":<20}{"dtype":<7}{"out":<10}{"dx":<10}ddeter']
  shapes = [(37, d, b) for d, b in gates.SHAPES] + [gates.LARGE, gates.STRIDED]
  for rows, deter, blocks in shapes:
    for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
      worst = dict(out=0.0, dx=0.0, ddeter=0.0)
      for scale in (1.0, 5.0, 30.0):
        inp = gates.inputs_of(rows, deter, scale, np.random.default_rng([rows, deter, int(scale)]))
        if kind == 'bf16':
          inp = {k: gates.bf16_round(v) for k, v in inp.items()}
        want = gates.reference64(inp['x'], inp['deter'], blocks, inp['gout'])
        x, d = dev(inp['x'], dtype).requires_grad_(), dev(inp['deter'], dtype).requires_grad_()
        out = nets.gru_gate(x, d, blocks, fused=True)
        out.backward(dev(inp['gout'], dtype))
        s = gates.row_scale(inp['gout'], inp['x'], inp['deter'])
        bf16 = kind == 'bf16'
        got = dict(out=gates.out_ratio(host(out), want['out'], bf16), dx=gates.grad_ratio(host(x.grad), want['dx'], s, bf16),
                   ddeter=gates.grad_ratio(host(d.grad), want['ddeter'], s, bf16))
        worst = {k: max(v, got[k]) for k, v in worst.items()}
      for k, v in worst.items():
        top['gate ' + k] = max(top.get('gate ' + k, 0.0), v)
      lines.append(f'  {f"{rows} x {deter} / {blocks}":<20}{kind:<7}{worst["out"]:<10.3f}{worst["dx"]:<10.3f}{worst["ddeter"]:.3f}')
  lines.append('# worst: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(top.items())))
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
