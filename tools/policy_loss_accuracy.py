"""Worst error of `outs.policy_loss` on both paths against float64
(tests.policy_loss_cases.reference64), as a share of the bars of
tests/test_gpu_policy_loss.py.

    python tools/policy_loss_accuracy.py [--out profiles/policy_loss_accuracy.txt]

Per shape (groups x classes; groups 0: no group axis), dtype and unimix, over
every logit scale of the cases module at (N, T) = (37, 4) with drop_last:
  forward   |got - want| / (1e-5 + 1e-5 |want|) over loss, logpi and ent
  gradient  |got - want| / (1e-5 s (1 + |want| / s)), s = |gout weight| (|adv| + actent)
            (a bfloat16 gradient: + 2^-8 |want|)
Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, T = 37, 4


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'policy_loss_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'policy_loss_accuracy needs a GPU'
  from embodied_amd import outs
  from tests import policy_loss_cases as cases

  lines = [
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
      '# tools/policy_loss_accuracy.py: worst error against float64 (tests.policy_loss_cases.reference64) as a share of the bars',
      '# forward: |got - want| / (1e-5 + 1e-5 |want|) over loss, logpi and ent;',
      '# gradient: |got - want| / (1e-5 s (1 + |want| / s)), s = |gout weight| (|adv| + actent) (bf16: + 2^-8 |want|);',
      f'# (N, T) = ({N}, {T}), drop_last, actent {cases.ACTENT:g}, logit scales ' + ', '.join(f'{s:g}' for s in cases.SCALES),
      '# shapes: tests.policy_loss_cases.FUSED_SHAPES (groups x classes; groups 0: no group axis)',
      f'# {"shape":<12}{"dtype":<7}{"unimix":<8}{"fused fwd":<12}{"fused grad":<12}{"composed fwd":<14}composed grad']
  host = lambda t: t.detach().float().cpu().numpy()
  worst_all = {True: [0.0, 0.0], False: [0.0, 0.0]}
  for groups, classes in cases.FUSED_SHAPES:
    for kind in ('f32', 'bf16'):
      for unimix in cases.UNIMIX:
        worst = {True: [0.0, 0.0], False: [0.0, 0.0]}
        for scale in cases.SCALES:
          rng = np.random.default_rng([groups, classes, int(scale * 10)])
          logits = cases.logits_of(N, T, groups, classes, scale, rng)
          if kind == 'bf16':
            logits = cases.bf16_round(logits)
          act = cases.actions_of(N, T, groups, classes, rng)
          adv, gout = (2 * rng.standard_normal((2, N, T - 1))).astype(np.float32)
          weight = np.cumprod(0.997 * (rng.random((N, T)) > 0.05), 1).astype(np.float32)
          dims = 1 if groups else 0
          ref = cases.reference64(logits, act, adv, weight, cases.ACTENT, unimix, dims, 1, gout)
          s = cases.row_scale(gout, weight[:, :-1], adv, cases.ACTENT)
          for fused in (True, False):
            x = torch.from_numpy(logits).cuda().to(torch.float32 if kind == 'f32' else torch.bfloat16).requires_grad_()
            out = outs.policy_loss(x, torch.from_numpy(act).cuda(), torch.from_numpy(adv).cuda(),
                                   torch.from_numpy(weight).cuda(), actent=cases.ACTENT, unimix=unimix, dims=dims,
                                   fused=fused)
            (out['loss'] * torch.from_numpy(gout).cuda()).sum().backward()
            forward = max(cases.forward_ratio(host(out[key]), ref[key]) for key in cases.FIELDS)
            grad = cases.grad_ratio(host(x.grad)[:, :-1], ref['grad'][:, :-1], s, kind == 'bf16')
            worst[fused] = [max(worst[fused][0], forward), max(worst[fused][1], grad)]
        lines.append(f'  {f"{groups}x{classes}":<12}{kind:<7}{unimix:<8g}{worst[True][0]:<12.3f}{worst[True][1]:<12.3f}'
                     f'{worst[False][0]:<14.3f}{worst[False][1]:.3f}')
        for fused in worst:
          worst_all[fused] = [max(a, b) for a, b in zip(worst_all[fused], worst[fused])]
  lines.append(f'# worst: fused forward {worst_all[True][0]:.3f}, gradient {worst_all[True][1]:.3f}; '
               f'composed forward {worst_all[False][0]:.3f}, gradient {worst_all[False][1]:.3f}')
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
