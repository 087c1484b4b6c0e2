"""Worst error of `outs.OneHot.sample` on both paths against float64
(tests.onehot_sample_cases), as a share of the bars of
tests/test_gpu_onehot_sample.py.

    python tools/onehot_sample_accuracy.py [--out profiles/onehot_sample_accuracy.txt]

Per shape (groups x classes; groups 0: no group axis), dtype and unimix, over
every logit scale of the cases module at 37 rows:
  gradient  |got - want| / (1e-5 s (1 + |want| / s)), s = (1 - unimix) max |g| over
            the group, want the float64 autograd of the reference expression
            (a bfloat16 gradient: + 2^-8 |want|)
  refused   draws outside the acceptance rule C64[k - 1] - tol <= u < C64[k] + tol,
            tol = (classes + 8) 2^-23 (the tests assert none)
  near      draws within tol of a boundary of the float64 CDF, where either
            neighbour is accepted
Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROWS, SEED = 37, 0x9e3779b97f4a7c15


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'onehot_sample_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'onehot_sample_accuracy needs a GPU'
  from embodied_amd import outs
  from tests import onehot_sample_cases as cases

  lines = [
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
      '# tools/onehot_sample_accuracy.py: worst error against float64 (tests.onehot_sample_cases) as a share of the bars',
      '# gradient: |got - want| / (1e-5 s (1 + |want| / s)), s = (1 - unimix) max |g| over the group (bf16: + 2^-8 |want|);',
      '# refused / near: draws outside the acceptance rule / within tol = (classes + 8) 2^-23 of a boundary, of all draws;',
      f'# {ROWS} rows, logit scales ' + ', '.join(f'{s:g}' for s in cases.SCALES) + ', the Philox stream\'s uniforms',
      '# shapes: tests.onehot_sample_cases.FUSED_SHAPES (groups x classes; groups 0: no group axis)',
      f'# {"shape":<12}{"dtype":<7}{"unimix":<8}{"fused grad":<12}{"composed grad":<15}{"fused refused / near / draws":<30}'
      'composed refused / near / draws']
  host = lambda t: t.detach().float().cpu().numpy()
  worst_all = {True: 0.0, False: 0.0}
  for groups, classes in cases.FUSED_SHAPES:
    tol = cases.tol_of(classes)
    for kind in ('f32', 'bf16'):
      for unimix in cases.UNIMIX:
        worst = {True: 0.0, False: 0.0}
        tally = {True: [0, 0, 0], False: [0, 0, 0]}
        for scale in cases.SCALES:
          rng = np.random.default_rng([groups, classes, int(scale * 10)])
          logits = cases.logits_of(ROWS, groups, classes, scale, rng)
          gout = cases.gout_of(logits.shape, rng)
          if kind == 'bf16':
            logits, gout = cases.bf16_round(logits), cases.bf16_round(gout)
          lead = logits.shape[:-1]
          u = cases.uniforms(SEED, 0, 0, int(np.prod(lead))).reshape(lead)
          p64 = cases.probs64(logits, unimix)
          want = cases.restate(logits, unimix, np.zeros(lead, np.int64), gout)['grad']
          s = cases.group_scale(gout, unimix)
          dtype = torch.float32 if kind == 'f32' else torch.bfloat16
          for fused in (True, False):
            x = torch.from_numpy(logits).cuda().to(dtype).requires_grad_()
            out = outs.OneHot(x, unimix, fused=fused).sample(SEED, 0)
            (out * torch.from_numpy(gout).cuda().to(dtype)).sum().backward()
            ok, near = cases.accepted(p64, u, host(out).argmax(-1), tol)
            tally[fused] = [tally[fused][0] + int((~ok).sum()), tally[fused][1] + int(near.sum()), tally[fused][2] + ok.size]
            worst[fused] = max(worst[fused], cases.grad_ratio(host(x.grad), want, s, kind == 'bf16'))
        cell = lambda f: ' / '.join(str(v) for v in tally[f])
        lines.append(f'  {f"{groups}x{classes}":<12}{kind:<7}{unimix:<8g}{worst[True]:<12.3f}{worst[False]:<15.3f}'
                     f'{cell(True):<30}{cell(False)}')
        for fused in worst:
          worst_all[fused] = max(worst_all[fused], worst[fused])
  lines.append(f'# worst gradient: fused {worst_all[True]:.3f}, composed {worst_all[False]:.3f} of the bar')
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
