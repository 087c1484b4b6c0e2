"""Worst ratios of the Normal policy-head kernels (csrc/normal_policy.hip) and of
the composed path against the bars of tests/normal_policy_cases.py, over every
case of tests/golden/normal_policy.npz, float32 and bfloat16-rounded inputs.

    python tools/normal_policy_accuracy.py [--out profiles/normal_policy_accuracy.txt]

  forward   |got - want| / (1e-5 (1 + S)) for logpi and ent, times |weight| (|adv| +
            actent) for the loss; S = sum_a (z^2 / 2 + |log std_a| + 1) from the
            float64 run; `want` is the reference's own float64 run of imag_loss
            (float32 inputs) or `cases.reference64` (rounded inputs).
  gradient  |got - want| / (1e-5 (s + |want|)), s = |gout weight| (|adv| + actent),
            plus 2^-8 |want| for a bfloat16 gradient; `want` is `reference64`'s autograd.
  draw      |eps - want| / (1e-5 (1 + |want|)) over 2^16 draws, `want` the float64
            Box-Muller of the same Philox words.
A ratio of 1 is the bar.  Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import normal_policy_cases as cases  # noqa: E402


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'normal_policy_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'normal_policy_accuracy needs a GPU'
  from embodied_amd import outs
  device = lambda x, bf16=False: (lambda t: t.to(torch.bfloat16) if bf16 else t)(torch.from_numpy(x).cuda())
  host = lambda t: t.detach().float().cpu().numpy()
  worst = {}
  with np.load(ROOT / 'tests' / 'golden' / 'normal_policy.npz') as f:
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      adv, weight, fixture = f[f'adv_{name}'], f[f'weight_{name}'], f[f'out64_{name}']
      gout = np.random.default_rng(case).standard_normal(adv.shape).astype(np.float32)
      dims = 1 if c.actions else 0
      for rounded in (False, True):
        inp = cases.inputs(case)
        if rounded:
          inp.update(mean_raw=cases.bf16_round(inp['mean_raw']), std_raw=cases.bf16_round(inp['std_raw']))
        want = cases.reference64(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, cases.ACTENT, c.kind, dims, 1,
                                 gout)
        if not rounded:
          want.update(zip(cases.FIELDS, fixture))
        s = cases.row_scale(gout, weight[:, :-1], adv, cases.ACTENT)
        for fused in (True, False):
          if fused and c.actions > outs.NORMAL_MAX_ACTIONS:
            continue
          m, sd = (device(inp[k], rounded).requires_grad_() for k in ('mean_raw', 'std_raw'))
          out = outs.normal_policy_loss(m, sd, device(inp['act']), device(adv), device(weight), cases.ACTENT, c.kind,
                                        cases.MINSTD, cases.MAXSTD, dims, True, fused)
          (out['loss'] * device(gout)).sum().backward()
          got = {k: host(v) for k, v in out.items()}
          forward = cases.forward_ratios(got, want, adv, weight[:, :-1], cases.ACTENT)
          gradient = max(cases.grad_ratio(host(x.grad)[:, :-1], want[k][:, :-1], s, rounded)
                         for k, x in (('grad_mean', m), ('grad_std', sd)))
          key = ('fused' if fused else 'composed', c.kind, c.scale, 'bf16' if rounded else 'f32')
          old = worst.get(key, (0.0, 0.0))
          worst[key] = (max(old[0], forward), max(old[1], gradient))
  eps = host(outs.philox_normal(2024, 1, 0, 1 << 16)).astype(np.float64)
  want = cases.box_muller64(2024, 1, 0, 1 << 16)
  draw = float(np.max(np.abs(eps - want) / (1e-5 * (1 + np.abs(want)))))
  lines = [
      '# tools/normal_policy_accuracy.py',
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
      f'# worst ratios against the bars over the {len(cases.CASES)} cases of tests/golden/normal_policy.npz (1 = the bar)',
      f'# {"path":<10}{"kind":<9}{"scale":<8}{"inputs":<8}{"forward":<12}gradient',
  ]
  for key in sorted(worst):
    lines.append(f'  {key[0]:<10}{key[1]:<9}{key[2]:<8g}{key[3]:<8}{worst[key][0]:<12.3g}{worst[key][1]:.3g}')
  lines.append(f'# draw: {draw:.3g} of its bar over 2^16 draws; mean {eps.mean():+.4f}, variance {eps.var():.4f}')
  lines.append(f'# worst forward {max(v[0] for v in worst.values()):.3g}, worst gradient '
               f'{max(v[1] for v in worst.values()):.3g}')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text(text)


if __name__ == '__main__':
  main()
