"""Worst error of the TwoHot kernels against float64, as a share of the bars of
tests/test_gpu_twohot.py, per case of tests/golden/twohot.npz.

    python tools/twohot_accuracy.py [--out profiles/twohot_accuracy.txt]

  pred   |pred - pred64| / (1e-5 * (1 + sum |p_i b_i|))
  loss   |loss - loss64| / (1e-5 + 1e-5 |loss64|), both targets
  grad   the same bar for the gradient of loss_sum((t1, t2), (1.0, 0.7)) against
         the closed form in float64 (tests/twohot_cases.py)
for the kernels (`fused=True`) and, beside them, the composed torch ops.  The
last lines: (16384, 255), more rows than one sweep of the capped grid, fused
against float64; and the reference's own float32 run for comparison.
Needs a GPU."""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import twohot_cases as cases  # noqa: E402

COEFS = (1.0, 0.7)


def ratio(got, want, scale=None):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert np.array_equal(np.isnan(got), np.isnan(want))
  ok = ~np.isnan(want)
  bar = 1e-5 * (1 + scale) if scale is not None else 1e-5 + 1e-5 * np.abs(want)
  return float(np.max((np.abs(got - want) / bar)[ok], initial=0.0))


def measure(outs, logits, bins, targets, ref, fused):
  x = torch.from_numpy(logits).cuda().requires_grad_()
  head = outs.TwoHot(x, bins, fused=fused)
  pred = head.pred().cpu().numpy()
  each = [head.loss(torch.from_numpy(t).cuda()).detach().cpu().numpy() for t in targets]
  finite = [torch.from_numpy(np.nan_to_num(t, nan=0.0)).cuda() for t in targets]     # the gradient of finite rows
  ref_finite = cases.reference64(logits, bins, [t.cpu().numpy() for t in finite])
  head.loss_sum(finite, COEFS).sum().backward()
  return (ratio(pred, ref['pred'], ref['scale']), max(ratio(l, w) for l, w in zip(each, ref['loss'])),
          ratio(x.grad.cpu().numpy(), cases.grad64(ref_finite, COEFS, np.ones(len(logits)))))


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'twohot_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'twohot_accuracy needs a GPU'
  from embodied_amd import outs
  lines = ['# tools/twohot_accuracy.py', f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
           '# worst error against float64 as a share of the test bars (1.0 = at the bar)',
           f'# {"case":<24}{"fused pred":<12}{"loss":<10}{"grad":<10}{"composed pred":<15}{"loss":<10}{"grad":<10}'
           f'{"reference f32 pred":<20}loss']
  worst = np.zeros(8)
  with np.load(ROOT / 'tests' / 'golden' / 'twohot.npz') as f:
    for case, c in enumerate(cases.CASES):
      name, bins = cases.tag(case), f[f'bins_{c.n}']
      inp = cases.inputs(case, bins)
      targets = [inp[f'target{k}'] for k in range(cases.TARGETS)]
      ref = cases.reference64(inp['logits'], bins, targets)
      ref['pred'], ref['loss'] = f[f'pred64_{name}'], list(f[f'loss64_{name}'])      # the reference's own float64 run
      row = [*measure(outs, inp['logits'], bins, targets, ref, True),
             *measure(outs, inp['logits'], bins, targets, ref, False),
             ratio(f[f'pred_{name}'], ref['pred'], ref['scale']),
             max(ratio(l, w) for l, w in zip(f[f'loss_{name}'], ref['loss']))]
      worst = np.maximum(worst, row)
      lines.append(f'  {name:<24}{row[0]:<12.3g}{row[1]:<10.3g}{row[2]:<10.3g}{row[3]:<15.3g}{row[4]:<10.3g}'
                   f'{row[5]:<10.3g}{row[6]:<20.3g}{row[7]:.3g}')
      print(lines[-1], flush=True)
  lines.append(f'  {"worst":<24}{worst[0]:<12.3g}{worst[1]:<10.3g}{worst[2]:<10.3g}{worst[3]:<15.3g}{worst[4]:<10.3g}'
               f'{worst[5]:<10.3g}{worst[6]:<20.3g}{worst[7]:.3g}')
  rng = np.random.default_rng(16384)
  for n in (255, 256):
    bins = outs.symexp_twohot_bins(n)
    logits = (3 * rng.standard_normal((16384, n))).astype(np.float32)
    targets = [cases.targets_of(16384, bins, rng) for _ in range(2)]
    ref = cases.reference64(logits, bins, targets)
    row = measure(outs, logits, bins, targets, ref, True)
    lines.append(f'# (16384, {n}), two sweeps of the grid, fused: pred {row[0]:.3g}, loss {row[1]:.3g}, grad {row[2]:.3g}')
  print('\n'.join(lines[-3:]), flush=True)
  assert worst[:6].max() <= 1.0 and max(row) <= 1.0
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
