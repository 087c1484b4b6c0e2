"""Worst ratio of the reconstruction heads to each bar of
tests/test_gpu_recon_loss.py, over every case of `tests/recon_loss_cases.GRID`.

    python tools/recon_loss_accuracy.py [--out profiles/recon_loss_accuracy.txt]

Per op, dtype of x and path: the worst |loss - want64| / (1e-5 sum |term|) and the
worst gradient element against 1e-5 s (1 + |want| / s) (+ 2^-8 |want| for a
bfloat16 gradient), s = max |want| over the row.  The fused path is held to the
float64 restatement that rounds nothing, the composed path to the one built
around the device's own sigmoid in the compute dtype and the rounding of its
backward's upstream gradient, where the reference rounds.  The first
block is the float32 definition in numpy, which needs no GPU; the rest does.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import recon_loss_cases as cases  # noqa: E402


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'recon_loss_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'recon_loss_accuracy needs a GPU'
  from embodied_amd import outs

  def head(op, x, target, fused):
    if op == 'mse':
      return outs.MSE(x, fused=fused).loss(target, 1)
    if op == 'symlog':
      return outs.MSE(x, 'symlog', fused=fused).loss(target, 1)
    if op == 'sigmoid':
      return outs.ImageMSE(x, fused=fused).loss(target, 1)
    return outs.Binary(x, fused=fused).loss(target, 1)

  worst = {}

  def note(key, c, loss, grad):
    w = worst.setdefault(key, [0.0, None, 0.0, None])
    if loss > w[0]:
      w[0], w[1] = loss, c
    if grad > w[2]:
      w[2], w[3] = grad, c

  for c in cases.GRID:
    for kind in cases.KINDS:
      d = cases.data(c.op, c.units, c.rows, c.scale, kind)
      exact = cases.restate(c.op, d['x'], d['target'], d['gout'])
      dtype = torch.float32 if kind == 'f32' else torch.bfloat16
      y = torch.sigmoid(torch.from_numpy(d['x']).cuda().to(dtype)).float().cpu().numpy()
      rounded = cases.restate_rounded(c.op, d['x'], d['target'], d['gout'], kind, y=y)
      got = cases.define32(c.op, d['x'], d['target'], d['gout'])
      note((c.op, kind, 'definition'), c, cases.loss_ratio(got['loss'], exact),
           cases.grad_ratio(got['grad'], exact['grad'], cases.row_scale(exact['grad'])))
      for fused, want in ((True, exact), (False, rounded)):
        x = torch.from_numpy(d['x']).cuda().to(torch.float32 if kind == 'f32' else torch.bfloat16).requires_grad_()
        loss = head(c.op, x, torch.from_numpy(d['target']).cuda(), fused)
        (loss * torch.from_numpy(d['gout']).cuda()).sum().backward()
        note((c.op, kind, 'fused' if fused else 'composed'), c, cases.loss_ratio(loss.detach().cpu().numpy(), want),
             cases.grad_ratio(x.grad.float().cpu().numpy(), want['grad'], cases.row_scale(want['grad']), kind == 'bf16'))
  lines = [
      '# tools/recon_loss_accuracy.py',
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
      f'# {len(cases.GRID)} cases x {len(cases.KINDS)} dtypes: ops {cases.OPS}, widths {cases.WIDTHS}, rows {cases.ROWS}, '
      f'scales {cases.SCALES}',
      '# worst ratio to the bar (1.0 = on the bar) and the case it was met at',
      f'# {"op":<10}{"x":<6}{"path":<12}{"loss":<10}{"at (units, rows, scale)":<28}{"gradient":<10}at (units, rows, scale)',
  ]
  at = lambda c: '-' if c is None else f'({c.units}, {c.rows}, {c.scale:g})'
  for (op, kind, path), (loss, loss_at, grad, grad_at) in sorted(worst.items()):
    lines.append(f'  {op:<10}{kind:<6}{path:<12}{loss:<10.3g}{at(loss_at):<28}{grad:<10.3g}{at(grad_at)}')
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
