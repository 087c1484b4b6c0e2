"""Worst share of the bars of tests/stat_metric_cases.py that the kernels of
csrc/stat_rows.hip, and the composed paths beside them, use on the GPU.

    python tools/stat_metrics_accuracy.py [--out profiles/stat_metrics_accuracy.txt]

  stat_rows     |got - float64| / (1e-5 mean |x'|) for mean, std and mean |x'| over
                every element count, affine mode, matrix view and odd offset of
                the case table; min, max and rate are compared bit for bit.
  imag_metrics  the same share per metric, fused and composed, over every case of
                tests/golden/imag_metrics.npz and its train steps (state carried),
                `want` the float64 restatement over the arrays `dreamer_targets`
                left on the device.
  total_loss    |got - float64| / (1e-5 sum |scale_k| mean |v_k|), K = 1, 3, 10,
                and the gradients' worst relative error in units of 2^-24.
A share of 1 is the bar.  Needs a GPU.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stat_metric_cases as cases  # noqa: E402

MODES = {cases.NONE: None, cases.MUL_ADD: 'mul_add', cases.SUB_DIV: 'sub_div'}


def _cuda(array, offset=0):
  array = np.ascontiguousarray(array, np.float32)
  buffer = torch.zeros(array.size + offset + 4, dtype=torch.float32, device='cuda')
  view = buffer[offset:offset + array.size]
  view.copy_(torch.from_numpy(array.reshape(-1)))
  return view.view(array.shape)


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'stat_metrics_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'stat_metrics_accuracy needs a GPU'
  from embodied_amd import DeviceNormalize, ops, outs, scans
  bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
  pairs = {m: torch.tensor(p, dtype=torch.float32, device='cuda') for m, p in cases.AFFINE.items()}
  entry = lambda x, m: x if m == cases.NONE else (x, MODES[m], pairs[m])
  # ---- stat_rows
  groups = {}
  for mode in cases.AFFINE:
    for n in cases.COUNTS:
      x = cases.edge_data(n, mode)[0]
      groups.setdefault(f'aligned, mode {MODES[mode] or "none"}', []).append(
          (entry(_cuda(x), mode), cases.affine32(x, mode, *cases.AFFINE[mode])))
  for rows, cols, width in cases.VIEWS:
    full = cases.stat_data('view', rows * width).reshape(rows, width)
    groups.setdefault('matrix views', []).append((_cuda(full)[:, :cols], full[:, :cols]))
  for offset in cases.OFFSETS:
    x = cases.stat_data('offset', cases.OFFSET_COUNT + offset)[offset:]
    groups.setdefault('odd offsets', []).append((_cuda(x, offset), x))
  lines = [f'# tools/stat_metrics_accuracy.py; {torch.cuda.get_device_name(0)} '
           f'({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
           '# worst share of the bar (1 = the bar); exact: entries whose min, max and rate have the restatement\'s bits',
           '# stat_rows: bar = 1e-5 mean |x\'|']
  for name, items in groups.items():
    got = ops.stat_rows([e for e, _ in items]).cpu().numpy()
    worst, exact = dict.fromkeys(cases.COLUMNS[:3], 0.0), 0
    for row, (_, xp) in zip(got, items):
      want, bar = cases.stats64(xp), cases.moment_bar(xp)
      for index, column in enumerate(cases.COLUMNS[:3]):
        worst[column] = max(worst[column], abs(float(row[index]) - want[index]) / bar)
      exact += int(np.array_equal(bits(row[3:]), bits(np.array(cases.exact32(xp)))))
    lines.append(f'  {name:<28}' + '  '.join(f'{k} {v:.5f}' for k, v in worst.items()) + f'  exact {exact}/{len(items)}')
  # ---- imag_metrics
  lines.append('# imag_metrics: bar = 1e-5 mean |x\'| of the metric\'s array; ret_min, ret_max, ret_rate are counted as exact or not')
  for path, fused in (('fused', True), ('composed', False)):
    worst, exact, total = {}, 0, 0
    for case, (_, c) in enumerate(cases.IMAG_CASES):
      retnorm, valnorm, advnorm = (DeviceNormalize(impl, **{**cases.NORM, **fields})
                                   for impl, fields in (c.retnorm, c.valnorm, c.advnorm))
      for step in range(cases.STEPS):
        inp = cases.imag_inputs(case, step)
        dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
        vstats = None if valnorm.impl == 'none' else tuple(v.clone() for v in valnorm.latest())
        targets = scans.dreamer_targets(dev['rew'], dev['con'], torch.from_numpy(cases.target_pred(case, inp)).cuda(),
                                        retnorm, valnorm, advnorm, contdisc=c.contdisc, update=True, **cases.PARAMS)
        got = scans.imag_metrics(targets, dev['rew'], dev['con'], dev['pred'], dev['slow'], retnorm, vstats,
                                 {k: dev[f'ent_{k}'] for k in cases.KEYS}, cases.ENTLIMITS, fused=fused)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        want, bars = cases.imag_metrics64(
            inp['rew'], inp['con'], inp['pred'], inp['slow'], targets.ret.cpu().numpy(), targets.adv.cpu().numpy(),
            targets.weight.cpu().numpy(), targets.tar_padded.cpu().numpy(), [float(v) for v in retnorm._stats],
            (0.0, 1.0) if vstats is None else [float(v) for v in vstats],
            {k: inp[f'ent_{k}'] for k in cases.KEYS}, cases.ENTLIMITS)
        for metric in cases.METRICS:
          if bars[metric] == 0.0:
            total += 1
            exact += int(np.array_equal(bits(got[metric]), bits(want[metric])))
          else:
            worst[metric] = max(worst.get(metric, 0.0), abs(float(got[metric]) - want[metric]) / bars[metric])
    lines.append(f'  {path:<10}' + '  '.join(f'{k} {v:.5f}' for k, v in worst.items()) + f'  exact {exact}/{total}')
  # ---- total_loss
  lines.append('# total_loss: bar = 1e-5 sum |scale_k| mean |v_k|; gradient: worst |got - float64| / |float64| in units of 2^-24')
  for path, fused in (('fused', True), ('composed', False)):
    cells = []
    for count in cases.LOSS_COUNTS:
      losses, scales = cases.loss_inputs(count)
      tensors = {k: torch.from_numpy(v).cuda().requires_grad_() for k, v in losses.items()}
      loss, _ = outs.total_loss(tensors, scales, fused=fused)
      loss.backward()
      total, _, bar, grads = cases.total_loss64(losses, scales)
      ulps = max(float(np.max(np.abs(v.grad.cpu().numpy().astype(np.float64) - grads[k]) / abs(grads[k]))) / 2.0 ** -24
                 for k, v in tensors.items())
      cells.append(f'K={count} total {abs(float(loss.detach()) - total) / bar:.5f} gradient {ulps:.2f}')
    lines.append(f'  {path:<10}' + '  '.join(cells))
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
