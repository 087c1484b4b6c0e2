"""Worst error of `embodied_amd.optim.LaProp` against float64, per list of
tensors and quantity, as a share of the bars of tests/optim_cases.py.

    python tools/optim_accuracy.py [--out profiles/optim_accuracy.txt]

Rows: the reference's own float32 run (the fixture), the float32 restatement on
the CPU, and, on the GPU, the composed path and the kernels of csrc/optim.hip,
over every case of `cases.CASES` and each of its 4 steps; every element of p, nu
and mu against `cases.reference64`, the metrics against the fixture's float64
run.  Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import optim_cases as cases  # noqa: E402

KEYS = ('p', 'nu', 'mu', 'metrics')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'optim_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'optim_accuracy needs a GPU'
  from tests import test_gpu_optim as gpu
  worst = {}

  def note(who, name, key, value):
    slot = (name, who, key)
    worst[slot] = max(worst.get(slot, 0.0), value)

  with np.load(ROOT / 'tests' / 'golden' / 'optim.npz') as f:
    for case, c in enumerate(cases.CASES):
      specs = cases.LISTS[c.list]
      want = gpu._reference(case)
      fixture = cases.unpack(f[f'out64_{cases.tag(case)}'])
      reference32 = cases.unpack(f[f'out_{cases.tag(case)}'])
      runs = {'float32 restated (CPU)': cases.restate(cases.inputs(case), c.hyper, specs, torch.float32),
              'composed (GPU)': gpu._run(case, False), 'fused (GPU)': gpu._run(case, True)}
      for step in range(cases.STEPS):
        for key in KEYS:
          bar = cases.ratio_nu if key == 'nu' else cases.ratio
          note('float32 reference', c.list, key, bar(reference32[key][step], fixture[key][step]))
          for who, got in runs.items():
            if key == 'metrics':
              note(who, c.list, key, bar(got[step][key], fixture[key][step]))
            else:
              note(who, c.list, key, max([bar(g, w) for g, w in zip(got[step][key], want[step][key])], default=0.0))
  lines = ['# tools/optim_accuracy.py',
           f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
           f'# {len(cases.CASES)} cases x {cases.STEPS} steps; worst |got - float64| as a share of the bar:',
           '#   p, mu, metrics: 1e-5 + 1e-5 |want|;  nu: max(1e-5 |want|, smallest normal float32)',
           f'# {"list":<10}{"path":<26}' + ''.join(f'{key:<12}' for key in KEYS)]
  for name in cases.LISTS:
    for who in ('float32 reference', 'float32 restated (CPU)', 'composed (GPU)', 'fused (GPU)'):
      lines.append(f'  {name:<10}{who:<26}' + ''.join(f'{worst[(name, who, key)]:<12.3g}' for key in KEYS))
  over = sorted(slot for slot, value in worst.items() if value > 1.0)
  lines.append('# over a bar: ' + (', '.join(' / '.join(slot) for slot in over) or 'nothing'))
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
