"""Worst error of `embodied_amd.optim.Adam` against float64, per list of tensors
and quantity, as a share of the bars of tests/adam_cases.py.

    python tools/adam_accuracy.py [--out profiles/adam_accuracy.txt]

Rows: the float32 restatement on the CPU and, on the GPU, the composed path and
the kernels of csrc/optim.hip, over every case of `cases.CASES` and each of its
4 steps; every element of p, nu and mu and the four metrics against
`cases.reference64`, the float64 run that is the definition.  Below them the same
three rows for the lists of tests/adam_sweep_cases.py, which take the kernels
past the first iteration of their loops, over each of their cases and steps
against `sweep.reference`.  Needs a GPU: there is no CPU fallback and no figure
without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from tests import adam_cases as cases  # noqa: E402
from tests import adam_sweep_cases as sweep  # noqa: E402

KEYS = ('p', 'nu', 'mu', 'metrics')
PATHS = ('float32 restated (CPU)', 'composed (GPU)', 'fused (GPU)')


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'adam_accuracy.txt'))
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'adam_accuracy needs a GPU'
  from tests import test_gpu_adam as gpu
  worst = {}
  for case, c in enumerate(cases.CASES):
    want = cases.reference64(case)
    runs = {'float32 restated (CPU)': cases.restate(cases.inputs(case), c.hyper, cases.LISTS[c.list], torch.float32),
            'composed (GPU)': gpu._run(case, False), 'fused (GPU)': gpu._run(case, True)}
    for who, got in runs.items():
      for key, value in cases.worst_ratios(got, want).items():
        slot = (c.list, who, key)
        worst[slot] = max(worst.get(slot, 0.0), value)
  deeper = {}
  for case in sweep.CASES:
    name, i = case
    h = sweep.HYPERS[name][i]
    want = sweep.reference(case)
    runs = {'float32 restated (CPU)': cases.restate(sweep.inputs(name, h.bf16), h, sweep.LISTS[name], torch.float32),
            'composed (GPU)': gpu._run_from(gpu._make_sweep(case, False), sweep.STEPS[name]),
            'fused (GPU)': gpu._run_from(gpu._make_sweep(case, True), sweep.STEPS[name])}
    for who, got in runs.items():
      for key, value in sweep.worst_ratios(got, want).items():
        slot = (name, who, key)
        deeper[slot] = max(deeper.get(slot, 0.0), value)
  lines = ['# tools/adam_accuracy.py',
           f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}',
           f'# {len(cases.CASES)} cases x {cases.STEPS} steps; worst |got - float64| as a share of the bar, every element:',
           '#   p, metrics: 1e-5 + 1e-5 |want|;  nu: max(1e-5 |want|, smallest normal float32);',
           '#   mu: 1e-5 (|want| + A), A = the same moving average over |g1| in float64',
           f'# {"list":<10}{"path":<26}' + ''.join(f'{key:<12}' for key in KEYS)]
  for name in cases.LISTS:
    for who in PATHS:
      lines.append(f'  {name:<10}{who:<26}' + ''.join(f'{worst[(name, who, key)]:<12.3g}' for key in KEYS))
  for who in PATHS:
    lines.append(f'  {"all":<10}{who:<26}' +
                 ''.join(f'{max(worst[(name, who, key)] for name in cases.LISTS):<12.3g}' for key in KEYS))
  k = sweep.K
  lines += ["# ---- past the first iteration of the kernels' loops (lists of tests/adam_sweep_cases.py; the same bars):",
            f'#   many: {len(sweep.LISTS["many"])} tensors of 1 .. 5 elements, {sweep.chunks(sweep.LISTS["many"])} chunks (kMaxBlocks = '
            f'{k["kMaxBlocks"]}, kMetricThreads = {k["kMetricThreads"]}, kThreads = {k["kThreads"]}),',
            f'#     {len(sweep.HYPERS["many"])} cases x {sweep.STEPS["many"]} steps, the bfloat16 cases with bfloat16 gradients in every third tensor only;',
            f'#   deep: two tensors of {k["kThreads"] + 2} chunks and one of 3 elements, {sweep.chunks(sweep.LISTS["deep"])} chunks, '
            f'{len(sweep.HYPERS["deep"])} cases x {sweep.STEPS["deep"]} steps']
  for name in sweep.LISTS:
    for who in PATHS:
      lines.append(f'  {name:<10}{who:<26}' + ''.join(f'{deeper[(name, who, key)]:<12.3g}' for key in KEYS))
  over = sorted(slot for slot, value in list(worst.items()) + list(deeper.items()) if value > 1.0)
  lines.append('# over a bar: ' + (', '.join(' / '.join(slot) for slot in over) or 'nothing'))
  print('\n'.join(lines), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
