"""The symlog bar of `nets.DictConcat` and where the paths stand against it.

    python tools/dict_concat_accuracy.py [--out profiles/dict_concat_accuracy.txt]

Without a GPU: the worst error of the reference's own float32 run against its
float64 run over the fixture's symlog cases (tests/golden/dict_concat.npz), in
float32 ulps of the float64 value, and the bar that follows from it (twice that,
not less than one ulp); tests/dict_concat_cases.py must hold both figures.
With a GPU it adds the kernel and the composed path, float32 and bfloat16 out,
against the same float64 values.  Identity, one-hot, masks and clamp are exact
and are not listed: the tests hold them bit for bit.
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import dict_concat_cases as cases  # noqa: E402


def reference_ulps(golden):
  worst = {}
  for case, c in enumerate(cases.CASES):
    if c.squish == 'symlog':
      name = cases.tag(case)
      worst[name] = float(cases.ulps(golden[f'out_{name}'], golden[f'out64_{name}']).max())
  return worst


def device_ulps(golden):
  import torch
  from embodied_amd import nets
  lines = []
  for case, c in enumerate(cases.CASES):
    if c.squish != 'symlog':
      continue
    name, inp = cases.tag(case), cases.inputs(case)
    xs = {k.name: torch.from_numpy(inp[k.name]).cuda() for k in c.keys}
    reset = torch.from_numpy(inp['reset']).cuda() if 'reset' in inp else None
    want = golden[f'out64_{name}']
    for dtype, label in ((torch.float32, 'float32'), (torch.bfloat16, 'bfloat16')):
      concat = nets.DictConcat(cases.spaces_of(c.keys), squish=c.squish, dtype=dtype)
      for fused in (True, False):
        got = concat(xs, reset=reset, unit=c.unit, fused=fused).float().cpu().numpy()
        if dtype == torch.float32:
          figure = f'{cases.ulps(got, want).max():.4f} float32 ulp (bar {cases.SYMLOG_BAR_ULP:.4f})'
        else:
          same = (np.isnan(got) & np.isnan(want)) | (got == want)
          share = np.where(same, 0.0, np.abs(got - want) / cases.bf16_bar(want))
          figure = f'{share.max():.4f} of the bfloat16 bar'
        lines.append(f'{name:16s} {label:8s} {"fused" if fused else "composed":8s} worst {figure}')
  return lines


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'dict_concat_accuracy.txt'))
  args = parser.parse_args()
  with np.load(ROOT / 'tests' / 'golden' / 'dict_concat.npz') as f:
    golden = {k: f[k] for k in f.files}
  worst = reference_ulps(golden)
  measured = max(worst.values())
  bar = max(2 * measured, 1.0)
  lines = ['# tools/dict_concat_accuracy.py',
           '# symlog, against the reference\'s float64 run, in float32 ulps of the float64 value']
  lines += [f'{name:16s} reference float32 run, worst {value:.4f} ulp' for name, value in worst.items()]
  lines += [f'measured worst {measured:.4f} ulp; the bar: max(2 x measured, 1) = {bar:.4f} ulp',
            f'tests/dict_concat_cases.py holds {cases.SYMLOG_REFERENCE_ULP:.4f} and {cases.SYMLOG_BAR_ULP:.4f}',
            'bfloat16 out: half a bfloat16 ulp of the float64 value plus that bar']
  assert abs(cases.SYMLOG_REFERENCE_ULP - measured) < 5e-5, (cases.SYMLOG_REFERENCE_ULP, measured)
  try:
    import torch
    gpu = torch.cuda.is_available()
  except ImportError:
    gpu = False
  if gpu:
    import torch
    lines.append(f'# {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    lines += device_ulps(golden)
  else:
    lines.append('# no GPU: the kernel and the composed path were not measured')
  print('\n'.join(lines))
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
