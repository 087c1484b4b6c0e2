"""Generate tests/golden/conv_stage.npz: the tails of the reference's convolution
stages, 2x2 max pool + Norm + act (dreamerv3/rssm.py:238-241) and Norm + act + 2x2
repeat (dreamerv3/rssm.py:327, 336), over the cases of tests/conv_stage_cases.py.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_conv_stage_golden.py

`Norm.__call__` and `act` are the reference's own text, EXECUTED under the numpy
stand-ins of `tools/gen_rssm_core_golden.py` (`reference_norm`, `run_norm`).  The
pool and the repeat are expressions inside `Encoder.__call__` / `Decoder.__call__`
that cannot be called on their own; each is restated here as the one numpy line
it is, with its line number (numpy's `reshape`, `max` and `repeat` are what
jnp's follow).  Nothing of the reference's text is written anywhere.

Every case runs in float32 and in float64 over the same float32 inputs.  Only
data is written: per case the inputs' digest, the output per precision, and the
reference's line numbers.
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tests import conv_stage_cases as stages  # noqa: E402

POOL_LINES, REPEAT_LINE = (239, 240), 336


def run_stage(run_norm, Norm, act, inp, c, ftype):
  x = inp['x'].astype(ftype)
  if c.stage == 'pool':
    B, H, W, C = x.shape                                           # rssm.py:239
    x = x.reshape((B, H // 2, 2, W // 2, 2, C)).max((2, 4))        # rssm.py:240
  rows = dict(inp, x=x.reshape(-1, x.shape[-1]))
  x = run_norm(Norm, act, rows, c, ftype).reshape(x.shape)    # rssm.py:241 / :327
  if c.stage == 'upsample':
    x = x.repeat(2, -2).repeat(2, -3)                              # rssm.py:336
  assert x.dtype == ftype and x.shape == stages.out_shape(c.stage, inp['x'].shape)
  return x


def generate():
  from tools.gen_rssm_core_golden import reference_norm, run_norm
  out = {'lines_pool': np.array(POOL_LINES), 'lines_repeat': np.array([REPEAT_LINE])}
  for ftype, suffix in ((np.float32, ''), (np.float64, '64')):
    Norm, act, lines = reference_norm(ftype)
    out.update({f'lines_{name}': np.array(span) for name, span in lines.items()})
    for case, c in enumerate(stages.CASES):
      inp = stages.inputs(case)
      out[f'in_{stages.tag(case)}'] = stages.digest(stages.present(inp))
      out[f'out{suffix}_{stages.tag(case)}'] = run_stage(run_norm, Norm, act, inp, c, ftype)
  return out


def main():
  arrays = generate()
  path = ROOT / 'tests' / 'golden' / 'conv_stage.npz'
  np.savez_compressed(path, **arrays)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'conv_stage: {len(stages.CASES)} cases, {len(arrays)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
