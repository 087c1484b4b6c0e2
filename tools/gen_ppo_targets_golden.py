"""Generate tests/golden/ppo_targets.npz by EXECUTING the reference's own
`ppo_loss` (ppo/agent.py) against two instances of its own `Normalize`
(embodied/jax/utils.py) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ppo_targets_golden.py

`ppo_loss` is taken out of the syntax tree whole and unmodified
(`oracle.gen_scan_golden.extract`), the class likewise
(`oracle.gen_normalize_golden.reference_class`); neither text is written
anywhere.  Around them: the two normalisers wrapped only to record what they
were fed and what `__call__` returned, `value.pred = pred`, a `value.loss`
that records its argument, zero `logp` and entropy (as
`oracle.gen_scan_golden.run_ppo_loss`).  Per train step the fixture holds
  adv, tar          what the two normalisers were fed
  tarnormed         the padded, clipped target handed to value.loss
  stats             (voffset, vscale, aoffset, ascale) as returned
  advnormed         (adv - aoffset) / ascale in float32, formed here from the
                    recorded values: `ppo_loss` keeps that array to itself, so
                    this ONE line of it (agent.py:210) is restated by this tool.
Only data is written: those arrays, the inputs' digests, the reference's line
numbers.
"""
import pathlib
import sys
import types

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import gen_normalize_golden, gen_scan_golden  # noqa: E402
from tests import ppo_target_cases as cases  # noqa: E402


class Recording:
  """The reference's normaliser, with what it was fed and what it returned."""

  def __init__(self, norm):
    self.norm, self.fed, self.returned = norm, None, None

  def stats(self):
    return self.norm.stats()

  def __call__(self, x, update):
    self.fed = np.array(x, np.float32)
    self.returned = self.norm(x, update)
    return self.returned


def generate():
  ppo_loss, ppo_lines = gen_scan_golden.extract('ppo/agent.py', 'ppo_loss')
  Normalize, norm_lines = gen_normalize_golden.reference_class()
  out = {'ppo_loss_lines': np.array(ppo_lines), 'normalize_lines': np.array(norm_lines),
         'steps': np.array(cases.STEPS)}
  for case, (shape, tarclip) in enumerate(cases.CASES):
    valnorm, advnorm = Recording(Normalize('meanstd')), Recording(Normalize('meanstd'))
    for norm in (valnorm.norm, advnorm.norm):
      for name, value in cases.NORM.items():
        setattr(norm, name, value)            # the module's class-level fields (utils.py:18-22)
    rows = {k: [] for k in ('adv', 'tar', 'tarnormed', 'advnormed', 'stats')}
    digests = []
    for step in range(cases.STEPS):
      inp = cases.inputs(case, step)
      digests.append(cases.digest(inp))
      zeros = np.zeros(shape, np.float32)
      seen = {}
      head = types.SimpleNamespace(logp=lambda a: zeros, entropy=lambda: zeros)
      value = types.SimpleNamespace(
          pred=lambda: inp['pred'], loss=lambda target: seen.setdefault('target', np.array(target)) * 0)
      data = {'reward': inp['rew'], 'is_last': inp['last'], 'is_terminal': inp['term'],
              'action': np.zeros(shape, np.int32), 'logp/action': zeros}
      ppo_loss(data, {'action': head}, value, advnorm, valnorm, {'action': None}, True,
               hor=cases.PARAMS['hor'], lam=cases.PARAMS['lam'], tarclip=tarclip)
      adv, tar = advnorm.fed, valnorm.fed
      aoffset, ascale = (np.float32(v) for v in advnorm.returned)
      assert adv.dtype == tar.dtype == seen['target'].dtype == np.float32
      rows['adv'].append(adv)
      rows['tar'].append(tar)
      rows['tarnormed'].append(seen['target'])
      rows['advnormed'].append(((adv - aoffset) / ascale).astype(np.float32))
      rows['stats'].append(np.array([*valnorm.returned, *advnorm.returned], np.float64))
    name = cases.tag(case)
    out[f'in_{name}'] = np.stack(digests)
    for key, values in rows.items():
      out[f'{key}_{name}'] = np.stack(values)
    if case == cases.CLIP_CASE:
      clipped = np.mean(np.abs(out[f'tarnormed_{name}'][:, :, :-1]) == np.float32(tarclip))
      assert 0.01 <= clipped <= 0.5, f'the clip case clips {clipped:.1%} of its targets'
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'ppo_targets.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  # (21 328 float32 per step over the seven cases, six steps: 512 KB of values that
  # do not compress; the repository's limit for a committed file is 1 MiB)
  assert size < 600_000, size
  print(f'ppo_targets: {len(cases.CASES)} cases x {cases.STEPS} steps, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
