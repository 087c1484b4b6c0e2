"""Generate tests/golden/dreamer_targets.npz by EXECUTING the reference's own
`imag_loss` and `lambda_return` (dreamerv3/agent.py) against three instances of
its own `Normalize` (embodied/jax/utils.py) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_dreamer_targets_golden.py

`imag_loss` is taken out of the syntax tree whole and unmodified
(`oracle.gen_scan_golden.extract`), `lambda_return` the same way and put into
its globals, the class likewise (`oracle.gen_normalize_golden.reference_class`);
none of these texts is written anywhere.  Around them: the three normalisers
wrapped only to record what they were fed and what `__call__` returned,
`value.pred = pred`, a `slowvalue.pred` that returns a DIFFERENT array (a wrong
choice under `slowtar` shows), a `value.loss` that records its argument, zero
`logp` and entropy.  Per train step the fixture holds
  ret               outs['ret']
  adv               what advnorm was fed
  tarpadded         what value.loss received first
  stats             (roffset, rscale, aoffset, ascale, voffset, vscale) as returned
  advnormed         (adv - aoffset) / ascale in float32, formed here from the
                    recorded values, as tools/gen_ppo_targets_golden.py does
  weight            cumprod(disc * con, 1) / disc: `imag_loss` keeps that array to
                    itself (only its mean leaves, as a metric), so this ONE line
                    of it (agent.py:402) is restated by this tool; the metric
                    `weight` of the executed function is asserted equal to the
                    restated array's mean.
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
from tests import dreamer_target_cases as cases  # noqa: E402


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


def _normaliser(Normalize, spec):
  impl, fields = spec
  norm = Normalize(impl)
  for name, value in {**cases.NORM, **fields}.items():
    setattr(norm, name, value)              # the module's class-level fields (utils.py:18-22)
  return Recording(norm)


def generate():
  imag_loss, imag_lines = gen_scan_golden.extract('dreamerv3/agent.py', 'imag_loss')
  lambda_return, lambda_lines = gen_scan_golden.extract('dreamerv3/agent.py', 'lambda_return')
  imag_loss.__globals__['lambda_return'] = lambda_return
  Normalize, norm_lines = gen_normalize_golden.reference_class()
  out = {'imag_loss_lines': np.array(imag_lines), 'lambda_return_lines': np.array(lambda_lines),
         'normalize_lines': np.array(norm_lines), 'steps': np.array(cases.STEPS)}
  for case, c in enumerate(cases.CASES):
    retnorm, valnorm, advnorm = (_normaliser(Normalize, spec) for spec in (c.retnorm, c.valnorm, c.advnorm))
    rows = {k: [] for k in ('ret', 'weight', 'adv', 'advnormed', 'tarpadded', 'stats')}
    digests = []
    for step in range(cases.STEPS):
      inp = cases.inputs(case, step)
      digests.append(cases.digest(inp))
      zeros = np.zeros(c.shape, np.float32)
      seen = {}
      head = types.SimpleNamespace(logp=lambda a: zeros, entropy=lambda: zeros)
      value = types.SimpleNamespace(
          pred=lambda: inp['pred'], loss=lambda target: seen.setdefault('target', np.array(target)) * 0)
      slowvalue = types.SimpleNamespace(pred=lambda: inp['slow'])
      act = {'action': np.zeros(c.shape, np.int32)}
      losses, outs, metrics = imag_loss(
          act, inp['rew'], inp['con'], {'action': head}, value, slowvalue, retnorm, valnorm, advnorm, True,
          contdisc=c.contdisc, slowtar=c.slowtar, **cases.PARAMS)
      ret, adv, target = np.asarray(outs['ret']), advnorm.fed, seen['target']
      aoffset, ascale = (np.float32(v) for v in advnorm.returned)
      disc = 1 if c.contdisc else 1 - 1 / cases.PARAMS['horizon']
      weight = np.cumprod(disc * inp['con'], 1) / disc           # agent.py:402, restated (see above)
      assert ret.dtype == adv.dtype == target.dtype == weight.dtype == np.float32
      assert np.array_equal(np.float32(metrics['weight']), weight.mean()), 'the restated line is not agent.py:402'
      assert np.array_equal(retnorm.fed, ret) and np.array_equal(valnorm.fed, ret)
      assert np.isfinite(ret).all(), cases.tag(case)
      rows['ret'].append(ret)
      rows['weight'].append(weight)
      rows['adv'].append(adv)
      rows['advnormed'].append(((adv - aoffset) / ascale).astype(np.float32))
      rows['tarpadded'].append(target)
      rows['stats'].append(np.array([*retnorm.returned, *advnorm.returned, *valnorm.returned], np.float64))
    name = cases.tag(case)
    out[f'in_{name}'] = np.stack(digests)
    for key, values in rows.items():
      out[f'{key}_{name}'] = np.stack(values)
    if c.tie:
      # both order statistics of both percentiles sit inside runs of equal values
      for ret in out[f'ret_{name}']:
        ordered = np.sort(ret.reshape(-1))
        for q in (c.retnorm[1].get('perclo', 5.0), c.retnorm[1].get('perchi', 95.0)):
          k = int(np.floor(q / 100 * (ordered.size - 1)))
          assert ordered[k] == ordered[k + 1] and (ordered == ordered[k]).sum() >= c.shape[0], (name, q)
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'dreamer_targets.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  # (about 35 000 float32 per step over the seven cases, four steps: values that
  # do not compress; the repository's limit for a committed file is 1 MiB)
  assert size < 900_000, size
  print(f'dreamer_targets: {len(cases.CASES)} cases x {cases.STEPS} steps, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
