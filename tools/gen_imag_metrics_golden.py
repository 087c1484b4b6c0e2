"""Generate tests/golden/imag_metrics.npz by EXECUTING the reference's own
`imag_loss` (dreamerv3/agent.py) and recording the metrics it returns.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_imag_metrics_golden.py

As tools/gen_dreamer_targets_golden.py: `imag_loss` and `lambda_return` are taken
out of the syntax tree whole and unmodified (`oracle.gen_scan_golden.extract`),
the `Normalize` class likewise (`oracle.gen_normalize_golden.reference_class`);
none of these texts is written anywhere, and nothing under oracle/ is edited.
Around them: two action keys whose heads return recorded, non-zero entropies and
carry `minent` / `maxent`, `value.pred` and a different `slowvalue.pred`, zero
`logp`, a `value.loss` of zeros.  Per case of tests/stat_metric_cases.py and per
train step (the three normalisers' state carried) the fixture holds
  metrics   the whole metrics dict, in the order of `cases.METRICS`, float32
  vstats    valnorm.stats() from before the step (agent.py:397), as returned
  rstats    what retnorm(ret, update) returned (agent.py:407)
Only data is written: those arrays, the metric names, the inputs' digests, the
reference's line numbers.
"""
import pathlib
import sys
import types

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import gen_normalize_golden, gen_scan_golden  # noqa: E402
from tests import stat_metric_cases as cases  # noqa: E402


class Recording:
  """The reference's normaliser, with what `__call__` returned."""

  def __init__(self, norm):
    self.norm, self.returned = norm, None

  def stats(self):
    return self.norm.stats()

  def __call__(self, x, update):
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
         'normalize_lines': np.array(norm_lines), 'steps': np.array(cases.STEPS),
         'names': np.array(cases.METRICS)}
  for case, (_, c) in enumerate(cases.IMAG_CASES):
    retnorm, valnorm, advnorm = (_normaliser(Normalize, spec) for spec in (c.retnorm, c.valnorm, c.advnorm))
    rows = {k: [] for k in ('metrics', 'vstats', 'rstats')}
    digests = []
    for step in range(cases.STEPS):
      inp = cases.imag_inputs(case, step)
      digests.append(cases.digest(inp))
      zeros = np.zeros(c.shape, np.float32)
      policy = {}
      for k in cases.KEYS:
        lo, hi = cases.ENTLIMITS[k]
        policy[k] = types.SimpleNamespace(
            logp=lambda a: zeros, entropy=lambda k=k: inp[f'ent_{k}'], minent=lo, maxent=hi)
      value = types.SimpleNamespace(pred=lambda: inp['pred'], loss=lambda target: zeros)
      slowvalue = types.SimpleNamespace(pred=lambda: inp['slow'])
      act = {k: np.zeros(c.shape, np.int32) for k in cases.KEYS}
      before = valnorm.stats()
      losses, outs, metrics = imag_loss(
          act, inp['rew'], inp['con'], policy, value, slowvalue, retnorm, valnorm, advnorm, True,
          contdisc=c.contdisc, slowtar=c.slowtar, **cases.PARAMS)
      assert sorted(metrics) == sorted(cases.METRICS), sorted(metrics)
      values = [metrics[name] for name in cases.METRICS]
      # (numpy's mean of a bool array is float64 where jnp's is float32: ret_rate is
      # count / n rounded once to float32 here, a quotient of two integers <= 16 384)
      assert all(np.asarray(v).shape == () and np.asarray(v).dtype == (np.float64 if n == 'ret_rate' else np.float32)
                 for n, v in zip(cases.METRICS, values)), [(n, np.asarray(v).dtype) for n, v in zip(cases.METRICS, values)]
      assert np.isfinite(values).all(), cases.imag_tag(case)
      rows['metrics'].append(np.array(values, np.float32))
      rows['vstats'].append(np.array(before, np.float64))
      rows['rstats'].append(np.array(retnorm.returned, np.float64))
    name = cases.imag_tag(case)
    out[f'in_{name}'] = np.stack(digests)
    for key, values in rows.items():
      out[f'{key}_{name}'] = np.stack(values)
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'imag_metrics.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 100_000, size
  print(f'imag_metrics: {len(cases.IMAG_CASES)} cases x {cases.STEPS} steps, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
