"""Generate tests/golden/normal_policy.npz by EXECUTING the reference's own
`imag_loss` (dreamerv3/agent.py) with its own output classes `Output`, `Agg` and
`Normal` (embodied/jax/outs.py) as the policy, built by its own
`Head.bounded_normal` / `Head.normal_logstd` (embodied/jax/heads.py), under numpy
stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_normal_policy_golden.py

The method is `tools/gen_policy_loss_golden.py`'s: the three classes are taken
out of the syntax tree together and compiled, the two head methods and
`imag_loss` / `lambda_return` each on their own (`oracle.gen_scan_golden.extract`).
None of these texts is written anywhere.  A head method is called on a stand-in
`self` whose `sub(name, ...)` hands back the case's raw `mean` / `stddev` arrays
in place of the two linear layers; what it returns is wrapped as `Head.__call__`
does (heads.py:90-91).  `imag_loss` is executed whole, with the stand-ins of
`tools/gen_policy_loss_golden.py` for the values and the normalisers.

Stand-ins defined here, for one float type at a time:
  jax.nn.sigmoid               1 / (1 + exp(-x))
  jax.scipy.stats.norm.logpdf  -(log(2 pi scale^2) + ((x - loc) / scale)^2) / 2 as
                               jax writes it (log_normalizer and quadratic)
  jnp                          numpy, with a `sum` that takes `Agg`'s list of axes
  f32                          the float type of the run
Every case runs in float32 (what the reference computes) and in float64 over the
same float32 inputs (what the parity tests hold the kernels against).

Only data is written: per case the inputs' digest, one (3, N, T - 1) array per
precision -- `cases.FIELDS`: logpi, ent and losses['policy'] -- the recorded adv
(N, T - 1) and weight (N, T) per precision, and the reference's line numbers.
"""
import ast
import pathlib
import sys
import types

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import gen_scan_golden, refload  # noqa: E402
from oracle.shims import jaxlike  # noqa: E402
from tests import normal_policy_cases as cases  # noqa: E402

CLASSES = ('Output', 'Agg', 'Normal')
HEADS = {'bounded': 'bounded_normal', 'logstd': 'normal_logstd'}


class _Jnp:
  """numpy; `sum` accepts the list of axes that `Agg` passes (numpy.sum refuses one)."""

  def __getattr__(self, name):
    return getattr(np, name)

  @staticmethod
  def sum(x, axis=None):
    return np.sum(x, tuple(axis) if isinstance(axis, list) else axis)


jnp = _Jnp()


def _jax(ftype):
  def sigmoid(x):
    with np.errstate(over='ignore'):
      return (1 / (1 + np.exp(-x))).astype(ftype)

  def logpdf(x, loc=0, scale=1):
    scale_sqrd = np.square(scale)
    log_normalizer = np.log(ftype(2 * np.pi) * scale_sqrd)
    quadratic = np.square(x - loc) / scale_sqrd
    return -(log_normalizer + quadratic) / 2

  return types.SimpleNamespace(
      nn=types.SimpleNamespace(sigmoid=sigmoid),
      scipy=types.SimpleNamespace(stats=types.SimpleNamespace(norm=types.SimpleNamespace(logpdf=logpdf))),
      lax=types.SimpleNamespace(stop_gradient=lambda x: x))


def reference_classes(ftype):
  """The reference's three output classes, compiled with `f32` = ftype."""
  path = refload.REFERENCE / 'embodied' / 'jax' / 'outs.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
  assert [n.name for n in nodes] == list(CLASSES)
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(jax=_jax(ftype), jnp=jnp, f32=ftype, i32=np.int32)
  exec(compile(ast.Module(body=nodes, type_ignores=[]), str(path), 'exec'), namespace)
  lines = {n.name: (n.lineno, n.end_lineno) for n in nodes}
  return types.SimpleNamespace(**{name: namespace[name] for name in CLASSES}), lines


class Recording:
  """A normaliser stand-in: offset 0, scale 1, remembers what it was fed."""

  def __init__(self):
    self.fed = None

  def stats(self):
    return 0.0, 1.0

  def __call__(self, x, update):
    self.fed = np.array(x)
    return 0.0, 1.0


def runner(ftype):
  """run(inp, c) -> (logpi, ent, loss, adv, weight) of `imag_loss`, executed whole in `ftype`."""
  outs, lines = reference_classes(ftype)
  heads = {}
  for kind, name in HEADS.items():
    heads[kind], lines[name] = gen_scan_golden.extract('embodied/jax/heads.py', name, 'Head')
    heads[kind].__globals__.update(jax=_jax(ftype), jnp=jnp, outs=outs, nets=types.SimpleNamespace(Linear=None))
  imag_loss, lines['imag_loss'] = gen_scan_golden.extract('dreamerv3/agent.py', 'imag_loss')
  lambda_return, lines['lambda_return'] = gen_scan_golden.extract('dreamerv3/agent.py', 'lambda_return')
  imag_loss.__globals__.update(lambda_return=lambda_return, jnp=jnp)

  def run(inp, c):
    dims = 1 if c.actions else 0
    raw = {'mean': inp['mean_raw'].astype(ftype), 'stddev': inp['std_raw'].astype(ftype)}
    space = types.SimpleNamespace(discrete=False, shape=(c.actions,) if dims else ())
    head = types.SimpleNamespace(space=space, kw={}, minstd=cases.MINSTD, maxstd=cases.MAXSTD,
                                 sub=lambda name, ctor, shape, **kw: (lambda x: raw[name]))
    output = heads[c.kind](head, None)
    assert type(output) is outs.Normal and output.mean.dtype == ftype and output.stddev.dtype == ftype
    policy = outs.Agg(output, len(space.shape), jnp.sum)           # heads.py:90-91
    policy.axes = tuple(policy.axes)
    rew, con, pred = (inp[k].astype(ftype) for k in ('rew', 'con', 'pred'))
    value = types.SimpleNamespace(pred=lambda: pred, loss=lambda target: np.zeros_like(pred))
    retnorm, valnorm, advnorm = Recording(), Recording(), Recording()
    act = inp['act'].astype(ftype)      # Normal.logp widens with f32(event): the run's float type
    losses, _, metrics = imag_loss(
        {'action': act}, rew, con, {'action': policy}, value, value, retnorm, valnorm, advnorm, True, **cases.PARAMS)
    weight = np.cumprod(con, 1)                    # agent.py:402 with contdisc (disc = 1), restated
    assert np.array_equal(metrics['weight'], weight.mean()), 'the restated line is not agent.py:402'
    logpi, ent = policy.logp(act)[:, :-1], policy.entropy()[:, :-1]
    assert np.array_equal(metrics['ent/action'], ent.mean())
    loss, adv = losses['policy'], advnorm.fed
    for array in (logpi, ent, loss, adv, weight):
      assert array.dtype == ftype, array.dtype
    assert np.array_equal(loss, weight[:, :-1] * -(logpi * adv + cases.ACTENT * ent))
    return logpi, ent, loss, adv, weight

  return run, lines


def generate():
  run32, lines = runner(np.float32)
  run64, _ = runner(np.float64)
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  for case, c in enumerate(cases.CASES):
    inp = cases.inputs(case)
    name = cases.tag(case)
    out[f'in_{name}'] = cases.digest(inp)
    for run, suffix in ((run32, ''), (run64, '64')):
      logpi, ent, loss, adv, weight = run(inp, c)
      stacked = np.stack([logpi, ent, loss])
      assert stacked.shape == (len(cases.FIELDS), cases.N, cases.T - 1) and np.isfinite(stacked).all(), name
      out[f'out{suffix}_{name}'] = stacked
      out[f'adv{suffix}_{name}'] = adv
      out[f'weight{suffix}_{name}'] = weight
    # exact in float32: both runs hand the loss the same constants
    assert np.array_equal(out[f'adv_{name}'], out[f'adv64_{name}']), name
    assert np.array_equal(out[f'weight_{name}'], out[f'weight64_{name}']), name
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'normal_policy.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'normal_policy: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
