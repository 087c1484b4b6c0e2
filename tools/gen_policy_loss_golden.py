"""Generate tests/golden/policy_loss.npz by EXECUTING the reference's own
`imag_loss` (dreamerv3/agent.py) with its own output classes `Output`, `Agg` and
`Categorical` (embodied/jax/outs.py) as the policy, under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_policy_loss_golden.py

The three classes are taken out of the syntax tree together and compiled, as
`tools/gen_rssm_kl_golden.py` does; `imag_loss` and `lambda_return` as
`tools/gen_dreamer_targets_golden.py` does (`oracle.gen_scan_golden.extract`).
None of these texts is written anywhere.  `imag_loss` is executed whole: the
policy is `{'action': Agg(Categorical(logits, unimix), dims, jnp.sum)}` built
from the reference's classes (heads.py:90-91, 101-110 builds the same), `value`
and `slowvalue` return the case's `pred`, `value.loss` returns zeros, and the
three normalisers are recording stand-ins that return (0, 1), so `adv_normed` is
exactly the `adv` the advantage normaliser was handed.

Stand-ins defined here, for one float type at a time:
  jax.nn.softmax       exp(x - max) / sum(exp(x - max)) over the axis
  jax.nn.log_softmax   (x - max) - log(sum(exp(x - max)))
  jax.nn.one_hot       (index == arange(n)) in the float type
  jnp                  numpy, with a `sum` that takes `Agg`'s list of axes
  f32                  the float type of the run
  Agg(...).axes        the list `Agg.__init__` made, as a tuple (ndarray.sum
                       refuses a list)
Every case runs in float32 (what the reference computes) and in float64 over
the same float32 inputs (what the parity tests hold the kernels against).
`cases.PARAMS` and the inputs make the lambda-return exact in float32, so both
runs hand the loss the same advantages and weights (asserted).

`imag_loss` keeps `weight` to itself (only its mean leaves, as a metric), so
that ONE line of it (agent.py:402) is restated by this tool and the metric
`weight` of the executed function is asserted equal to the restated array's mean,
as tools/gen_dreamer_targets_golden.py does.

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
from tests import policy_loss_cases as cases  # noqa: E402

CLASSES = ('Output', 'Agg', 'Categorical')


class _Jnp:
  """numpy; `sum` accepts the list of axes that `Agg` passes (numpy.sum refuses one)."""

  def __getattr__(self, name):
    return getattr(np, name)

  @staticmethod
  def sum(x, axis=None):
    return np.sum(x, tuple(axis) if isinstance(axis, list) else axis)


jnp = _Jnp()


def _jax(ftype):
  def softmax(x, axis=-1):
    unnormalized = np.exp(x - x.max(axis, keepdims=True))
    return unnormalized / unnormalized.sum(axis, keepdims=True)

  def log_softmax(x, axis=-1):
    shifted = x - x.max(axis, keepdims=True)
    return shifted - np.log(np.exp(shifted).sum(axis, keepdims=True))

  def one_hot(index, n, dtype=None):
    return (np.asarray(index)[..., None] == np.arange(n)).astype(dtype or ftype)

  return types.SimpleNamespace(
      nn=types.SimpleNamespace(softmax=softmax, log_softmax=log_softmax, one_hot=one_hot),
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
  outs, class_lines = reference_classes(ftype)
  imag_loss, imag_lines = gen_scan_golden.extract('dreamerv3/agent.py', 'imag_loss')
  lambda_return, lambda_lines = gen_scan_golden.extract('dreamerv3/agent.py', 'lambda_return')
  imag_loss.__globals__.update(lambda_return=lambda_return, jnp=jnp)

  def run(inp, c):
    dims = 1 if c.groups else 0
    policy = outs.Agg(outs.Categorical(inp['logits'].astype(ftype), c.unimix), dims, jnp.sum)
    policy.axes = tuple(policy.axes)
    rew, con, pred = (inp[k].astype(ftype) for k in ('rew', 'con', 'pred'))
    value = types.SimpleNamespace(pred=lambda: pred, loss=lambda target: np.zeros_like(pred))
    retnorm, valnorm, advnorm = Recording(), Recording(), Recording()
    losses, _, metrics = imag_loss(
        {'action': inp['act']}, rew, con, {'action': policy}, value, value, retnorm, valnorm, advnorm, True,
        **cases.PARAMS)
    weight = np.cumprod(con, 1)                    # agent.py:402 with contdisc (disc = 1), restated (see above)
    assert np.array_equal(metrics['weight'], weight.mean()), 'the restated line is not agent.py:402'
    logpi, ent = policy.logp(inp['act'])[:, :-1], policy.entropy()[:, :-1]
    assert np.array_equal(metrics['ent/action'], ent.mean())
    loss, adv = losses['policy'], advnorm.fed
    for array in (logpi, ent, loss, adv, weight):
      assert array.dtype == ftype, array.dtype
    # the loss is what agent.py:413-414 makes of these
    assert np.array_equal(loss, weight[:, :-1] * -(logpi * adv + cases.ACTENT * ent))
    return logpi, ent, loss, adv, weight

  return run, dict(class_lines, imag_loss=imag_lines, lambda_return=lambda_lines)


def generate():
  run32, lines = runner(np.float32)
  run64, _ = runner(np.float64)
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  for case, c in enumerate(cases.CASES):
    inp = cases.inputs(case)
    name = cases.tag(case)
    out[f'in_{name}'] = cases.digest(inp)
    for run, ftype, suffix in ((run32, np.float32, ''), (run64, np.float64, '64')):
      logpi, ent, loss, adv, weight = run(inp, c)
      stacked = np.stack([logpi, ent, loss])
      assert stacked.shape == (len(cases.FIELDS), cases.N, cases.T - 1) and np.isfinite(stacked).all(), name
      out[f'out{suffix}_{name}'] = stacked
      out[f'adv{suffix}_{name}'] = adv
      out[f'weight{suffix}_{name}'] = weight
    # exact in float32: both runs hand the loss the same constants
    assert np.array_equal(out[f'adv_{name}'], out[f'adv64_{name}']), name
    assert np.array_equal(out[f'weight_{name}'], out[f'weight64_{name}']), name
    assert (out[f'weight_{name}'] == 0).any() and (out[f'weight_{name}'] == 1).any()
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'policy_loss.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'policy_loss: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
