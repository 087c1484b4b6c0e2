"""Generate tests/golden/recon_loss.npz by EXECUTING the reference's own `Output`,
`Agg`, `MSE` and `Binary` classes (embodied/jax/outs.py) and `symlog`
(embodied/jax/nets.py) under numpy stand-ins, in float64.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_recon_loss_golden.py

The classes are taken out of the syntax tree together and compiled, as
`tools/gen_onehot_sample_golden.py` does; `symlog` as
`oracle.gen_scan_golden.extract` takes a function.  None of these texts is
written anywhere.  What is executed per case of `tests/recon_loss_cases.CASES`:

  mse      Agg(MSE(x), 1, jnp.sum).loss(target)
  symlog   Agg(MSE(x, symlog), 1, jnp.sum).loss(target)               (heads.py:127-130)
  sigmoid  Agg(MSE(jax.nn.sigmoid(x)), 1, jnp.sum).loss(f32(image) / 255)
           (rssm.py:349, 353-356, agent.py:181; the division in float32, then widened)
  binary   Agg(Binary(x), 1, jnp.sum).loss(label)                     (agent.py:177)

Stand-ins beyond those of `tools/gen_policy_loss_golden.py`, defined here:
  jax.nn.sigmoid       1 / (1 + exp(-x))
  jax.nn.log_sigmoid   min(x, 0) - log1p(exp(-|x|))
  jnp.square, jnp.issubdtype, jnp.floating    numpy's own

Only data is written: per case the inputs' digest, the per-row losses (float64),
the per-element losses for rows of at most 64 units, and the reference's line
numbers.
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
from tests import recon_loss_cases as cases  # noqa: E402
from tools.gen_policy_loss_golden import _jax, jnp  # noqa: E402

CLASSES = ('Output', 'Agg', 'MSE', 'Binary')


def _jax_with_sigmoid(ftype):
  jax = _jax(ftype)

  def sigmoid(x):
    return 1 / (1 + np.exp(-x))

  def log_sigmoid(x):
    return np.minimum(x, 0) - np.log1p(np.exp(-np.abs(x)))

  jax.nn.sigmoid, jax.nn.log_sigmoid = sigmoid, log_sigmoid
  return jax


def reference_classes(ftype):
  """The reference's four output classes and `symlog`, compiled with `f32` = ftype."""
  path = refload.REFERENCE / 'embodied' / 'jax' / 'outs.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
  assert [n.name for n in nodes] == list(CLASSES)
  jax = _jax_with_sigmoid(ftype)
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(jax=jax, jnp=jnp, f32=ftype, i32=np.int32, sg=jax.lax.stop_gradient)
  exec(compile(ast.Module(body=nodes, type_ignores=[]), str(path), 'exec'), namespace)
  lines = {n.name: (n.lineno, n.end_lineno) for n in nodes}
  symlog, lines['symlog'] = gen_scan_golden.extract('embodied/jax/nets.py', 'symlog')
  symlog.__globals__.update(jnp=jnp)
  outs = types.SimpleNamespace(**{name: namespace[name] for name in CLASSES}, symlog=symlog, jax=jax)
  return outs, lines


def run(outs, op, x, target, dims, ftype):
  """The reference's per-row loss (dims = 1) or per-element loss (dims = 0)."""
  x = x.astype(ftype)
  if op == 'sigmoid':
    head, target = outs.MSE(outs.jax.nn.sigmoid(x)), (target.astype(np.float32) / np.float32(255)).astype(ftype)
  elif op == 'symlog':
    head, target = outs.MSE(x, outs.symlog), target.astype(ftype)
  elif op == 'mse':
    head, target = outs.MSE(x), target.astype(ftype)
  else:
    head, target = outs.Binary(x), target.astype(ftype)
  agg = outs.Agg(head, dims, jnp.sum)
  agg.axes = tuple(agg.axes)                                         # ndarray.sum refuses a list
  return agg.loss(target) if dims else head.loss(target)


def generate():
  ftype = np.float64
  outs, lines = reference_classes(ftype)
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  for case, c in enumerate(cases.CASES):
    inp = cases.inputs(case)
    name = cases.tag(case)
    loss = run(outs, c.op, inp['x'], inp['target'], 1, ftype)
    assert loss.dtype == ftype and loss.shape == (c.rows,) and np.isfinite(loss).all(), name
    out[f'in_{name}'] = cases.digest(inp)
    out[f'loss_{name}'] = loss
    if c.units <= cases.ELEMENTWISE_MAX:
      terms = run(outs, c.op, inp['x'], inp['target'], 0, ftype)
      assert terms.shape == inp['x'].shape and np.allclose(terms.sum(-1), loss, rtol=1e-14, atol=0), name
      out[f'terms_{name}'] = terms
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'recon_loss.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'recon_loss: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
