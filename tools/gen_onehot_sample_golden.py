"""Generate tests/golden/onehot_sample.npz by EXECUTING the reference's own
`Categorical.__init__`, `Categorical.pred` and `OneHot._onehot_with_grad`
(embodied/jax/outs.py) under numpy stand-ins, in float64.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_onehot_sample_golden.py

The classes `Output`, `Categorical` and `OneHot` are taken out of the syntax tree
together and compiled, as `tools/gen_policy_loss_golden.py` does (whose numpy
stand-ins for `jax.nn.softmax`, `log_softmax`, `one_hot`, `jnp` and
`stop_gradient` are used here too); none of these texts is written anywhere.
`sample` itself is not executed: `jax.random.categorical` draws from threefry
keys, whose bits are outside this project's contract.  What the fixture holds is
what the draw is made from and into:

  probs    softmax of the logits `Categorical.__init__` keeps: the distribution
           `jax.random.categorical(seed, self.logits)` samples from
  argmax   `Categorical.pred()`
  value    `OneHot(...)._onehot_with_grad(index)` for the case's stored index

Only data is written: per case the inputs' digest, these three arrays (float64,
int32, float64) and the reference's line numbers.
"""
import ast
import pathlib
import sys
import types

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import refload  # noqa: E402
from oracle.shims import jaxlike  # noqa: E402
from tests import onehot_sample_cases as cases  # noqa: E402
from tools.gen_policy_loss_golden import _jax, jnp  # noqa: E402

CLASSES = ('Output', 'Categorical', 'OneHot')


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


def generate():
  ftype = np.float64
  outs, lines = reference_classes(ftype)
  softmax = _jax(ftype).nn.softmax
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  for case, c in enumerate(cases.CASES):
    inp = cases.inputs(case)
    name = cases.tag(case)
    logits = inp['logits'].astype(ftype)
    dist = outs.OneHot(logits, c.unimix)
    probs = softmax(dist.dist.logits, -1)
    argmax = dist.dist.pred()
    value = dist._onehot_with_grad(inp['index'])
    assert probs.dtype == ftype and value.dtype == ftype and probs.shape == value.shape == logits.shape, name
    assert np.isfinite(probs).all() and np.allclose(probs.sum(-1), 1.0, rtol=0, atol=1e-12), name
    assert set(np.unique(value)) <= {0.0, 1.0} and np.array_equal(np.argmax(value, -1), inp['index']), name
    out[f'in_{name}'] = cases.digest(inp)
    out[f'probs_{name}'] = probs
    out[f'argmax_{name}'] = np.asarray(argmax, np.int32)
    out[f'value_{name}'] = value
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'onehot_sample.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'onehot_sample: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
