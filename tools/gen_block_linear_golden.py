"""Generate tests/golden/block_linear.npz by EXECUTING the reference's own
`BlockLinear.__call__` (embodied/jax/nets.py) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_block_linear_golden.py

`BlockLinear` is taken out of the syntax tree as a class and compiled, as
`tools/gen_rssm_core_golden.py` does with `Norm`.  Its text is written nowhere.

Stand-ins defined here:
  nj.Module            a plain base class
  Initializer, init    placeholders: the class body names them, `value` below never calls them
  BlockLinear.value    returns the case's kernel / bias in the shape it is asked for
  ensure_dtypes        nothing
  jnp                  numpy (oracle/shims/jaxlike.py): `einsum('...ki,kio->...ko')`

Every case runs in float32 and in float64 over the same inputs (x rounded to
bfloat16, the parameters float32).  Only data is written: per case the inputs,
the output per precision, and the reference's line numbers.
"""
import ast
import math
import pathlib
import sys
import types
from typing import Callable

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import refload  # noqa: E402
from oracle.shims import jaxlike  # noqa: E402
from tests import block_linear_cases as cases  # noqa: E402


class _Module:
  pass


def reference_block_linear():
  path = refload.REFERENCE / 'embodied' / 'jax' / 'nets.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'BlockLinear')
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(nj=types.SimpleNamespace(Module=_Module), Initializer=lambda *a, **k: None, init=lambda x: x,
                   ensure_dtypes=lambda x: None, math=math, Callable=Callable)
  exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), 'exec'), namespace)
  return namespace['BlockLinear'], (node.lineno, node.end_lineno)


def run(BlockLinear, inp, g, i, o, ftype):
  layer = BlockLinear(g * o, g)
  layer.bias = inp['bias'] is not None
  params = {'kernel': inp['kernel'], 'bias': inp['bias']}
  shapes = {'kernel': (g, i, o), 'bias': g * o}

  def value(name, initializer, shape):
    assert shape == shapes[name], (name, shape)
    return np.asarray(params[name], ftype).reshape(shape)

  layer.value = value
  out = layer(inp['x'].astype(ftype))
  assert out.dtype == ftype and out.shape == (*inp['x'].shape[:-1], g * o)
  return np.asarray(out)


def generate():
  BlockLinear, lines = reference_block_linear()
  arrays = {'lines_BlockLinear': np.array(lines)}
  for case, (g, i, o, lead, bias) in enumerate(cases.GOLDEN):
    inp = cases.inputs(case)
    name = cases.tag(case)
    arrays[f'in_{name}'] = cases.digest(cases.present(inp))
    for ftype, suffix in ((np.float32, ''), (np.float64, '64')):
      arrays[f'out{suffix}_{name}'] = run(BlockLinear, inp, g, i, o, ftype)
  return arrays


def main():
  arrays = generate()
  path = ROOT / 'tests' / 'golden' / 'block_linear.npz'
  np.savez_compressed(path, **arrays)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'block_linear: {len(cases.GOLDEN)} cases, {len(arrays)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
