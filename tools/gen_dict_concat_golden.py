"""Generate tests/golden/dict_concat.npz by EXECUTING the reference's own
`DictConcat`, `available`, `mask`, `where` and `symlog` (embodied/jax/nets.py)
under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_dict_concat_golden.py

`DictConcat` is taken out of the syntax tree as a class and compiled, as
`tools/gen_rssm_core_golden.py` does with `Norm`; the four functions with
`oracle.gen_scan_golden.extract`.  None of these texts is written anywhere.

Stand-ins defined here, for one float type at a time:
  jnp                  numpy (oracle/shims/jaxlike.py)
  jax.nn.one_hot       (x[..., None] == arange(classes)).astype(dtype): JAX's definition
  jax.tree.map         over dicts of arrays, or the arrays themselves
  COMPUTE_DTYPE        the float type of the run
Spaces are `embodied_amd.space.Space`, whose `classes` the reference reads.

Around the extracted call, restated here with the reference's lines cited:
  dreamerv3/rssm.py:76-79   action = mask(action, ~reset) in front, mask(..., ~reset) behind
  dreamerv3/rssm.py:137     action /= max(1, |action|)
(the masks run through the reference's own `mask`).

Every case runs in float32 and in float64 over the same inputs; a float input
is widened before the float64 run, so `symlog` runs in float64 too.  Only data
is written: per case the inputs' digest, the output per precision, and the
reference's line numbers.
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
from tests import dict_concat_cases as cases  # noqa: E402

RSSM_MASK_LINES, RSSM_CLAMP_LINE = (76, 79), 137


def _tree_map(fn, *trees):
  if isinstance(trees[0], dict):
    return {k: _tree_map(fn, *(t[k] for t in trees)) for k in trees[0]}
  return fn(*trees)


def _one_hot(x, classes, dtype):
  return (np.asarray(x)[..., None] == np.arange(classes)).astype(dtype)


JAX = types.SimpleNamespace(nn=types.SimpleNamespace(one_hot=_one_hot), tree=types.SimpleNamespace(map=_tree_map))


def reference(ftype):
  """The reference's `DictConcat` compiled with COMPUTE_DTYPE = ftype, its `mask`
  and `symlog`, and the lines of all five."""
  lines, fns = {}, {}
  for name in ('available', 'mask', 'where', 'symlog'):
    fns[name], lines[name] = gen_scan_golden.extract('embodied/jax/nets.py', name)
  for fn in fns.values():
    fn.__globals__.update(jax=JAX, **fns)
  path = refload.REFERENCE / 'embodied' / 'jax' / 'nets.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DictConcat')
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(jax=JAX, COMPUTE_DTYPE=ftype, **fns)
  exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), 'exec'), namespace)
  lines['DictConcat'] = (node.lineno, node.end_lineno)
  return namespace['DictConcat'], fns, lines


def run(DictConcat, fns, c, inp, ftype):
  xs = {k.name: (inp[k.name].astype(ftype) if inp[k.name].dtype.kind == 'f' else inp[k.name]) for k in c.keys}
  squish = {None: (lambda x: x), 'symlog': fns['symlog']}[c.squish]
  reset = inp.get('reset')
  if reset is not None:
    xs = fns['mask'](xs, ~reset)                                     # rssm.py:76-79, in front
  out = DictConcat(cases.spaces_of(c.keys), 1, squish)(xs)
  if reset is not None:
    out = fns['mask'](out, ~reset)                                   # rssm.py:76-79, behind
  if c.unit:
    with np.errstate(invalid='ignore'):
      out = out / np.maximum(1, np.abs(out))                         # rssm.py:137
  assert out.dtype == ftype and out.shape == (c.rows, cases.width_of(c.keys)), (out.dtype, out.shape)
  return np.asarray(out)


def generate():
  out = {'lines_rssm_mask': np.array(RSSM_MASK_LINES), 'lines_rssm_clamp': np.array([RSSM_CLAMP_LINE] * 2)}
  for ftype, suffix in ((np.float32, ''), (np.float64, '64')):
    DictConcat, fns, lines = reference(ftype)
    out.update({f'lines_{name}': np.array(span) for name, span in lines.items()})
    for case, c in enumerate(cases.CASES):
      inp = cases.inputs(case)
      out[f'in_{cases.tag(case)}'] = cases.digest(inp)
      with np.errstate(invalid='ignore'):
        out[f'out{suffix}_{cases.tag(case)}'] = run(DictConcat, fns, c, inp, ftype)
  return out


def main():
  arrays = generate()
  path = ROOT / 'tests' / 'golden' / 'dict_concat.npz'
  np.savez_compressed(path, **arrays)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'dict_concat: {len(cases.CASES)} cases, {len(arrays)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
