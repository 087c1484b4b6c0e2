"""Generate tests/golden/twohot.npz and tests/golden/twohot_edges.npz by EXECUTING the reference's own `TwoHot`
class with the `Output` class it inherits from (embodied/jax/outs.py),
`nets.symexp` (embodied/jax/nets.py) and the bin construction of
`Head.symexp_twohot` (embodied/jax/heads.py) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_twohot_golden.py

The two classes are taken out of the syntax tree together and compiled, as
`oracle.gen_normalize_golden.reference_class` does; `symexp` and the method
`symexp_twohot` as `oracle.gen_scan_golden.extract` does.  None of these texts
is written anywhere.  The method is executed whole against a stand-in `self`
(`space`, `bins`, `kw`, and a `sub` that returns the case's logits in place of
the linear layer), so the bins are the method's own: nothing of it is restated.

Stand-ins defined here, for one float type at a time:
  jax.nn.softmax                  exp(x - max) / sum(exp(x - max)) over the last axis
  jax.nn.one_hot                  (index == arange(n)) in the float type
  jax.scipy.special.logsumexp     log(sum(exp(x - max))) + max, max made finite
  jax.lax.stop_gradient           the identity
  jnp, f32, i32                   numpy; f32 is the float type of the run
Every case runs twice: in float32 (f32 = numpy.float32: what the reference
computes) and in float64 (f32 = numpy.float64 over the same float32 inputs and
bins: what the parity tests hold the kernels against).

Caveat, as oracle/shims/jaxlike.py states for FMA: numpy's
`linspace(dtype=float32)` and `expm1` may differ from XLA's in the last bit of
a bin, and numpy sums pairwise where XLA reduces in its own order.

Only data is written: the bins per n, per case the inputs' digest, `pred` and
the loss per target in both precisions, and the reference's line numbers.

twohot_edges.npz (`generate_edges`) is the float64 run of the same class over
`tests.twohot_cases.EDGE_CASES`: bins that are not the symexp set (asymmetric,
with runs of equal neighbours), logits with -inf, +inf, NaN and magnitudes up
to 1e4, four target sets per case at every edge of the two counts.  It is what
`tests.twohot_cases.reference64` is held against before the GPU tests use it
there.
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
from tests import twohot_cases as cases  # noqa: E402


def _jax(ftype):
  def softmax(x, axis=-1):
    unnormalized = np.exp(x - x.max(axis, keepdims=True))
    return unnormalized / unnormalized.sum(axis, keepdims=True)

  def one_hot(index, n, dtype=None):
    return (np.asarray(index)[..., None] == np.arange(n)).astype(dtype or ftype)

  def logsumexp(x, axis=None, keepdims=False):
    amax = x.max(axis, keepdims=True)
    amax = np.where(np.isfinite(amax), amax, 0)
    out = np.log(np.exp(x - amax).sum(axis, keepdims=True)) + amax
    return out if keepdims else np.squeeze(out, axis)

  return types.SimpleNamespace(
      nn=types.SimpleNamespace(softmax=softmax, one_hot=one_hot),
      scipy=types.SimpleNamespace(special=types.SimpleNamespace(logsumexp=logsumexp)),
      lax=types.SimpleNamespace(stop_gradient=lambda x: x))


def reference_classes(ftype):
  """The reference's `Output` and `TwoHot`, compiled with `f32` = ftype."""
  path = refload.REFERENCE / 'embodied' / 'jax' / 'outs.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ('Output', 'TwoHot')]
  assert [n.name for n in nodes] == ['Output', 'TwoHot']
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(jax=_jax(ftype), f32=ftype, i32=np.int32)
  exec(compile(ast.Module(body=nodes, type_ignores=[]), str(path), 'exec'), namespace)
  twohot = nodes[1]
  return namespace['TwoHot'], (twohot.lineno, twohot.end_lineno)


def head_of(TwoHot):
  """`Head.symexp_twohot`, executed whole: (logits, n) -> the TwoHot it returns."""
  method, lines = gen_scan_golden.extract('embodied/jax/heads.py', 'symexp_twohot', cls='Head')
  symexp, symexp_lines = gen_scan_golden.extract('embodied/jax/nets.py', 'symexp')
  method.__globals__.update(
      nets=types.SimpleNamespace(symexp=symexp, Linear=None), outs=types.SimpleNamespace(TwoHot=TwoHot))

  def build(logits, n):
    fake = types.SimpleNamespace(
        space=types.SimpleNamespace(discrete=False, shape=()), bins=n, kw={},
        sub=lambda name, ctor, shape, **kw: (lambda x: logits))
    return method(fake, None)

  return build, lines, symexp_lines


def generate():
  TwoHot32, class_lines = reference_classes(np.float32)
  TwoHot64, _ = reference_classes(np.float64)
  build, head_lines, symexp_lines = head_of(TwoHot32)
  out = {'twohot_lines': np.array(class_lines), 'head_lines': np.array(head_lines),
         'symexp_lines': np.array(symexp_lines)}
  for n in cases.BINS:
    bins = np.asarray(build(np.zeros((1, n), np.float32), n).bins)
    assert bins.dtype == np.float32 and bins.shape == (n,) and np.all(np.diff(bins) >= 0), n
    out[f'bins_{n}'] = bins
  for case, c in enumerate(cases.CASES):
    bins = out[f'bins_{c.n}']
    inp = cases.inputs(case, bins)
    name = cases.tag(case)
    out[f'in_{name}'] = cases.digest(inp)
    targets = [inp[f'target{k}'] for k in range(cases.TARGETS)]
    with np.errstate(invalid='ignore'):
      head = build(inp['logits'], c.n)                       # float32, through Head.symexp_twohot
      assert np.array_equal(head.bins, bins)
      pred, loss = head.pred(), np.stack([head.loss(t) for t in targets])
      assert pred.dtype == loss.dtype == np.float32, (pred.dtype, loss.dtype)
      head64 = TwoHot64(inp['logits'].astype(np.float64), bins.astype(np.float64))
      pred64 = head64.pred()
      loss64 = np.stack([head64.loss(t.astype(np.float64)) for t in targets])
      assert pred64.dtype == loss64.dtype == np.float64
    out[f'pred_{name}'], out[f'loss_{name}'] = pred, loss
    out[f'pred64_{name}'], out[f'loss64_{name}'] = pred64, loss64
  return out


def generate_edges():
  TwoHot64, class_lines = reference_classes(np.float64)
  build, _, _ = head_of(reference_classes(np.float32)[0])
  symexp_bins = lambda n: np.asarray(build(np.zeros((1, n), np.float32), n).bins)
  out = {'twohot_lines': np.array(class_lines)}
  for kind, n in cases.EDGE_SETS:
    out[f'bins_{kind}{n}'] = cases.edge_bins(kind, n, symexp_bins)
  for case, c in enumerate(cases.EDGE_CASES):
    bins = out[f'bins_{c.bins}{c.n}']
    inp = cases.edge_inputs(case, bins)
    name = cases.edge_tag(case)
    out[f'in_{name}'] = cases.digest(inp)
    with np.errstate(all='ignore'):
      head64 = TwoHot64(inp['logits'].astype(np.float64), bins.astype(np.float64))
      pred64 = head64.pred()
      loss64 = np.stack([head64.loss(inp[f'target{k}'].astype(np.float64)) for k in range(cases.EDGE_TARGETS)])
    assert pred64.dtype == loss64.dtype == np.float64
    out[f'pred64_{name}'], out[f'loss64_{name}'] = pred64, loss64
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'twohot.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'twohot: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')
  out = generate_edges()
  path = ROOT / 'tests' / 'golden' / 'twohot_edges.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 100_000, size
  print(f'twohot_edges: {len(cases.EDGE_CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
