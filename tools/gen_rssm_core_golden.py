"""Generate tests/golden/norm_act.npz and tests/golden/gru_gate.npz by EXECUTING
the reference's own `Norm.__call__` and `act` (embodied/jax/nets.py) and
`RSSM._core` (dreamerv3/rssm.py) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_rssm_core_golden.py

`Norm` is taken out of the syntax tree as a class and compiled, as
`tools/gen_policy_loss_golden.py` does with the output classes; `act` and `_core`
with `oracle.gen_scan_golden.extract`.  None of these texts is written anywhere.

Stand-ins defined here, for one float type at a time:
  nj.Module            a plain base class whose `_fields[...] = v` sets the attribute
  Norm.value           returns the case's scale / shift in the shape it is asked for
  f32                  the float type of the run, as an array whose `mean` takes the
                       list of axes `Norm` passes (numpy refuses a list)
  jax.lax.rsqrt        1 / sqrt(x)
  jax.nn.sigmoid       1 / (1 + exp(-x));  silu x sigmoid(x);  relu maximum(x, 0);
  jax.nn.gelu          the tanh approximation, jax's default (these four are JAX's,
                       not the reference's: restated from JAX's documentation)
  adc.checkpoint_name, ensure_dtypes    identities
For `_core`: `self.sub(name, ...)` returns a layer that returns a fixed array --
`dyngru` the case's x, every other layer zeros of its width, a `Norm` the
identity -- `nn.act` returns the identity and `einops.rearrange` is a reshape for
the two patterns `_core` uses.  What `_core` returns is then exactly the gate of
(x, deter).

Every case runs in float32 and in float64 over the same float32 inputs.  Only
data is written: per case the inputs' digest, the output per precision, and the
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
from tests import gru_gate_cases as gates  # noqa: E402
from tests import norm_act_cases as norms  # noqa: E402


class _Array(np.ndarray):
  """ndarray whose mean accepts the list of axes nets.py:378 builds."""

  def mean(self, axis=None, **kw):
    return np.asarray(self).mean(tuple(axis) if isinstance(axis, list) else axis, **kw).view(_Array)


def _sigmoid(x):
  with np.errstate(over='ignore'):
    return 1 / (1 + np.exp(-x))


def _gelu(x, approximate=True):
  assert approximate
  c = x.dtype.type(np.sqrt(2 / np.pi))
  cdf = x.dtype.type(0.5) * (x.dtype.type(1) + np.tanh(c * (x + x.dtype.type(0.044715) * (x ** 3))))
  return x * cdf


JAX = types.SimpleNamespace(
    nn=types.SimpleNamespace(sigmoid=_sigmoid, silu=lambda x: x * _sigmoid(x), gelu=_gelu,
                             relu=lambda x: np.maximum(x, 0)),
    lax=types.SimpleNamespace(rsqrt=lambda x: 1 / np.sqrt(x), stop_gradient=lambda x: x))


class _Fields:
  def __init__(self, owner):
    self.owner = owner

  def __setitem__(self, key, value):
    setattr(self.owner, key, value)


class _Module:
  @property
  def _fields(self):
    return _Fields(self)


def reference_norm(ftype):
  """The reference's `Norm`, compiled with f32 = ftype, and its `act`."""
  path = refload.REFERENCE / 'embodied' / 'jax' / 'nets.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Norm')
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(
      jax=JAX, nj=types.SimpleNamespace(Module=_Module), f32=lambda x: np.asarray(x, ftype).view(_Array),
      adc=types.SimpleNamespace(checkpoint_name=lambda x, name: x), ensure_dtypes=lambda x: None)
  exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), 'exec'), namespace)
  act, act_lines = gen_scan_golden.extract('embodied/jax/nets.py', 'act')
  act.__globals__.update(jax=JAX)
  return namespace['Norm'], act, {'Norm': (node.lineno, node.end_lineno), 'act': act_lines}


def run_norm(Norm, act, inp, c, ftype):
  spelled = c.impl if c.eps == 1e-4 else f'{c.impl}1em{round(-np.log10(c.eps))}'      # nets.py:369-371
  norm = Norm(spelled)
  assert norm.impl == c.impl and norm.eps == c.eps, (norm.impl, norm.eps)
  norm.scale, norm.shift = inp['scale'] is not None, inp['shift'] is not None
  params = {'scale': inp['scale'], 'shift': inp['shift']}
  norm.value = lambda name, init, shape, dtype: np.asarray(params[name], ftype).reshape(shape)
  out = act(c.act)(norm(inp['x'].astype(ftype)))
  assert out.dtype == ftype and out.shape == inp['x'].shape
  return np.asarray(out)


def generate_norm():
  out = {}
  for ftype, suffix in ((np.float32, ''), (np.float64, '64')):
    Norm, act, lines = reference_norm(ftype)
    out.update({f'lines_{name}': np.array(span) for name, span in lines.items()})
    for case, c in enumerate(norms.CASES):
      inp = norms.inputs(case)
      out[f'in_{norms.tag(case)}'] = norms.digest(norms.present(inp))
      out[f'out{suffix}_{norms.tag(case)}'] = run_norm(Norm, act, inp, c, ftype)
  return out


def _rearrange(x, pattern, g):
  if pattern == '... (g h) -> ... g h':
    return x.reshape(*x.shape[:-1], g, x.shape[-1] // g)
  assert pattern == '... g h -> ... (g h)', pattern
  return x.reshape(*x.shape[:-2], -1)


def generate_gate():
  core, lines = gen_scan_golden.extract('dreamerv3/rssm.py', '_core', cls='RSSM')
  nn = types.SimpleNamespace(Linear='Linear', BlockLinear='BlockLinear', Norm='Norm', act=lambda name: (lambda x: x))
  core.__globals__.update(jax=JAX, nn=nn, einops=types.SimpleNamespace(rearrange=_rearrange))
  out = {'lines__core': np.array(lines)}
  for case, (deter, blocks, scale) in enumerate(gates.CASES):
    inp = gates.inputs(case)
    name = gates.tag(case)
    out[f'in_{name}'] = gates.digest(inp)
    for ftype, suffix in ((np.float32, ''), (np.float64, '64')):
      rows = inp['x'].shape[0]

      def sub(layer, ctor, *args, **kw):
        if ctor == 'Norm':
          return lambda x: x
        if layer == 'dyngru':
          assert args == (3 * deter, blocks), args
          return lambda x: inp['x'].astype(ftype)
        return lambda x: np.zeros((rows, args[0]), ftype)

      rssm = types.SimpleNamespace(blocks=blocks, deter=deter, hidden=4, dynlayers=1, act='gelu', norm='rms', kw={},
                                   sub=sub)
      got = core(rssm, inp['deter'].astype(ftype), np.zeros((rows, 2, 3), ftype), np.zeros((rows, 2), ftype))
      assert got.dtype == ftype and got.shape == (rows, deter)
      out[f'out{suffix}_{name}'] = got
  return out


def main():
  for name, arrays, cases in (('norm_act', generate_norm(), norms.CASES), ('gru_gate', generate_gate(), gates.CASES)):
    path = ROOT / 'tests' / 'golden' / f'{name}.npz'
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    assert size < 900_000, size
    print(f'{name}: {len(cases)} cases, {len(arrays)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
