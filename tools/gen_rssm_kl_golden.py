"""Generate tests/golden/rssm_kl.npz by EXECUTING the reference's own
`RSSM.loss` and `RSSM._dist` (dreamerv3/rssm.py) with the output classes they
use, `Output`, `Agg`, `Categorical` and `OneHot` (embodied/jax/outs.py), under
numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_rssm_kl_golden.py

The four classes are taken out of the syntax tree together and compiled, as
`tools/gen_twohot_golden.py` does for `TwoHot`; the two methods as
`oracle.gen_scan_golden.extract` does.  None of these texts is written
anywhere.  `loss` is executed whole against a stand-in `self`: `observe`
returns the case's `feat` (its 'logit' is the posterior), `_prior` returns the
case's prior logits, `unimix` and `free_nats` are plain attributes, `_dist` is
the reference's own method, `sg` is the identity.  `loss` reduces the two
entropies to their means, so the rows' entropies (and the raw kl) are read off
`_dist(...)` directly, the same objects `loss` builds.

Stand-ins defined here, for one float type at a time:
  jax.nn.softmax       exp(x - max) / sum(exp(x - max)) over the axis
  jax.nn.log_softmax   (x - max) - log(sum(exp(x - max)))
  jax.nn.one_hot       (index == arange(n)) in the float type
  jnp                  numpy, with a `sum` that takes `Agg`'s list of axes
  f32                  the float type of the run
Every case runs in float32 (what the reference computes) and in float64 over
the same float32 inputs (what the parity tests hold the kernels against), with
free_nats = 1 and free_nats = 0.

Only data is written: per case the inputs' digest and one (4, rows) array per
precision -- `cases.FIELDS`: the raw kl (= dyn = rep at free_nats = 0), dyn (=
rep) at free_nats = 1, and the rows' two entropies -- and the reference's line
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
from tests import rssm_kl_cases as cases  # noqa: E402

CLASSES = ('Output', 'Agg', 'Categorical', 'OneHot')


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
  """The reference's four output classes, compiled with `f32` = ftype."""
  path = refload.REFERENCE / 'embodied' / 'jax' / 'outs.py'
  tree = ast.parse(path.read_text(), filename=str(path))
  nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
  assert [n.name for n in nodes] == list(CLASSES)
  namespace = dict(jaxlike.NAMESPACE)
  namespace.update(jax=_jax(ftype), jnp=jnp, f32=ftype, i32=np.int32)
  exec(compile(ast.Module(body=nodes, type_ignores=[]), str(path), 'exec'), namespace)
  lines = {n.name: (n.lineno, n.end_lineno) for n in nodes}
  return types.SimpleNamespace(**{name: namespace[name] for name in CLASSES}), lines


def rssm_of(ftype):
  """`RSSM.loss` and `RSSM._dist`, executed whole: run(post, prior, unimix, free_nats)
  -> (losses, metrics, dist) with `dist` the bound `_dist`."""
  outs, class_lines = reference_classes(ftype)
  loss, loss_lines = gen_scan_golden.extract('dreamerv3/rssm.py', 'loss', cls='RSSM')
  dist, dist_lines = gen_scan_golden.extract('dreamerv3/rssm.py', '_dist', cls='RSSM')
  embodied = types.SimpleNamespace(jax=types.SimpleNamespace(outs=outs))
  loss.__globals__.update(jnp=jnp)
  dist.__globals__.update(jnp=jnp, embodied=embodied)

  def run(post, prior, unimix, free_nats):
    post, prior = post.astype(ftype), prior.astype(ftype)
    feat = {'deter': object(), 'logit': post}
    fake = types.SimpleNamespace(unimix=unimix, free_nats=free_nats)
    fake.observe = lambda carry, tokens, acts, reset, training: (carry, {}, feat)
    fake._prior = lambda deter: prior if deter is feat['deter'] else None
    fake._dist = lambda logits: dist(fake, logits)
    _, _, losses, got_feat, metrics = loss(fake, None, None, None, None, True)
    assert got_feat is feat and sorted(losses) == ['dyn', 'rep'] and sorted(metrics) == ['dyn_ent', 'rep_ent']
    return losses, metrics, fake._dist

  return run, dict(class_lines, loss=loss_lines, _dist=dist_lines)


def generate():
  run32, lines = rssm_of(np.float32)
  run64, _ = rssm_of(np.float64)
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  for case, c in enumerate(cases.CASES):
    inp = cases.inputs(case)
    name = cases.tag(case)
    out[f'in_{name}'] = cases.digest(inp)
    for run, ftype, suffix in ((run32, np.float32, ''), (run64, np.float64, '64')):
      rows = {}
      for free_nats, key in ((1.0, 'f1'), (0.0, 'f0')):
        losses, metrics, dist = run(inp['post'], inp['prior'], c.unimix, free_nats)
        rows[f'dyn_{key}'], rows[f'rep_{key}'] = losses['dyn'], losses['rep']
        post_d, prior_d = dist(inp['post'].astype(ftype)), dist(inp['prior'].astype(ftype))
        ent_post, ent_prior = post_d.entropy(), prior_d.entropy()
        # loss's own metrics are the means of these rows
        assert metrics['rep_ent'] == ent_post.mean() and metrics['dyn_ent'] == ent_prior.mean()
      rows['kl'] = post_d.kl(prior_d)
      assert np.array_equal(rows['kl'], rows['dyn_f0']) and np.array_equal(rows['kl'], rows['rep_f0'])
      assert np.array_equal(rows['dyn_f1'], np.maximum(rows['kl'], ftype(1.0)))
      assert np.array_equal(rows['dyn_f1'], rows['rep_f1'])       # sg only routes gradients
      stacked = np.stack([rows['kl'], rows['dyn_f1'], ent_post, ent_prior])
      assert stacked.dtype == ftype and stacked.shape == (len(cases.FIELDS), cases.ROWS), (name, stacked.dtype)
      out[f'out{suffix}_{name}'] = stacked
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'rssm_kl.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'rssm_kl: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
