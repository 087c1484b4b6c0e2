"""Generate tests/golden/optim.npz by EXECUTING the reference's own `clip_by_agc`,
`scale_by_rms` and `scale_by_momentum` (embodied/jax/opt.py:109-164) and its `rms`
(embodied/jax/nets.py:120-124) under numpy stand-ins.

Needs the reference tree (oracle/refload.py says where).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_optim_golden.py

The functions are taken out of the syntax tree and compiled on their own
(`oracle.gen_scan_golden.extract`); none of their text is written anywhere.

Stand-ins defined here, for one float type at a time:
  jnp               numpy; `linalg.norm`, `zeros_like(t, f32)`, `zeros((), i32)`
  f32               the float type of the run
  jax.tree.map      a list comprehension over lists of arrays; `leaves` = list
  optax.GradientTransformation   a pair (init, update)
  optax.safe_int32_increment     + 1
  optax.bias_correction(m, d, t) m / (1 - d ** t), the divisor in the float type
  optax.update_moment(g, m, d, 1)   (1 - d) * g + d * m
The rest of the chain is restated here, its places in the reference asserted by
what those lines call (public optax names only):
  agent.py:365   optax.add_decayed_weights(wd, mask): + wd * p where masked
  agent.py:376-378   the warm-up joined to the constant, optax.scale_by_learning_rate:
                 * -schedule(count), count the number of updates so far
  opt.py:62      optax.apply_updates: p + upd
  opt.py:64      optax.global_norm of the raw gradients

Every case runs in float32 (what the reference computes) and in float64 over the
same float32 inputs (what the tests hold the kernels against).  Only data is
written: the cases' input digests and, per case and precision, one (steps, 3 S + 4)
array (`cases.unpack`): p, nu and mu at `cases.sample_index` of every tensor, S
elements each, and the four metrics.
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
from tests import optim_cases as cases  # noqa: E402

CALLS = (('dreamerv3/agent.py', 365, 'add_decayed_weights'), ('dreamerv3/agent.py', 376, 'linear_schedule'),
         ('dreamerv3/agent.py', 377, 'join_schedules'), ('dreamerv3/agent.py', 378, 'scale_by_learning_rate'),
         ('embodied/jax/opt.py', 62, 'apply_updates'), ('embodied/jax/opt.py', 64, 'global_norm'))


def assert_calls():
  """The restated lines still call what this tool restates."""
  for relpath, line, name in CALLS:
    tree = ast.parse((refload.REFERENCE / relpath).read_text())
    called = {n.func.attr for n in ast.walk(tree)
              if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.lineno == line}
    assert name in called, (relpath, line, name, called)


def stand_ins(ftype):
  tree_map = lambda fn, *trees: [fn(*leaves) for leaves in zip(*trees)]

  class Jnp:
    linalg = types.SimpleNamespace(norm=lambda x, order: np.sqrt(np.sum(np.square(x))).astype(ftype))

    def __getattr__(self, name):
      return getattr(np, name)

  optax = types.SimpleNamespace(
      GradientTransformation=lambda init, update: types.SimpleNamespace(init=init, update=update),
      safe_int32_increment=lambda step: step + 1,
      bias_correction=lambda moment, decay, count: tree_map(lambda m: m / ftype(1 - decay ** int(count)), moment),
      update_moment=lambda updates, moments, decay, order: tree_map(
          lambda g, m: (1 - decay) * (g ** order) + decay * m, updates, moments))
  jax = types.SimpleNamespace(tree=types.SimpleNamespace(map=tree_map, leaves=list))
  return dict(jax=jax, jnp=Jnp(), optax=optax, f32=ftype, i32=np.int32)


def runner(ftype):
  """run(inp, hyper, specs) -> per step (p, nu, mu, metrics), the reference's
  three transformations executed in `ftype`, the rest restated."""
  names = stand_ins(ftype)
  fns, lines = {}, {}
  for name in ('clip_by_agc', 'scale_by_rms', 'scale_by_momentum'):
    fns[name], lines[name] = gen_scan_golden.extract('embodied/jax/opt.py', name)
    fns[name].__globals__.update(names)
  rms, lines['rms'] = gen_scan_golden.extract('embodied/jax/nets.py', 'rms')
  rms.__globals__.update(names)

  def run(inp, hyper, specs):
    mask = cases.mask_of(specs)
    chain = [fns['clip_by_agc'](hyper.agc, cases.PMIN), fns['scale_by_rms'](cases.BETA2, cases.EPS),
             fns['scale_by_momentum'](cases.BETA1, hyper.nesterov)]                 # agent.py:358-360
    params = [x.astype(ftype) for x in inp['p']]
    states = [t.init(params) for t in chain]
    out = []
    for step in range(cases.STEPS):
      grads = [x.astype(ftype) for x in inp['g'][step]]
      updates = grads
      for k, t in enumerate(chain):
        updates, states[k] = t.update(updates, states[k], params)
      if hyper.wd:                                                                  # agent.py:361-365
        updates = [u + hyper.wd * p if decays else u for u, p, decays in zip(updates, params, mask)]
      rate = cases.schedule(hyper.lr, hyper.warmup, step)                           # agent.py:367-377
      updates = [u * -rate for u in updates]                                        # agent.py:378
      params = [p + u for p, u in zip(params, updates)]                             # opt.py:62
      global_norm = np.sqrt(sum(np.sum(np.square(g)) for g in grads)) if grads else ftype(0)   # opt.py:64
      metrics = np.array([global_norm, rms(grads), rms(updates), rms(params)])      # opt.py:75-78
      (step_rms, nu), (step_mom, mu) = states[1], states[2]
      assert step_rms == step_mom == step + 1
      for array in (*params, *nu, *mu, metrics):
        assert array.dtype == ftype, array.dtype
      out.append((params, list(nu), list(mu), metrics))
    return out

  return run, lines


def generate():
  assert_calls()
  run32, lines = runner(np.float32)
  run64, _ = runner(np.float64)
  out = {f'lines_{name}': np.array(span) for name, span in lines.items()}
  digests = []
  for case, c in enumerate(cases.CASES):
    specs = cases.LISTS[c.list]
    inp = cases.inputs(case)
    name = cases.tag(case)
    digests.append(cases.flat_digest(inp))
    for run, suffix in ((run32, ''), (run64, '64')):
      steps = run(inp, c.hyper, specs)
      packed = np.stack([np.concatenate([*(cases.sampled(step[k]) for k in range(3)), step[3]]) for step in steps])
      assert np.isfinite(packed).all() and packed.dtype == (np.float64 if suffix else np.float32), name
      out[f'out{suffix}_{name}'] = packed
    if c.list == 'agc' and c.hyper.agc:
      # the three regimes the list is there for, at the first step
      g, p = inp['g'][0], inp['p']
      rel = [np.linalg.norm(g[i].ravel()) / (c.hyper.agc * max(cases.PMIN, np.linalg.norm(p[i].ravel()))) for i in range(3)]
      assert rel[0] < 1 < rel[1] and np.linalg.norm(p[2].ravel()) < cases.PMIN, rel
  out['inputs'] = np.stack(digests)
  return out


def main():
  out = generate()
  path = ROOT / 'tests' / 'golden' / 'optim.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  assert size < 900_000, size
  print(f'optim: {len(cases.CASES)} cases, {len(out)} arrays, {size} bytes')


if __name__ == '__main__':
  main()
