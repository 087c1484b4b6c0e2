"""Shapes, seeded inputs and a numpy float64 restatement, with all three
gradients and the derived error bars, of BlockLinear (embodied/jax/nets.py:254-278).

Shared by `tools/gen_block_linear_golden.py` (which feeds the fixture's inputs to
the reference's own `BlockLinear.__call__`) and the tests.  `reference64` is this
project's own numpy code.  The host test holds its forward against the fixture's
float64 values, its gradients against central differences, and the case table
against the conditions it was chosen for.  The table, the exact-integer inputs
and the bars are what a device BlockLinear on the bfloat16 matrix cores is to be
tested with; no such kernel is in the library yet.
"""
import itertools

import numpy as np

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# The geometry the table is chosen for: the `v_mfma_f32_16x16x32_bf16` tile (32 of
# the contraction index, 16 of the other), a switch from a skinny to a tiled
# kernel above 32 rows, a tiled kernel of 128-row tiles with at most 1024 of them
# per grid pass, a weight-gradient tile of 64 x 64 that walks 32 rows at a time
TILE_K, TILE_N, SKINNY_ROWS, TILED_ROWS, MAX_ROW_BLOCKS, GRAD_TILE, GRAD_ROWS = 32, 16, 32, 128, 1024, 64, 32

G = (1, 3, 8)
I = (8, 40, 64, 264)              # K tail; more than one K step; not a multiple of 32
O = (8, 24, 64, 136)              # column-tile tail; several tiles
# row-tile tails; the skinny / tiled switch (32 | 33) on both sides
ROWS = (1, 15, 16, 17, 32, 33, 130)


def _sweep():
  """Every (I, O) pair at two row counts, g in turn; every row count at two fixed
  shapes, one with tails everywhere and the largest."""
  cases = []
  for n, (i, o) in enumerate(itertools.product(I, O)):
    cases.append((G[n % 3], i, o, ROWS[n % 7]))
    cases.append((G[(n + 1) % 3], i, o, ROWS[(n + 4) % 7]))
  for rows in ROWS:
    cases.append((3, 40, 24, rows))
    cases.append((8, 264, 136, rows))
  return tuple(dict.fromkeys(cases))


SWEEP = _sweep()                                  # (g, I, O, rows)
REAL = (8, 256, 64, 16)                           # size1m dynhid0 at the scan's 16 rows
# more rows than one grid pass of the tiled kernel takes, tiny I and O
STRIDED = (1, 8, 8, TILED_ROWS * MAX_ROW_BLOCKS + 1)
LEADING = (3, 40, 24, (2, 3))                     # leading dims (2, 3)
EXACT = ((1, 8, 8, 1), (3, 40, 24, 17), (8, 64, 64, 33), (8, 264, 136, 130), (3, 264, 24, 32))
# the size1m _core tail: rows, deter, hidden, blocks
CHAIN = (16, 512, 64, 8)
# the fixture (tests/golden/block_linear.npz): small shapes, with and without a bias,
# leading dims, the debug config
GOLDEN = ((1, 8, 8, (1,), True), (3, 40, 24, (5,), True), (8, 64, 8, (2, 3), False), (4, 11, 2, (3,), True),
          (3, 264, 136, (2,), True))


def tag(case):
  g, i, o, lead, bias = GOLDEN[case]
  return f'c{case}_{g}x{i}x{o}_{"x".join(map(str, lead))}_{"bias" if bias else "plain"}'


def inputs_of(g, i, o, rows, rng, bias=True):
  """x (rows, g * I) and gout (rows, g * O) N(0, 1) rounded to bfloat16, kernel
  (g, I, O) N(0, 1) / sqrt(I) and bias N(0, 1), float32."""
  return {'x': bf16_round(rng.standard_normal((rows, g * i)).astype(f32)),
          'kernel': (rng.standard_normal((g, i, o)) / np.sqrt(i)).astype(f32),
          'bias': rng.standard_normal(g * o).astype(f32) if bias else None,
          'gout': bf16_round(rng.standard_normal((rows, g * o)).astype(f32))}


def inputs(case):
  g, i, o, lead, bias = GOLDEN[case]
  inp = inputs_of(g, i, o, int(np.prod(lead)), np.random.default_rng([case, g, i, o]), bias)
  inp['x'] = inp['x'].reshape(*lead, g * i)
  inp['gout'] = inp['gout'].reshape(*lead, g * o)
  return inp


def present(inp):
  return {k: v for k, v in inp.items() if v is not None}


def reference64(x, kernel, bias=None, gout=None):
  """nets.py:269-277 in float64 over the values given (x (rows, g * I), kernel
  (g, I, O)): dict of out and its `S = sum |a b|`; with gout also dx, dw, dbias and
  their S."""
  w = np.asarray(kernel, np.float64)
  g, i, o = w.shape
  x = np.asarray(x, np.float64).reshape(-1, g, i)
  out = np.einsum('rki,kio->rko', x, w)
  result = {'out_abs': np.einsum('rki,kio->rko', np.abs(x), np.abs(w)).reshape(-1, g * o)}
  result['product'] = out.reshape(-1, g * o)
  if bias is not None:
    out = out + np.asarray(bias, np.float64).reshape(g, o)
  result['out'] = out.reshape(-1, g * o)
  if gout is None:
    return result
  dy = np.asarray(gout, np.float64).reshape(-1, g, o)
  result.update(
      dx=np.einsum('rko,kio->rki', dy, w).reshape(-1, g * i),
      dx_abs=np.einsum('rko,kio->rki', np.abs(dy), np.abs(w)).reshape(-1, g * i),
      dw=np.einsum('rki,rko->kio', x, dy), dw_abs=np.einsum('rki,rko->kio', np.abs(x), np.abs(dy)),
      dbias=dy.sum(0).reshape(-1), dbias_abs=np.abs(dy).sum(0).reshape(-1))
  return result


def bar_bf16(total, absolute, length, bias=None):
  """2^-8 (|sum a b| + |bias|) + 2 (K + 1) 2^-24 S: a bfloat16 rounding and the
  float32 accumulation bound of a contraction of length K.  bfloat16 keeps 8
  significant bits, so ONE rounding to nearest is already up to 2^-8 relative: a
  path that rounds once (float32 bias added before the store) fits this bar, the
  reference's own sequence (round the product, round the bias, add, round) can
  reach about twice it."""
  beta = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64))
  return 2.0 ** -8 * (np.abs(total) + beta) + 2 * (length + 1) * 2.0 ** -24 * absolute


def bar_f32(total, absolute, length):
  """2^-23 |sum a b| + 2 (K + 1) 2^-24 S for a float32 result."""
  return 2.0 ** -23 * np.abs(total) + 2 * (length + 1) * 2.0 ** -24 * absolute


def bars(ref, kernel_shape, rows, bias=None, wide_sums=False):
  """The bar of every output of `reference64` (a dict by the same names).  `dw`
  and `dbias` get the float32 bar, or with `wide_sums` (the composed path, whose
  sums pass through bfloat16) the bfloat16 one."""
  g, i, o = kernel_shape
  out = {'out': bar_bf16(ref['product'], ref['out_abs'], i, None if bias is None else np.tile(bias, (rows, 1)))}
  if 'dx' in ref:
    sums = bar_bf16 if wide_sums else bar_f32
    out.update(dx=bar_bf16(ref['dx'], ref['dx_abs'], o), dw=sums(ref['dw'], ref['dw_abs'], rows),
               dbias=sums(ref['dbias'], ref['dbias_abs'], rows))
  return out


def ratio(got, want, bar):
  """Worst |got - want| / bar over EVERY element (an element with a zero bar must be exact)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(got).all() and np.isfinite(want).all()
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))


def exact_inputs(g, i, o, rows):
  """Small integers, the kernel asymmetric in (k, i, o): every partial sum is far
  below 2^24 (at most 264 * 16 forward, 136 * 16 for dx, 130 * 16 for dW)."""
  r, k, ii, oo = np.arange(rows)[:, None, None], np.arange(g)[None, :, None], np.arange(i), np.arange(o)
  x = ((r * 7 + k * 3 + ii[None, None, :] * 5) % 9 - 4).reshape(rows, g * i)
  gout = ((r * 5 + k * 7 + oo[None, None, :] * 3) % 7 - 3).reshape(rows, g * o)
  kernel = (np.arange(g)[:, None, None] * 3 + ii[None, :, None] * 5 + oo[None, None, :] * 7) % 9 - 4
  bias = (np.arange(g * o) * 11) % 13 - 6
  return {'x': x.astype(np.int64), 'kernel': kernel.astype(np.int64), 'bias': bias.astype(np.int64),
          'gout': gout.astype(np.int64)}


def exact_outputs(inp):
  g, i, o = inp['kernel'].shape
  x, dy, w = inp['x'].reshape(-1, g, i), inp['gout'].reshape(-1, g, o), inp['kernel']
  return {'out': (np.einsum('rki,kio->rko', x, w) + inp['bias'].reshape(g, o)).reshape(-1, g * o),
          'dx': np.einsum('rko,kio->rki', dy, w).reshape(-1, g * i),
          'dw': np.einsum('rki,rko->kio', x, dy), 'dbias': dy.sum(0).reshape(-1)}
