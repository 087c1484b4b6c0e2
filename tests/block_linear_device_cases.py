"""What a device BlockLinear's tests add to `tests/block_linear_cases.py`: the
shapes that reach every extent of the benchmark's shape table (below) one at a
time, a per-block `@` restatement for them (`reference64` contracts with
`np.einsum`, which does not use BLAS), the bench's table itself, and helpers for
the plan test and for a GPU test to come.  Plain numpy; no GPU, no torch."""
import numpy as np

from tests import block_linear_cases as cases
from tests.block_linear_cases import (  # noqa: F401
    CHAIN, EXACT, GOLDEN, GRAD_ROWS, GRAD_TILE, LEADING, MAX_ROW_BLOCKS, REAL, SKINNY_ROWS, STRIDED, SWEEP, TILE_K,
    TILE_N, TILED_ROWS, bars, bf16_round, exact_inputs, inputs_of, ratio, reference64)

# csrc/block_linear.h, beside the constants the old table already names: the
# tiled kernel's columns per workgroup, and the row splits of dW
TILED_COLS, GRAD_SPLIT_ROWS, GRAD_MAX_SPLITS, WORKSPACE_MAX_MULTIPLE = 64, 256, 8, 9
OUT, DX, DW, DBIAS = 1, 2, 4, 8                     # EMB_BLOCK_LINEAR_*
ALL = OUT | DX | DW | DBIAS

# The benchmark's shape table.  (g, I, O): `dynhid` and `dyngru` block shapes at
# size1m, deter 512 / hidden 64 / 8 blocks, and size12m's dynhid0, deter 2048 /
# hidden 256: I = 2048 / 8 + 3 * 256, O = 2048 / 8 (tools/count_params.py).  Each at
# the scan's 16 rows, at 1024 and at 16 384.  (8, 256, 768) at 16 384 rows is the
# shape at which two benchmarks met a device memory fault whose cause was not found
# (DESIGN.md); no benchmark tool and no kernel is in the tree, the plan test reads
# the table from here.
BENCH_BLOCKS = ((8, 256, 64), (8, 256, 192), (8, 256, 768), (8, 1024, 256))
BENCH_ROWS = (16, 1024, 16384)
BENCH = tuple((g, i, o, rows) for (g, i, o) in BENCH_BLOCKS for rows in BENCH_ROWS)

# (g, I, O, rows, exact): the extents of the bench table no earlier test reached,
# one at a time at the smallest cost.  `exact`: integer inputs whose every partial
# sum stays below 2^24 (|x| <= 4, |w| <= 4, |gout| <= 3: 16 K forward, 12 K for dx,
# 12 rows for dW), compared bit for bit; otherwise `inputs_of` and the bars.
REACH = (
    # the bench's O = 768 with g = 8 (12 column workgroups of the tiled kernel, 48 of
    # the skinny one), one row past the skinny / tiled switch
    (8, 40, 768, 33, True),
    # the bench's block shape itself: three row tiles with a tail, K = 256 forward and
    # 768 for dx, two row splits of dW (257 > GRAD_SPLIT_ROWS) and their sum
    (8, 256, 768, 257, True),
    # one row past the bench's 16 384 rows: 129 row tiles, the dW row walk at the
    # cap of GRAD_MAX_SPLITS splits (65 steps of 32 rows each) and the sum of 8
    (3, 40, 24, 16385, True),
    # the first row count at which the splits reach their cap, not a multiple of anything
    (1, 8, 8, GRAD_SPLIT_ROWS * (GRAD_MAX_SPLITS - 1) + 1, True),
    # the larger bench block's K = 1024 (32 K steps; 8 per wave in the skinny kernel)
    (8, 1024, 256, 16, True),
)


def reference64_blocks(x, kernel, bias=None, gout=None):
  """`cases.reference64` with one `@` per block (BLAS) in place of `np.einsum`:
  the same dict.  `test_block_linear_plan_host.py` holds the two equal."""
  w = np.asarray(kernel, np.float64)
  g, i, o = w.shape
  x = np.asarray(x, np.float64).reshape(-1, g, i)
  rows = x.shape[0]
  blocks = lambda f: np.stack([f(k) for k in range(g)], 1)                     # (rows, g, n)
  product = blocks(lambda k: x[:, k] @ w[k])
  result = {'out_abs': blocks(lambda k: np.abs(x[:, k]) @ np.abs(w[k])).reshape(rows, g * o),
            'product': product.reshape(rows, g * o)}
  out = product if bias is None else product + np.asarray(bias, np.float64).reshape(g, o)
  result['out'] = out.reshape(rows, g * o)
  if gout is None:
    return result
  dy = np.asarray(gout, np.float64).reshape(rows, g, o)
  result.update(
      dx=blocks(lambda k: dy[:, k] @ w[k].T).reshape(rows, g * i),
      dx_abs=blocks(lambda k: np.abs(dy[:, k]) @ np.abs(w[k]).T).reshape(rows, g * i),
      dw=np.stack([x[:, k].T @ dy[:, k] for k in range(g)]),
      dw_abs=np.stack([np.abs(x[:, k]).T @ np.abs(dy[:, k]) for k in range(g)]),
      dbias=dy.sum(0).reshape(-1), dbias_abs=np.abs(dy).sum(0).reshape(-1))
  return result


def exact_outputs_blocks(inp):
  """`cases.exact_outputs` with one `@` per block; int64 throughout."""
  g, i, o = inp['kernel'].shape
  x, dy, w = inp['x'].reshape(-1, g, i), inp['gout'].reshape(-1, g, o), inp['kernel']
  rows = x.shape[0]
  return {'out': (np.stack([x[:, k] @ w[k] for k in range(g)], 1) + inp['bias'].reshape(g, o)).reshape(rows, g * o),
          'dx': np.stack([dy[:, k] @ w[k].T for k in range(g)], 1).reshape(rows, g * i),
          'dw': np.stack([x[:, k].T @ dy[:, k] for k in range(g)]), 'dbias': dy.sum(0).reshape(-1)}


def exact_bound(g, i, o, rows):
  """The largest magnitude any partial sum of the exact-integer case can reach."""
  return max(4 * 4 * i + 6, 3 * 4 * o, 4 * 3 * rows)


def plan_cases():
  """Every (g, I, O, rows) the plan test walks."""
  g, i, o, lead = LEADING
  table = list(SWEEP) + [REAL, STRIDED, (g, i, o, int(np.prod(lead)))] + list(EXACT)
  table += [c[:4] for c in REACH] + list(BENCH)
  return tuple(dict.fromkeys(table))
