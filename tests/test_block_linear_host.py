"""BlockLinear (embodied/jax/nets.py:254-278) as far as it goes without a GPU:
the fixture from the reference's own method, the float64 restatement with its
three gradients, and the case table a device kernel is to be tested with.  CPU only."""
import pathlib

import numpy as np
import pytest

from tests import block_linear_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'block_linear.npz'


def _central(f, x, gout, step=1e-6):
  """d sum(f(x) * gout) / dx by central differences in float64."""
  grad = np.zeros_like(x)
  flat, out = x.reshape(-1), grad.reshape(-1)
  for i in range(flat.size):
    keep = flat[i]
    flat[i] = keep + step
    hi = (f(x) * gout).sum()
    flat[i] = keep - step
    lo = (f(x) * gout).sum()
    flat[i] = keep
    out[i] = (hi - lo) / (2 * step)
  return grad


def test_fixture_is_current():
  from oracle import refload
  if not (refload.REFERENCE / 'embodied' / 'jax' / 'nets.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_block_linear', ROOT / 'tools' / 'gen_block_linear_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key


def test_restatement_equals_the_fixture():
  """`reference64` agrees with the reference's own float64 run of
  `BlockLinear.__call__` on every case; its float32 run differs by float32
  accumulation only."""
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_BlockLinear']) == (254, 281)
    for case, (g, i, o, lead, bias) in enumerate(cases.GOLDEN):
      name, inp = cases.tag(case), cases.inputs(case)
      assert np.array_equal(f[f'in_{name}'], cases.digest(cases.present(inp))), name
      want, got32 = f[f'out64_{name}'], f[f'out_{name}']
      assert want.dtype == np.float64 and got32.dtype == np.float32 and want.shape == (*lead, g * o)
      ref = cases.reference64(inp['x'].reshape(-1, g * i), inp['kernel'], inp['bias'])
      assert np.allclose(ref['out'].reshape(want.shape), want, rtol=1e-13, atol=1e-13), name
      bar = cases.bar_f32(ref['out'], ref['out_abs'] + (0 if inp['bias'] is None else np.abs(inp['bias'])), i + 1)
      assert (np.abs(got32.reshape(ref['out'].shape) - ref['out']) <= bar).all(), name


def test_block_linear_gradients_agree_with_central_differences():
  g, i, o, rows = 3, 4, 5, 2
  rng = np.random.default_rng(5)
  x, w = rng.standard_normal((rows, g * i)), rng.standard_normal((g, i, o))
  b, gout = rng.standard_normal(g * o), rng.standard_normal((rows, g * o))
  ref = cases.reference64(x, w, b, gout)
  assert np.allclose(ref['dx'], _central(lambda v: cases.reference64(v, w, b)['out'], x, gout), rtol=1e-6, atol=1e-8)
  assert np.allclose(ref['dw'], _central(lambda v: cases.reference64(x, v, b)['out'], w, gout), rtol=1e-6, atol=1e-8)
  assert np.allclose(ref['dbias'], _central(lambda v: cases.reference64(x, w, v)['out'], b, gout), rtol=1e-6, atol=1e-8)
  # the indexing of nets.py:273-275, element by element
  for k in range(g):
    for j in range(o):
      assert np.isclose(ref['out'][1, k * o + j], x[1, k * i:(k + 1) * i] @ w[k, :, j] + b[k * o + j], rtol=1e-13)
  exact = cases.exact_inputs(3, 8, 16, 5)
  w = exact['kernel']
  assert len({tuple(w[k].ravel()) for k in range(3)}) == 3                       # depends on k
  assert not np.array_equal(w[:, :8, :8], w[:, :8, :8].transpose(0, 2, 1))       # asymmetric in (i, o)


def test_case_table_covers_what_it_was_chosen_for():
  sweep = cases.SWEEP
  assert {c[0] for c in sweep} == {1, 3, 8}
  assert {c[1] for c in sweep} == {8, 40, 64, 264} and {c[2] for c in sweep} == {8, 24, 64, 136}
  assert {c[3] for c in sweep} >= {1, 15, 16, 17, 33, 130}
  assert {(c[1], c[2]) for c in sweep} == {(i, o) for i in cases.I for o in cases.O}        # every pair
  rows = {c[3] for c in sweep}
  assert cases.SKINNY_ROWS in rows and cases.SKINNY_ROWS + 1 in rows                         # the switch, both sides
  assert any(r % 16 for r in rows) and any(r > cases.TILED_ROWS and r % cases.TILED_ROWS for r in rows)
  assert any(i % cases.TILE_K for i in cases.I) and any(i > cases.TILE_K for i in cases.I)    # K tail, several K steps
  assert any(o % cases.TILE_N for o in cases.O) and any(o > 4 * cases.TILE_N for o in cases.O)
  assert any(c[3] > cases.GRAD_ROWS and c[1] > cases.GRAD_TILE and c[2] > cases.GRAD_TILE for c in sweep)
  for tiled in (False, True):                       # each kernel meets a K tail, a column tail and g > 1
    mine = [c for c in sweep if (c[3] > cases.SKINNY_ROWS) == tiled]
    assert any(c[1] % cases.TILE_K and c[2] % cases.TILE_N and c[0] > 1 for c in mine)
  g, i, o, many = cases.STRIDED
  assert many > cases.TILED_ROWS * cases.MAX_ROW_BLOCKS and i == o == 8
  assert cases.REAL == (8, 256, 64, 16) and cases.LEADING[3] == (2, 3) and cases.CHAIN == (16, 512, 64, 8)
  for inp in (cases.exact_inputs(8, 264, 136, 130),):                            # every partial sum below 2^24
    g, i, o = inp['kernel'].shape
    big = max(np.abs(inp['x']).max() * np.abs(inp['kernel']).max() * i + np.abs(inp['bias']).max(),
              np.abs(inp['gout']).max() * np.abs(inp['kernel']).max() * o,
              np.abs(inp['x']).max() * np.abs(inp['gout']).max() * 130)
    assert big < 2 ** 24
