"""`emb_block_linear_plan` (csrc/block_linear.h): the one function a BlockLinear's
launchers are to size everything with, held on the CPU over every shape of the
case tables and the benchmark's shape table -- grids inside HIP's limits, every
row, column and K step covered, the dW workspace bounded -- and its refusals, one
by one.  There are no kernels yet: nothing is launched; runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import block_linear_device_cases as dev

_CASES = dev.plan_cases()


def _lib():
  from embodied_amd import _lib
  return _lib


def _plan(g, i, o, rows, outputs=dev.ALL):
  lib = _lib()
  plan = lib.BlockLinearPlan()
  assert lib.lib.emb_block_linear_plan(C.c_int64(rows), C.c_int64(g), C.c_int64(i), C.c_int64(o), C.c_int32(outputs),
                                       C.byref(plan)) == 0, lib.lib.emb_last_error()
  return plan


def test_the_table_reaches_the_bench_and_the_caps():
  assert set(dev.BENCH) <= set(_CASES) and dev.STRIDED in _CASES
  assert (8, 256, 768, 16384) in dev.BENCH and len(dev.BENCH) == 12
  assert {c[3] for c in dev.BENCH} == {16, 1024, 16384}
  reach = {c[:4] for c in dev.REACH}
  assert {(8, 40, 768, 33), (8, 256, 768, 257), (3, 40, 24, 16385)} <= reach
  assert any(r > dev.GRAD_SPLIT_ROWS * (dev.GRAD_MAX_SPLITS - 1) for (_, _, _, r) in reach)      # the split cap
  for g, i, o, rows, exact in dev.REACH:
    assert not exact or dev.exact_bound(g, i, o, rows) < 2 ** 24


@pytest.mark.parametrize('case', _CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_plan_covers_the_shape_inside_hips_limits(case):
  g, i, o, rows = case
  plan = _plan(g, i, o, rows)
  for launch, (k_len, n_len) in ((plan.forward, (i, o)), (plan.grad_x, (o, i))):
    assert 1 <= launch.grid_x <= 2 ** 31 - 1 and 1 <= launch.grid_y <= 65535 and 1 <= launch.grid_z <= 65535
    assert launch.block == 256 <= 1024
    assert launch.grid_y == g
    assert launch.passes * launch.grid_z * launch.row_tile >= rows                    # every row
    assert (launch.passes - 1) * launch.grid_z * launch.row_tile < rows               # and no idle pass
    assert launch.grid_x == launch.col_tiles and launch.col_tiles * launch.col_tile >= n_len
    assert (launch.col_tiles - 1) * launch.col_tile < n_len
    assert launch.k_steps * launch.k_tile >= k_len
    skinny = rows <= dev.SKINNY_ROWS                                                  # the switch the table was drawn for
    assert launch.row_tile == (dev.SKINNY_ROWS if skinny else dev.TILED_ROWS)
    assert launch.col_tile == (dev.TILE_N if skinny else dev.TILED_COLS)
    assert launch.grid_z <= dev.MAX_ROW_BLOCKS and (not skinny or (launch.grid_z, launch.passes) == (1, 1))
  launch = plan.grad_w
  assert 1 <= launch.grid_x <= 2 ** 31 - 1 and launch.grid_y == g <= 65535 and 1 <= launch.grid_z <= 65535
  assert launch.block == 256
  assert launch.grid_z == plan.splits and 1 <= plan.splits <= dev.GRAD_MAX_SPLITS
  assert launch.row_tile == dev.GRAD_ROWS and plan.split_rows == launch.passes * launch.row_tile
  assert plan.splits * plan.split_rows >= rows and (plan.splits - 1) * plan.split_rows < rows
  assert launch.col_tile == launch.k_tile == dev.GRAD_TILE
  assert launch.col_tiles * launch.col_tile >= o and launch.k_steps * launch.k_tile >= i
  assert launch.grid_x == launch.col_tiles * launch.k_steps
  assert plan.launches_grad_w == (2 if plan.splits > 1 else 1)
  dw_bytes, db_bytes = g * i * o * 4, g * o * 4
  assert plan.workspace_max_multiple == dev.WORKSPACE_MAX_MULTIPLE
  if plan.splits > 1:
    assert plan.workspace_bytes >= plan.splits * (dw_bytes + db_bytes)
    assert 1 <= plan.sum_grid_x <= 2 ** 31 - 1
  assert plan.workspace_bytes <= plan.workspace_max_multiple * dw_bytes
  # no buffer of an accepted shape holds more than 2^31 - 1 elements (the rule block_linear.h states)
  assert max(rows * g * i, rows * g * o, g * i * o, plan.workspace_bytes // 4) <= 2 ** 31 - 1


def test_plan_sizes_only_what_is_asked_for():
  g, i, o, rows = 8, 256, 768, 16384
  only_out = _plan(g, i, o, rows, dev.OUT)
  assert only_out.forward.block and not only_out.grad_x.block and not only_out.grad_w.block
  assert only_out.workspace_bytes == 0 and only_out.splits == 0
  only_bias = _plan(g, i, o, rows, dev.DBIAS)
  assert only_bias.grad_w.k_steps == 1 and only_bias.workspace_bytes == only_bias.splits * g * o * 4
  only_dw = _plan(g, i, o, rows, dev.DW)
  assert only_dw.workspace_bytes == only_dw.splits * g * i * o * 4
  assert _plan(g, i, o, 0).forward.block == 0                                           # no rows: nothing


def test_every_refusal_is_a_status():
  """A null plan, a bad mask, negative rows, g, I or O below 1 (a width that is no
  whole number of blocks never reaches the ABI: it takes g, I, O), I or O no
  multiple of 8, and a buffer past 2^31 - 1 elements, each alone."""
  lib = _lib()
  raw = lib.lib
  raw.emb_block_linear_plan.argtypes = lib.SIGNATURES['emb_block_linear_plan']
  invalid = lib.ERR_INVALID

  def status(*args):
    code = raw.emb_block_linear_plan(*args)
    return code, (raw.emb_last_error() or b'').decode()

  plan = lib.BlockLinearPlan()
  code, msg = status(16, 8, 256, 64, dev.ALL, None)
  assert code == invalid and 'null' in msg
  for mask in (-1, 16):
    code, msg = status(16, 8, 256, 64, mask, C.byref(plan))
    assert code == invalid and 'mask' in msg
  for (rows, g, i, o), word in (((-1, 8, 256, 64), 'negative'), ((16, 0, 256, 64), 'at least 1'),
                                ((16, 8, 0, 64), 'at least 1'), ((16, 65536, 8, 8), '65535'),
                                ((16, 4, 11, 8), 'multiples of 8'), ((16, 4, 8, 2), 'multiples of 8'),
                                ((2 ** 20, 8, 256, 768), '2^31 - 1 elements of x or out'),       # x: 2^31 exactly
                                ((16, 8, 16384, 16384), '2^31 - 1 elements of W'),               # W: 2^31 exactly
                                ((16, 8, 4096, 8192), 'workspace'),                              # W fits, 8 copies do not
                                ((2 ** 40, 1, 8, 8), '2^31 - 1')):
    code, msg = status(rows, g, i, o, dev.ALL, C.byref(plan))
    assert code == invalid and word in msg, ((rows, g, i, o), code, msg)
  # the workspace bound holds only where dW or dbias is asked for
  assert status(16, 8, 4096, 8192, dev.OUT | dev.DX, C.byref(plan))[0] == 0
  assert plan.workspace_bytes == 0 and plan.forward.block and plan.grad_x.block and not plan.grad_w.block
  for mask in (dev.DW, dev.DBIAS):
    assert status(16, 8, 4096, 8192, mask, C.byref(plan))[0] == invalid
  # the largest shapes just inside: x of 2^31 - 2^11 elements
  assert status(2 ** 20 - 1, 8, 256, 256, dev.ALL, C.byref(plan))[0] == 0
  assert status(0, 8, 256, 64, dev.ALL, C.byref(plan))[0] == 0 and plan.forward.block == 0        # no rows: fine


def test_block_restatement_equals_reference64():
  g, i, o, rows = 3, 40, 24, 17
  inp = dev.inputs_of(g, i, o, rows, np.random.default_rng(7))
  want = dev.reference64(inp['x'], inp['kernel'], inp['bias'], inp['gout'])
  got = dev.reference64_blocks(inp['x'], inp['kernel'], inp['bias'], inp['gout'])
  assert sorted(got) == sorted(want)
  for key in want:
    assert got[key].shape == want[key].shape
    assert np.allclose(got[key], want[key], rtol=1e-13, atol=1e-13), key
  exact = dev.exact_inputs(g, i, o, rows)
  from tests.block_linear_cases import exact_outputs
  for key, value in exact_outputs(exact).items():
    assert np.array_equal(dev.exact_outputs_blocks(exact)[key], value), key
