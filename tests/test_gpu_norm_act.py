"""`embodied_amd.nets.norm_act` / `NormAct` on the GPU, kernels and composed torch
ops, against the float64 restatement of tests/norm_act_cases.py (the host test
holds it against the reference's own float64 run and central differences) and
the bars of tests/test_gpu_policy_loss.py."""
import numpy as np
import pytest
import torch

from tests import norm_act_cases as norms

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize('kind', ['f32', 'bf16'])


def _nets():
  from embodied_amd import nets
  return nets


def _dev(array, kind='f32'):
  if array is None:
    return None
  return torch.from_numpy(np.ascontiguousarray(array)).cuda().to(torch.float32 if kind == 'f32' else torch.bfloat16)


def _host(tensor):
  return tensor.detach().float().cpu().numpy()


def _run_norm(inp, impl, act, eps, kind, fused, grads=True):
  """(out, dx, dscale, dshift) as numpy through nets.norm_act."""
  nets = _nets()
  x = _dev(inp['x'], kind).requires_grad_(grads)
  scale = None if inp['scale'] is None else _dev(inp['scale']).requires_grad_(grads)
  shift = None if inp['shift'] is None else _dev(inp['shift']).requires_grad_(grads)
  out = nets.norm_act(x, scale, shift, impl, act, eps, fused=fused)
  assert out.dtype == x.dtype and out.shape == x.shape
  if not grads:
    return _host(out), None, None, None
  out.backward(_dev(inp['gout'], kind))
  return (_host(out), _host(x.grad), None if scale is None else _host(scale.grad),
          None if shift is None else _host(shift.grad))


def _rounded(inp, kind):
  if kind == 'f32':
    return inp
  return {k: (norms.bf16_round(v) if k in ('x', 'gout') else v) for k, v in inp.items()}


def _check_norm(inp, impl, act, eps, kind, fused, sums):
  inp = _rounded(inp, kind)
  want = norms.reference64(inp['x'], inp['scale'], inp['shift'], impl, act, eps, inp['gout'])
  out, dx, dscale, dshift = _run_norm(inp, impl, act, eps, kind, fused)
  bf16 = kind == 'bf16'
  s = norms.row_scale(inp['gout'], inp['scale'], want['rstd'])
  ratios = {'out': norms.out_ratio(out, want['out'], bf16), 'dx': norms.grad_ratio(dx, want['dx'], s, bf16)}
  if sums and dscale is not None:
    ratios['dscale'] = norms.sum_ratio(dscale, want['dscale'], want['dscale_abs'])
  if sums and dshift is not None:
    ratios['dshift'] = norms.sum_ratio(dshift, want['dshift'], want['dshift_abs'])
  print(impl, act, eps, kind, inp['x'].shape, 'fused' if fused else 'composed', ratios)
  assert max(ratios.values()) <= 1.0, ratios


FUSED_UNITS = [u for u in norms.UNITS if u <= norms.MAX_UNITS]


@pytest.mark.parametrize('units', FUSED_UNITS)
@DTYPES
def test_norm_act_widths(units, kind):
  """Every width at rows 1 and 3 on the kernels, impl and activation in turn."""
  for i, rows in enumerate(norms.ROWS):
    impl = norms.IMPLS[(units + i) % 2]
    act = norms.ACTS[(units // 2 + i) % 4]
    rng = np.random.default_rng([units, rows])
    inp = norms.inputs_of(rows, units, impl, True, 1.0, rng)
    _check_norm(inp, impl, act, 1e-4, kind, True, sums=False)


@pytest.mark.parametrize('rows,units', norms.RAGGED)
@pytest.mark.parametrize('impl', norms.IMPLS)
def test_norm_act_ragged_rows_and_column_sums(rows, units, impl):
  for act in norms.ACTS:
    for kind in ('f32', 'bf16'):
      inp = norms.inputs_of(rows, units, impl, True, 1.0, np.random.default_rng([rows, units]))
      _check_norm(inp, impl, act, 1e-4, kind, True, sums=rows >= norms.SUM_ROWS)


@pytest.mark.parametrize('rows,units', norms.LADDER)
def test_norm_act_column_sums_on_every_step_of_the_width_ladder(rows, units):
  """dscale and dshift (and out, dx) at every kernel of the ladder: the waves'
  meeting in LDS with a ragged last workgroup, the partial sums a workgroup keeps
  in memory over more than one row, the streamed gradient past 8192 units."""
  step = norms.LADDER.index((rows, units))
  impl, act = norms.IMPLS[step % 2], norms.ACTS[(step // 2 + step) % 4]
  inp = norms.inputs_of(rows, units, impl, True, 1.0, np.random.default_rng([rows, units]))
  _check_norm(inp, impl, act, 1e-4, 'f32', True, sums=True)
  other = norms.IMPLS[(step + 1) % 2]
  inp = norms.inputs_of(rows, units, other, True, 1.0, np.random.default_rng([units, rows]))
  _check_norm(inp, other, norms.ACTS[(step + 2) % 4], 1e-4, 'bf16', True, sums=True)


@pytest.mark.parametrize('impl', norms.IMPLS)
@pytest.mark.parametrize('act', norms.ACTS)
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_norm_act_options(impl, act, fused):
  """scale / shift given and null, both eps, the three input scales; float32 on
  both paths, bfloat16 on the kernels (the composed path rounds between norm and
  activation as the reference does: the documented difference)."""
  for affine in (True, False):
    for eps in norms.EPS:
      for scale in norms.SCALES:
        for kind in ('f32', 'bf16') if fused else ('f32',):
          inp = norms.inputs_of(norms.SUM_ROWS, 65, impl, affine, scale, np.random.default_rng([int(eps * 1e7), affine]))
          _check_norm(inp, impl, act, eps, kind, fused, sums=True)


def test_norm_act_zero_row_nan_row_views_and_leading_shape():
  nets = _nets()
  rng = np.random.default_rng(3)
  for impl in norms.IMPLS:
    inp = norms.inputs_of(3, 65, impl, True, 1.0, rng)
    clean, clean_dx, _, _ = _run_norm(inp, impl, 'silu', 1e-4, 'f32', True)
    zero = dict(inp, x=inp['x'].copy())
    zero['x'][1] = 0
    want = norms.reference64(zero['x'], zero['scale'], zero['shift'], impl, 'silu', 1e-4)
    out, dx, _, _ = _run_norm(zero, impl, 'silu', 1e-4, 'f32', True)
    assert norms.out_ratio(out, want['out']) <= 1.0 and np.isfinite(dx).all()      # layer: the tie, forward only
    for poison in (np.nan, np.inf):
      bad = dict(inp, x=inp['x'].copy())
      bad['x'][1, 7] = poison
      out, dx, dscale, _ = _run_norm(bad, impl, 'silu', 1e-4, 'f32', True)
      assert np.isnan(out[1]).all() and np.isnan(dx[1]).all()
      assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(dx[[0, 2]], clean_dx[[0, 2]])
      assert np.isnan(dscale).any()                                # the column sums see it
  # a non-contiguous view and a leading shape (2, 3, units)
  inp = norms.inputs_of(6, 65, 'rms', True, 1.0, rng)
  want = norms.reference64(inp['x'], inp['scale'], None, 'rms', 'gelu', 1e-4)['out']
  wide = torch.zeros(6, 130, device='cuda')
  wide[:, ::2] = _dev(inp['x'])
  view = wide[:, ::2]
  assert not view.is_contiguous()
  assert norms.out_ratio(_host(nets.norm_act(view, _dev(inp['scale']), None, 'rms', 'gelu', fused=True)), want) <= 1.0
  lead = nets.norm_act(_dev(inp['x']).view(2, 3, 65), _dev(inp['scale']), None, 'rms', 'gelu', fused=True)
  assert lead.shape == (2, 3, 65) and norms.out_ratio(_host(lead).reshape(6, 65), want) <= 1.0


def test_norm_act_launch_counts_and_determinism():
  nets = _nets()
  module = nets.NormAct(1025, 'layer1em6', 'silu', fused=True)
  assert module.eps == 1e-6 and module.impl == 'layer' and module.scale.dtype == torch.float32
  assert nets.NormAct(8, 'rms').shift is None
  x = torch.randn(37, 1025, device='cuda', requires_grad=True)
  gout = torch.randn(37, 1025, device='cuda')
  before = nets.norm_act_launches()
  out = module(x)
  assert nets.norm_act_launches() == before + 1
  out.backward(gout)
  assert nets.norm_act_launches() == before + 3                    # dx and the partial sums, then their sum
  first = module.scale.grad.clone()
  module.scale.grad = None
  module(x).backward(gout)
  assert torch.equal(module.scale.grad, first)                     # bit-identical run to run
  before = nets.norm_act_launches()
  nets.norm_act(x, None, None, 'rms', 'silu', fused=True).backward(gout)
  assert nets.norm_act_launches() == before + 2                    # no parameter gradients: one launch backward
  nets.norm_act(x, None, None, 'rms', 'silu', fused=False).backward(gout)
  assert nets.norm_act_launches() == before + 2                    # composed: none


def test_norm_act_refusals_and_the_composed_path_past_the_limit():
  nets = _nets()
  x = torch.randn(2, norms.MAX_UNITS + 1, device='cuda')
  with pytest.raises(ValueError, match=str(norms.MAX_UNITS)):
    nets.norm_act(x, fused=True)
  for units in (norms.MAX_UNITS + 1, 20000):
    inp = norms.inputs_of(2, units, 'rms', False, 1.0, np.random.default_rng(units))
    want = norms.reference64(inp['x'], None, None, 'rms', 'silu', 1e-4)['out']
    before = nets.norm_act_launches()
    assert norms.out_ratio(_host(nets.norm_act(_dev(inp['x']))), want) <= 1.0          # fused=None composes it
    assert nets.norm_act_launches() == before
  with pytest.raises(TypeError):
    nets.norm_act(torch.zeros(2, 8, device='cuda', dtype=torch.float16))
  with pytest.raises(ValueError, match='shape'):
    nets.norm_act(torch.zeros(2, 8, device='cuda'), torch.ones(7, device='cuda'))
  with pytest.raises(TypeError):
    nets.norm_act(torch.zeros(2, 8, device='cuda'), torch.ones(8, device='cuda', dtype=torch.bfloat16))
