"""`embodied_amd.nets.pool_norm_act` / `norm_act_upsample` on the GPU, kernels and
composed torch ops, against the float64 restatement of tests/conv_stage_cases.py
(the host test holds it against the reference's own float64 run, central
differences and a hand-written tie) and the bars of tests/norm_act_cases.py."""
import pathlib

import numpy as np
import pytest
import torch

from tests import conv_stage_cases as stages
from tests import norm_act_cases as norms

pytestmark = pytest.mark.gpu

STAGES = pytest.mark.parametrize('stage', stages.STAGES)
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'conv_stage.npz'


def _nets():
  from embodied_amd import nets
  return nets


def _call(stage):
  return _nets().pool_norm_act if stage == 'pool' else _nets().norm_act_upsample


def _dev(array, kind='f32'):
  if array is None:
    return None
  return torch.from_numpy(np.ascontiguousarray(array)).cuda().to(torch.float32 if kind == 'f32' else torch.bfloat16)


def _host(tensor):
  return None if tensor is None else tensor.detach().float().cpu().numpy()


def _run(stage, inp, impl, act, eps, kind, fused, grads=True):
  """(out, dx, dscale, dshift) as numpy through the facade."""
  x = _dev(inp['x'], kind).requires_grad_(grads)
  scale = None if inp['scale'] is None else _dev(inp['scale']).requires_grad_(grads)
  shift = None if inp['shift'] is None else _dev(inp['shift']).requires_grad_(grads)
  out = _call(stage)(x, scale, shift, impl, act, eps, fused=fused)
  assert out.dtype == x.dtype and tuple(out.shape) == stages.out_shape(stage, x.shape)
  if not grads:
    return _host(out), None, None, None
  out.backward(_dev(inp['gout'], kind))
  return (_host(out), _host(x.grad), None if scale is None else _host(scale.grad),
          None if shift is None else _host(shift.grad))


def _rounded(inp, kind):
  if kind == 'f32':
    return inp
  return {k: (norms.bf16_round(v) if k in ('x', 'gout') else v) for k, v in inp.items()}


def _check(stage, inp, impl, act, eps, kind, fused, sums):
  inp = _rounded(inp, kind)
  want = stages.reference(stage, inp['x'], inp['scale'], inp['shift'], impl, act, eps, inp['gout'])
  out, dx, dscale, dshift = _run(stage, inp, impl, act, eps, kind, fused)
  found = stages.ratios(stage, want, out, dx, dscale, dshift, kind == 'bf16', sums)
  print(stage, impl, act, eps, kind, inp['x'].shape, 'fused' if fused else 'composed', found)
  assert max(found.values()) <= 1.0, found
  return out, dx


@STAGES
@pytest.mark.parametrize('units', stages.UNITS)
def test_conv_stage_widths(stage, units):
  """Every width at both image shapes and both dtypes on the kernels, impl and activation in turn."""
  for i, (images, height, width) in enumerate(stages.SHAPES):
    for k, kind in enumerate(('f32', 'bf16')):
      impl = stages.IMPLS[(units + i + k) % 2]
      act = stages.ACTS[(units // 2 + i + 2 * k) % 4]
      inp = stages.inputs_of(stage, images, height, width, units, impl, True, 1.0, np.random.default_rng([units, i]))
      _check(stage, inp, impl, act, 1e-4, kind, True, sums=False)


@STAGES
@pytest.mark.parametrize('height,width', [(2, 6), (6, 2), (2, 10), (4, 6), (2, 22), (6, 14)])
def test_conv_stage_ragged_packing(stage, height, width):
  """At 8 channels a wave packs 8 pixels and a workgroup 32: image rows of 3, 5,
  7 and 11 pooled pixels end inside a wave, 5 images of (6, 14) put image and
  image-row boundaries inside a workgroup and leave a ragged last one; (2, 6)
  against (6, 2) catches a swapped stride."""
  for units, kind in ((8, 'f32'), (8, 'bf16'), (24, 'bf16'), (72, 'f32')):
    images = 5 if stage == 'pool' else 3
    rng = np.random.default_rng([height, width, units])
    inp = stages.inputs_of(stage, images, height, width, units, 'rms', True, 1.0, rng)
    _check(stage, inp, 'rms', 'silu', 1e-4, kind, True, sums=False)


# (images, H, W, C) of x: at 3 channels a workgroup takes 32 pixels, so a forward
# launch covers 2048 * 32 = 65 536 pixels in one pass and a gradient launch
# 1024 * 32 = 32 768.  The pool of (1, 528, 528, 3) has 69 696 pixels: a second
# pass forward, a third backward; so has the upsample of (1, 264, 264, 3).
PAST_THE_GRID = {'pool': (1, 528, 528, 3), 'upsample': (1, 264, 264, 3)}


@STAGES
def test_conv_stage_grid_stride_and_column_sums(stage):
  images, height, width, units = PAST_THE_GRID[stage]
  pixels = images * height * width // (4 if stage == 'pool' else 1)
  per = 256 // stages.lanes(units)
  assert pixels > stages.MAX_BLOCKS * per and pixels > 2 * stages.MAX_PARTIALS * per
  for impl, kind in (('layer', 'f32'), ('rms', 'bf16')):
    inp = stages.inputs_of(stage, images, height, width, units, impl, True, 1.0, np.random.default_rng(pixels))
    _check(stage, inp, impl, 'gelu', 1e-4, kind, True, sums=True)


# one case per step of the lanes ladder with at least SUM_ROWS Norm rows, (Norm rows as h x w, units):
# a ragged last workgroup at every step (310 = 9 * 32 + 22 = 19 * 16 + 6 = 38 * 8 + 6 = 77 * 4 + 2)
@STAGES
@pytest.mark.parametrize('units', [3, 64, 128, 129, 256, 512, 513, 1024])
def test_conv_stage_column_sums_on_every_step_of_the_lanes_ladder(stage, units):
  step = stages.UNITS.index(units)
  height, width = (10, 62) if stage == 'pool' else (5, 31)         # 2 images: 310 Norm rows
  for k, kind in enumerate(('f32', 'bf16')):
    impl, act = stages.IMPLS[(step + k) % 2], stages.ACTS[(step + 2 * k) % 4]
    inp = stages.inputs_of(stage, 2, height, width, units, impl, True, 1.0, np.random.default_rng([units, k]))
    assert np.prod(stages.out_shape('pool', inp['x'].shape)[:3] if stage == 'pool' else inp['x'].shape[:3]) >= stages.SUM_ROWS
    _check(stage, inp, impl, act, 1e-4, kind, True, sums=True)


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_pool_ties_share_the_gradient_equally(kind):
  """Inputs that are multiples of 0.5: windows tie two, three and four ways (held
  on the CPU first); dx is g / count at the ties and exactly 0 elsewhere."""
  for units, impl in ((8, 'rms'), (65, 'rms')):
    inp = stages.inputs_of('pool', 3, 4, 6, units, impl, True, 1.0, np.random.default_rng(units), ties=True)
    inp['x'][0, 0, 0, 0], inp['x'][0, 0, 1, 0], inp['x'][0, 1, 0, 0], inp['x'][0, 1, 1, 0] = 0.0, -0.0, -0.5, -1.0
    assert np.array_equal(inp['x'], norms.bf16_round(inp['x']))    # halves: the same inputs in both dtypes
    win = stages.windows(inp['x'])
    count = (win == win.max(1, keepdims=True)).sum(1)
    assert {1, 2, 3, 4} <= set(np.unique(count)) and count[0, 0] == 2          # +0 and -0 tie
    _, dx = _check('pool', inp, impl, 'silu', 1e-4, kind, True, sums=False)
    lost = stages.windows(inp['x']) != win.max(1, keepdims=True)
    assert lost.any() and (stages.windows(dx)[lost] == 0).all()
    # the composed path splits the same way (float32: it rounds bfloat16 between norm and activation)
    if kind == 'f32':
      _, dx = _check('pool', inp, impl, 'silu', 1e-4, kind, False, sums=False)
      assert (stages.windows(dx)[lost] == 0).all()


@pytest.mark.parametrize('units,kind', [(24, 'f32'), (72, 'bf16'), (200, 'f32'), (264, 'bf16'), (520, 'f32')])
def test_pool_nan_and_infinite_windows_poison_their_pixel_alone(units, kind):
  """At every step of the lanes ladder (8, 16, 32, 64 lanes per pixel, 16 values per
  lane at 520) and in both dtypes.  A NaN at a position that is not its window's max, and a window of all -inf:
  on the kernels that pixel is NaN throughout in out and in its window of dx,
  every other pixel -- its neighbours in the same wave among them -- is
  bit-equal to the run without the poison and inside its bar."""
  bf16 = kind == 'bf16'
  inp = _rounded(stages.inputs_of('pool', 2, 4, 6, units, 'rms', True, 1.0, np.random.default_rng(11)), kind)
  clean, clean_dx, clean_scale, _ = _run('pool', inp, 'rms', 'silu', 1e-4, kind, True)
  win = stages.windows(inp['x'])                                   # (12 pixels, 4, C)
  pixel, channel = 7, units - 3
  loser = int(np.argmin(win[pixel, :, channel]))                   # a position that is not the window's max
  for what in ('nan', '-inf'):
    bad = win.copy()
    if what == 'nan':
      bad[pixel, loser, channel] = np.nan
    else:
      bad[pixel, :, channel] = -np.inf
    poisoned = dict(inp, x=stages.unwindows(bad, inp['x'].shape))
    for fused in (True, False) if kind == 'f32' else (True,):
      out, dx, dscale, _ = _run('pool', poisoned, 'rms', 'silu', 1e-4, kind, fused)
      out, dxw = out.reshape(-1, units), stages.windows(dx)
      if fused:
        assert np.isnan(out[pixel]).all() and np.isnan(dxw[pixel]).all(), what
        others = np.arange(len(out)) != pixel
        assert np.array_equal(out[others], clean.reshape(-1, units)[others])
        assert np.array_equal(dxw[others], stages.windows(clean_dx)[others])
        want = stages.reference('pool', inp['x'], inp['scale'], None, 'rms', 'silu', 1e-4, inp['gout'])
        got = {'out': np.where(others[:, None], out, want['out'].reshape(-1, units)).reshape(want['out'].shape),
               'dx': stages.unwindows(np.where(others[:, None, None], dxw, stages.windows(want['dx'])), dx.shape)}
        assert max(stages.ratios('pool', want, got['out'], got['dx'], bf16=bf16).values()) <= 1.0
        assert np.isnan(dscale).any()                              # the column sums see it
      else:                                                        # the definition: the NaN wins its window
        assert np.isnan(out[pixel, channel]) and (what != 'nan' or np.isnan(dxw[pixel, :, channel]).all()), what


def test_upsample_layout_repeats_every_pixel_and_equals_norm_act():
  """Pixels that are all distinct, so a tiled layout fails.  Each of the four
  copies is bit-equal to the others.  Against `norm_act(fused=True)`: the two
  share the row's statistics and activation code but not the order of the row
  sums (a pixel has 8 .. 64 lanes here, a row of norm_act a whole wave), so the
  value is held within the forward bar, not bit for bit."""
  nets = _nets()
  for units, kind in ((8, 'f32'), (65, 'bf16'), (192, 'bf16'), (600, 'f32')):
    inp = stages.inputs_of('upsample', 2, 3, 5, units, 'layer', True, 1.0, np.random.default_rng(units))
    inp = _rounded(inp, kind)
    x, scale, shift = _dev(inp['x'], kind), _dev(inp['scale']), _dev(inp['shift'])
    assert len(np.unique(inp['x'].reshape(-1, units), axis=0)) == 2 * 3 * 5
    out = nets.norm_act_upsample(x, scale, shift, 'layer', 'gelu', fused=True)
    row = nets.norm_act(x, scale, shift, 'layer', 'gelu', fused=True)
    assert out.shape == (2, 6, 10, units)
    for i in (0, 1):
      for j in (0, 1):
        assert torch.equal(out[:, i::2, j::2], out[:, 0::2, 0::2]), (units, i, j)
    want = norms.reference64(inp['x'].reshape(-1, units), inp['scale'], inp['shift'], 'layer', 'gelu', 1e-4)['out']
    assert norms.out_ratio(_host(out[:, 0::2, 0::2]).reshape(-1, units), want, kind == 'bf16') <= 1.0
    assert norms.out_ratio(_host(row).reshape(-1, units), want, kind == 'bf16') <= 1.0


@STAGES
def test_conv_stage_views_leading_shapes_and_zero_images(stage):
  nets, call = _nets(), _call(stage)
  images, height, width, units = 6, 4, 6, 24
  inp = stages.inputs_of(stage, images, height, width, units, 'rms', True, 1.0, np.random.default_rng(5))
  want = stages.reference(stage, inp['x'], inp['scale'], None, 'rms', 'gelu', 1e-4, inp['gout'])
  scale = _dev(inp['scale'])
  base, base_dx, _, _ = _run(stage, inp, 'rms', 'gelu', 1e-4, 'f32', True)
  # x (and gout) one element into a larger buffer: off 16-byte alignment, the element-wise kernels
  def offset(array):
    room = torch.zeros(array.size + 5, device='cuda')
    view = room[1:1 + array.size].view(array.shape)
    view.copy_(_dev(array))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view
  x = offset(inp['x']).requires_grad_()
  out = call(x, scale, None, 'rms', 'gelu', fused=True)
  out.backward(offset(inp['gout']))
  assert np.array_equal(_host(out), base) and np.array_equal(_host(x.grad), base_dx)
  # a channels-first tensor, permuted to channels last: not contiguous, copied
  first = _dev(inp['x'].transpose(0, 3, 1, 2)).requires_grad_()
  view = first.permute(0, 2, 3, 1)
  assert not view.is_contiguous()
  out = call(view, scale, None, 'rms', 'gelu', fused=True)
  out.backward(_dev(inp['gout']))
  assert np.array_equal(_host(out), base) and np.array_equal(_host(first.grad).transpose(0, 2, 3, 1), base_dx)
  # a leading shape (B, T, H, W, C)
  lead = call(_dev(inp['x']).view(2, 3, height, width, units), scale, None, 'rms', 'gelu', fused=True)
  assert lead.shape == (2, 3, *base.shape[1:]) and np.array_equal(_host(lead).reshape(base.shape), base)
  assert max(stages.ratios(stage, want, base, base_dx).values()) <= 1.0
  # no images: the composed path, nothing is launched
  before = nets.conv_stage_launches()
  for fused in (None, True):
    empty = call(torch.zeros(0, height, width, units, device='cuda', requires_grad=True), scale, fused=fused)
    assert empty.shape == (0, *base.shape[1:])
    empty.sum().backward()
  empty = call(torch.zeros(2, 0, height, width, units, device='cuda'), scale)
  assert empty.shape == (2, 0, *base.shape[1:]) and nets.conv_stage_launches() == before
  if stage == 'pool':
    for bad in ((2, 3, 4, 8), (2, 4, 5, 8)):
      with pytest.raises(ValueError, match='even'):
        call(torch.zeros(*bad, device='cuda'))


@STAGES
@pytest.mark.parametrize('impl', stages.IMPLS)
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_conv_stage_options(stage, impl, fused):
  """scale / shift given and null, both eps, the three input scales, the
  activations in turn; float32 on both paths, bfloat16 on the kernels (the
  composed path rounds between norm and activation as the reference does: the
  difference `norm_act` documents)."""
  turn = 0
  for affine in (True, False):
    for eps in stages.EPS:
      for scale in stages.SCALES:
        for kind in ('f32', 'bf16') if fused else ('f32',):
          act = stages.ACTS[turn % 4]
          turn += 1
          height, width = (10, 62) if stage == 'pool' else (5, 31)
          rng = np.random.default_rng([int(eps * 1e7), affine, turn])
          inp = stages.inputs_of(stage, 2, height, width, 65, impl, affine, scale, rng)
          _check(stage, inp, impl, act, eps, kind, fused, sums=True)


@STAGES
def test_conv_stage_launch_counts_determinism_and_modules(stage):
  nets = _nets()
  Module = nets.PoolNormAct if stage == 'pool' else nets.NormActUpsample
  module = Module(129, 'layer1em6', 'silu', fused=True)
  assert module.eps == 1e-6 and module.impl == 'layer' and module.scale.dtype == torch.float32
  assert isinstance(module, nets.NormAct) and Module(8, 'rms').shift is None
  x = torch.randn(3, 2, 10, 14, 129, device='cuda', requires_grad=True)
  before = nets.conv_stage_launches()
  out = module(x)
  assert nets.conv_stage_launches() == before + 1
  gout = torch.randn_like(out)
  out.backward(gout)
  assert nets.conv_stage_launches() == before + 3                  # dx and the partial sums, then their sum
  first, first_shift, first_dx = module.scale.grad.clone(), module.shift.grad.clone(), x.grad.clone()
  module.scale.grad = module.shift.grad = x.grad = None
  again = module(x)
  again.backward(gout)
  assert torch.equal(again, out) and torch.equal(x.grad, first_dx)
  assert torch.equal(module.scale.grad, first) and torch.equal(module.shift.grad, first_shift)     # the same bits
  call = _call(stage)
  before, norm_before = nets.conv_stage_launches(), nets.norm_act_launches()
  call(x, None, None, 'rms', 'silu', fused=True).backward(gout)
  assert nets.conv_stage_launches() == before + 2                  # no parameter gradients: one launch backward
  call(x, None, None, 'rms', 'silu', fused=False).backward(gout)
  assert nets.conv_stage_launches() == before + 2 and nets.norm_act_launches() == norm_before     # composed: none
  wide = torch.randn(1, 2, 2, 1025, device='cuda')
  with pytest.raises(ValueError, match='1024'):
    call(wide, fused=True)
  before = nets.conv_stage_launches()
  inp = {'x': _host(wide), 'scale': None, 'shift': None}
  want = stages.reference(stage, inp['x'], None, None, 'rms', 'silu', 1e-4)['out']
  assert norms.out_ratio(_host(call(wide)), want) <= 1.0           # fused=None composes it
  assert nets.conv_stage_launches() == before
  with pytest.raises(TypeError):
    call(torch.zeros(2, 2, 2, 8, device='cuda', dtype=torch.float16))
  with pytest.raises(ValueError, match='shape'):
    call(torch.zeros(2, 2, 2, 8, device='cuda'), torch.ones(7, device='cuda'))
  with pytest.raises(ValueError, match='H, W, C'):
    call(torch.zeros(2, 8, device='cuda'))


def test_conv_stage_fixture_on_both_paths():
  with np.load(GOLDEN) as f:
    for case, c in enumerate(stages.CASES):
      inp, want = stages.inputs(case), f[f'out64_{stages.tag(case)}']
      for fused in (True, False):
        out, _, _, _ = _run(c.stage, inp, c.impl, c.act, c.eps, 'f32', fused, grads=False)
        assert norms.out_ratio(out, want) <= 1.0, (stages.tag(case), fused)
      out, _, _, _ = _run(c.stage, _rounded(inp, 'bf16'), c.impl, c.act, c.eps, 'bf16', True, grads=False)
      rounded = stages.reference(c.stage, norms.bf16_round(inp['x']), inp['scale'], inp['shift'], c.impl, c.act,
                                 c.eps)['out']
      assert norms.out_ratio(out, rounded, True) <= 1.0, stages.tag(case)
