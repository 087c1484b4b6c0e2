"""The non-GEMM pieces of DreamerV3's recurrence on device: `Norm` followed by the
activation (embodied/jax/nets.py:361-399, nets.py:26-39), which follows every
`Linear`, `BlockLinear` and `Conv2D` of the networks and runs four times inside
`RSSM._core` (dreamerv3/rssm.py:141-151), and the blocked GRU gate at the end of
`_core` (dreamerv3/rssm.py:152-159).

They feed what `outs` and `scans` consume: `_core`'s new `deter` goes through
`_prior` (two more norm + activation pairs, rssm.py:163-165) into the logits of
`outs.rssm_kl`.

Inputs are torch CUDA tensors, float32 or bfloat16; the kernels' arithmetic is
float32 and rounds once, at the store.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import address as _address, api
from .outs import _fused_path

# What the kernels take: a row of at most 16 384 units stays in the registers of
# one workgroup, indices are 32-bit.  Structural, not a crossover: the fused
# median is below the composed one at all 36 rows of profiles/rssm_core_bench.txt
# -- norm (16, 1024) f32: forward 15.7 us against 50.3, forward + backward 56.3
# against 176.2; (16384, 1024) f32: 24.7 / 139.3 and 101.5 / 539.3; gate (16, 8192,
# 8) f32: 14.2 / 63.1 and 52.1 / 183.8 -- so no size constant sits beside
# `_norm_path` or `_gate_path`.
NORM_ACT_MAX_UNITS = 16384
NORM_ACT_MAX_ELEMENTS = 2 ** 31 - 1
GRU_GATE_MAX_ELEMENTS = 2 ** 31 - 1                # of x: rows * 3 * deter
# csrc/norm_act.h: up to here a wave takes a row, four rows per workgroup; the
# gradient launch has at most this many workgroups, each leaves one row of partial sums
_WAVE_UNITS, _MAX_PARTIALS = 1024, 512

# The conv-stage kernels (csrc/conv_stage.h): a pixel of at most 1024 channels in
# the registers of one wave64, 32-bit indices into the larger tensor; the gradient
# launch has at most _STAGE_MAX_PARTIALS workgroups, one row of partial sums each.
# Structural, not a crossover: the fused median is below both rivals -- the
# composed path and amax + norm_act(fused=True) / norm_act(fused=True) +
# repeat_interleave -- at all 72 rows of profiles/conv_stage_bench.txt.  Pool
# (1024, 64, 64, 128) f32: forward 491.2 us against 1630.8 and 986.2, forward +
# backward 1456.6 against 10676.2 and 7977.0; (16, 64, 64, 128) f32: 16.9 / 59.8 /
# 24.7 and 115.5 / 250.8 / 158.8; upsample (1024, 32, 32, 128) bf16: 259.5 / 2264.2 /
# 1598.9 and 684.8 / 5960.5 / 3793.6 -- so no size constant sits beside
# `_pool_path` or `_upsample_path`.
CONV_STAGE_MAX_UNITS = 1024
CONV_STAGE_MAX_ELEMENTS = 2 ** 31 - 1
_STAGE_MAX_PARTIALS = 1024

IMPLS = {'rms': 0, 'layer': 1}
ACTS = {'none': 0, 'silu': 1, 'gelu': 2, 'relu': 3}
_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def norm_act_launches():
  """Kernel launches `emb_norm_act` and `emb_norm_act_grad` have issued in this process."""
  return _lib.launches('norm_act')


def conv_stage_launches():
  """Kernel launches `emb_pool_norm_act*` and `emb_norm_act_upsample*` have issued in this process."""
  return _lib.launches('conv_stage')


def gru_gate_launches():
  """Kernel launches `emb_gru_gate` and `emb_gru_gate_grad` have issued in this process."""
  return _lib.launches('gru_gate')


def _norm_path(fused, rows, units):
  """True: the kernels, False: the composed path (`norm_act` says when).
  The kernels' median was below the composed path's at every shape, dtype and
  piece measured (profiles/rssm_core_bench.txt), so `fused=None` takes them
  wherever they fit: that held, no crossover constant."""
  row, index = 1 <= units <= NORM_ACT_MAX_UNITS, rows * units <= NORM_ACT_MAX_ELEMENTS
  if row and index:
    return fused is None or bool(fused)
  return _fused_path(
      'norm_act', fused,
      (row, f'{units} units, the kernels keep a row of at most {NORM_ACT_MAX_UNITS} in one workgroup\'s registers'),
      (index, f'{rows} x {units} elements, the kernels index at most 2^31 - 1'))


def _gate_path(fused, rows, deter, blocks):
  """True: the kernel, False: the composed path (`gru_gate` says when).  As
  `_norm_path`: below the composed path at all 16 rows of profiles/rssm_core_bench.txt,
  so wherever it fits."""
  if rows * 3 * deter <= GRU_GATE_MAX_ELEMENTS:
    return fused is None or bool(fused)
  return _fused_path(
      'gru_gate', fused, (False, f'{rows} x {3 * deter} elements of x, the kernels index at most 2^31 - 1'))


def _check_device(who, x):
  if not (torch.is_tensor(x) and x.is_cuda):
    raise RuntimeError(f'embodied_amd.nets.{who} runs as HIP kernels: pass CUDA tensors (no CPU fallback)')


def _check_param(who, name, value, units, like):
  if value is None:
    return None
  if not torch.is_tensor(value):
    raise TypeError(f'{who}: {name} must be a float32 tensor, got {type(value).__name__}')
  if value.dtype != torch.float32:
    raise TypeError(f'{who}: {name} must be float32 (nets.py:404), got {value.dtype}')
  if tuple(value.shape) != (units,):
    raise ValueError(f'{who}: {name} of shape {tuple(value.shape)}, {units} units need ({units},)')
  if value.device != like.device:
    raise ValueError(f'{who}: {name} on {value.device}, x on {like.device}')
  return value


def _activation(name, x):
  """nets.py:26-39 for the four names the kernels know, as jax.nn writes them."""
  if name == 'none':
    return x
  if name == 'silu':
    return x * torch.sigmoid(x)
  if name == 'gelu':                     # jax.nn.gelu, approximate=True
    cdf = 0.5 * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * (x ** 3))))
    return x * cdf
  return torch.maximum(x, torch.zeros((), dtype=x.dtype, device=x.device))


def _composed_norm_act(x, scale, shift, impl, act, eps):
  """nets.py:374-399 and nets.py:26-39 operation by operation: float32 inside the
  norm, rounded to the dtype of `x`, the activation in that dtype."""
  dtype = x.dtype
  x = x.to(torch.float32)
  if impl == 'rms':
    mean2 = torch.square(x).mean(-1, keepdim=True)
    x = x * (torch.rsqrt(mean2 + eps) * (1.0 if scale is None else scale))
  else:
    mean = x.mean(-1, keepdim=True)
    mean2 = torch.square(x).mean(-1, keepdim=True)
    var = torch.maximum(torch.zeros((), dtype=x.dtype, device=x.device), mean2 - torch.square(mean))
    x = (x - mean) * (torch.rsqrt(var + eps) * (1.0 if scale is None else scale))
    if shift is not None:
      x = x + shift
  return _activation(act, x.to(dtype))


def _partial_floats(rows, units):
  """float32 values `emb_norm_act_grad` wants for its partial sums (norm_act_partials
  in csrc/norm_act.h; tests/test_norm_act_host.py holds the two against each other)."""
  per_block = 4 if units <= _WAVE_UNITS else 1
  return 2 * min(-(-rows // per_block), _MAX_PARTIALS) * units


class _FusedNormAct(torch.autograd.Function):
  """act(Norm(x)) on the kernels: one launch forward; backward one launch, two
  with a gradient for `scale` or `shift`."""

  @staticmethod
  def forward(ctx, x, scale, shift, impl, act, eps):
    units = x.shape[-1]
    flat = x.detach().reshape(-1, units).contiguous()
    out = torch.empty_like(flat)
    scale = None if scale is None else scale.detach().contiguous()
    shift = None if shift is None else shift.detach().contiguous()
    api.emb_norm_act(flat.data_ptr(), _address(scale), _address(shift), _DTYPES[x.dtype], flat.shape[0], units, impl,
                     act, eps, out.data_ptr(), _lib.raw_stream(x.device))
    ctx.saved = (flat, scale, shift, impl, act, eps, x.shape)
    ctx.set_materialize_grads(False)
    return out.view(x.shape)

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    if gout is None:
      return (None,) * 6
    flat, scale, shift, impl, act, eps, shape = ctx.saved
    rows, units = flat.shape
    want_x, want_scale, want_shift = ctx.needs_input_grad[:3]
    want_shift = want_shift and impl == IMPLS['layer']
    gout = gout.to(flat.dtype).reshape(rows, units).contiguous()
    dx = torch.empty_like(flat) if want_x else None
    dscale = _lib.empty((units,), torch.float32, flat.device) if want_scale else None
    dshift = _lib.empty((units,), torch.float32, flat.device) if want_shift else None
    partials, floats = None, 0
    if want_scale or want_shift:
      floats = _partial_floats(rows, units)
      partials = _lib.empty((floats,), torch.float32, flat.device)
    if dx is None and dscale is None and dshift is None:
      return (None,) * 6
    api.emb_norm_act_grad(
        flat.data_ptr(), _address(scale), _address(shift), gout.data_ptr(), _DTYPES[flat.dtype], rows, units, impl, act,
        eps, _address(dx), _address(dscale), _address(dshift), _address(partials), floats, _lib.raw_stream(flat.device))
    if ctx.needs_input_grad[2] and dshift is None:      # rms does not read its shift
      dshift = torch.zeros_like(shift)
    return (None if dx is None else dx.view(shape), dscale, dshift, None, None, None)


def _eps_of(impl, eps):
  """nets.py:369-371: 'rms1em6' is rms with eps = 10 ** -6."""
  if isinstance(impl, str) and '1em' in impl:
    impl, exp = impl.split('1em')
    eps = 10 ** -int(exp)
  return impl, eps


def norm_act(x, scale=None, shift=None, impl='rms', act='silu', eps=1e-4, fused=None):
  """`nn.act(act)(Norm(impl)(x))` (nets.py:361-399, nets.py:26-39) over the last
  axis of a CUDA tensor of float32 or bfloat16 with any leading shape; the result
  has the shape and dtype of `x` and is differentiable once with respect to `x`,
  `scale` and `shift`.

    rms    y = x * (rsqrt(mean(x^2) + eps) * scale)
    layer  y = (x - mean) * (rsqrt(max(0, mean(x^2) - mean^2) + eps) * scale) + shift

  `scale` and `shift` are float32 `(units,)` or None (ones / zeros); `rms` takes
  no shift.  `impl` may carry the reference's eps suffix ('rms1em6').  `act` is
  'none', 'silu', 'gelu' (the tanh approximation, jax.nn.gelu's default) or 'relu'.

  Two paths.  Composed restates the reference operation by operation in torch
  (the definition, every size): float32 inside the norm, rounded to the dtype of
  `x`, the activation in that dtype.  Fused is `emb_norm_act` /
  `emb_norm_act_grad`: 1 .. 16 384 units, one launch forward; backward one
  launch, two with a gradient for `scale` or `shift`; no atomics, the same bits
  run to run.  `fused=None` takes the kernels where they fit, True / False force
  a path (True raises where they do not fit, and says why).  No rows: the composed
  path, nothing is launched.

  The documented difference: the kernels apply the activation to the float32
  value and round once; the reference rounds to the compute dtype between norm
  and activation (nets.py:398).  For float32 inputs there is none.

  Non-finite inputs.  On the kernels a row with a NaN or an infinite element (or
  whose squares overflow float32) is NaN throughout, in the output and in `dx`,
  and no other row is touched; the gradients of `scale` and `shift` sum over it.
  Composed is the definition: an infinite element makes its row's rstd 0, so the
  row's finite elements come out 0 and the infinite one NaN."""
  _check_device('norm_act', x)
  if x.dtype not in _DTYPES:
    raise TypeError(f'norm_act: x must be float32 or bfloat16, got {x.dtype}')
  impl, eps = _eps_of(impl, eps)
  if impl not in IMPLS:
    raise ValueError(f'norm_act: impl = {impl!r}, needs one of {sorted(IMPLS)}')
  if act not in ACTS:
    raise ValueError(f'norm_act: act = {act!r}, needs one of {sorted(ACTS)}')
  eps = float(eps)
  if not (np.isfinite(eps) and eps >= 0):
    raise ValueError(f'norm_act: eps = {eps}, needs a finite value that is not negative')
  if x.dim() < 1 or x.shape[-1] < 1:
    raise ValueError(f'norm_act: x of shape {tuple(x.shape)}, needs (..., units)')
  units = x.shape[-1]
  scale = _check_param('norm_act', 'scale', scale, units, x)
  shift = _check_param('norm_act', 'shift', shift, units, x)
  if impl == 'rms' and shift is not None:
    raise ValueError('norm_act: rms takes no shift (nets.py:382-386)')
  rows = int(np.prod(x.shape[:-1], dtype=np.int64))
  if _norm_path(fused, rows, units) and rows > 0:
    return _FusedNormAct.apply(x, scale, shift, IMPLS[impl], ACTS[act], eps)
  return _composed_norm_act(x, scale, shift, impl, act, eps)


class NormAct(torch.nn.Module):
  """`nn.act(act)(Norm(impl)(x))` with the norm's parameters: float32 `scale`
  (ones, nets.py:401-404) and, for 'layer', `shift` (zeros, nets.py:406-409);
  `scale=False` / `shift=False` leave one out, as the reference's fields do.
  `impl` takes the reference's 'rms1em6' spelling of eps (nets.py:369-371).
  Parameters are made on `device` (default: the current CUDA device)."""

  def __init__(self, units, impl='rms', act='silu', eps=1e-4, scale=True, shift=True, fused=None, device=None):
    super().__init__()
    impl, eps = _eps_of(impl, eps)
    if impl not in IMPLS:
      raise ValueError(f'NormAct: impl = {impl!r}, needs one of {sorted(IMPLS)}')
    if act not in ACTS:
      raise ValueError(f'NormAct: act = {act!r}, needs one of {sorted(ACTS)}')
    if int(units) < 1:
      raise ValueError(f'NormAct: units = {units}, needs at least 1')
    self.units, self.impl, self.act, self.eps, self.fused = int(units), impl, act, float(eps), fused
    device = 'cuda' if device is None else device
    self.scale = torch.nn.Parameter(torch.ones(self.units, dtype=torch.float32, device=device)) if scale else None
    self.shift = (torch.nn.Parameter(torch.zeros(self.units, dtype=torch.float32, device=device))
                  if shift and impl == 'layer' else None)

  def forward(self, x):
    return norm_act(x, self.scale, self.shift, self.impl, self.act, self.eps, self.fused)

  def extra_repr(self):
    return f'{self.units}, impl={self.impl!r}, act={self.act!r}, eps={self.eps:g}'


def _stage_lanes(units):
  """Lanes of a wave64 that share one pixel (conv_stage_lanes in csrc/conv_stage.h)."""
  return 8 if units <= 64 else 16 if units <= 128 else 32 if units <= 256 else 64


def _stage_partial_floats(pixels, units):
  """float32 values `emb_pool_norm_act_grad` / `emb_norm_act_upsample_grad` want for
  their partial sums over `pixels` Norm rows (conv_stage_partials in
  csrc/conv_stage.h; tests/test_conv_stage_host.py holds the two against each other)."""
  per_block = 4 * (64 // _stage_lanes(units))
  return 2 * min(-(-pixels // per_block), _STAGE_MAX_PARTIALS) * units


def _stage_path(who, fused, units, elements):
  row, index = 1 <= units <= CONV_STAGE_MAX_UNITS, elements <= CONV_STAGE_MAX_ELEMENTS
  if row and index:
    return fused is None or bool(fused)
  return _fused_path(
      who, fused,
      (row, f'{units} channels, the kernels keep a pixel of at most {CONV_STAGE_MAX_UNITS} in one wave\'s registers'),
      (index, f'{elements} elements in the larger tensor, the kernels index at most 2^31 - 1'))


def _pool_path(fused, images, height, width, units):
  """True: the kernels, False: the composed path (`pool_norm_act` says when).  As
  `_norm_path`: below the composed path and below `amax` + the fused `norm_act`
  at all 40 pool rows of profiles/conv_stage_bench.txt, so wherever they fit."""
  return _stage_path('pool_norm_act', fused, units, images * height * width * units)


def _upsample_path(fused, images, height, width, units):
  """True: the kernels, False: the composed path (`norm_act_upsample` says when).
  Below both rivals at all 32 upsample rows of profiles/conv_stage_bench.txt."""
  return _stage_path('norm_act_upsample', fused, units, images * 4 * height * width * units)


def _composed_pool_norm_act(x, scale, shift, impl, act, eps):
  """rssm.py:239-241 operation by operation: the 2x2 windows as two axes of a
  reshape, their max (torch.amax: a NaN wins, tied maxima share the gradient
  equally), then `_composed_norm_act`."""
  *lead, height, width, units = x.shape
  pooled = x.reshape(*lead, height // 2, 2, width // 2, 2, units).amax((-4, -2))
  return _composed_norm_act(pooled, scale, shift, impl, act, eps)


def _composed_norm_act_upsample(x, scale, shift, impl, act, eps):
  """rssm.py:327, 336: `_composed_norm_act`, then every pixel repeated 2x2.  jnp's
  `x.repeat(2, axis)` repeats element by element: torch's `repeat_interleave`
  (`Tensor.repeat` tiles the whole axis instead)."""
  return _composed_norm_act(x, scale, shift, impl, act, eps).repeat_interleave(2, -2).repeat_interleave(2, -3)


class _FusedStage(torch.autograd.Function):
  """A conv stage's tail on the kernels (`pool`: 2x2 max + Norm + act, else Norm +
  act + 2x2 repeat): one launch forward; backward one launch, two with a gradient
  for `scale` or `shift`."""

  @staticmethod
  def forward(ctx, x, scale, shift, impl, act, eps, pool):
    height, width, units = x.shape[-3:]
    flat = x.detach().reshape(-1, height, width, units).contiguous()
    images = flat.shape[0]
    result = (images, height // 2, width // 2, units) if pool else (images, 2 * height, 2 * width, units)
    out = torch.empty(result, dtype=flat.dtype, device=flat.device)
    scale = None if scale is None else scale.detach().contiguous()
    shift = None if shift is None else shift.detach().contiguous()
    entry = api.emb_pool_norm_act if pool else api.emb_norm_act_upsample
    entry(flat.data_ptr(), _address(scale), _address(shift), _DTYPES[x.dtype], images, height, width, units, impl, act,
          eps, out.data_ptr(), _lib.raw_stream(x.device))
    ctx.saved = (flat, scale, shift, impl, act, eps, pool, x.shape, out.shape)
    ctx.set_materialize_grads(False)
    return out.view(*x.shape[:-3], *result[1:])

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    if gout is None:
      return (None,) * 7
    flat, scale, shift, impl, act, eps, pool, shape, out_shape = ctx.saved
    images, height, width, units = flat.shape
    want_x, want_scale, want_shift = ctx.needs_input_grad[:3]
    want_shift = want_shift and impl == IMPLS['layer']
    gout = gout.to(flat.dtype).reshape(out_shape).contiguous()
    dx = torch.empty_like(flat) if want_x else None
    dscale = _lib.empty((units,), torch.float32, flat.device) if want_scale else None
    dshift = _lib.empty((units,), torch.float32, flat.device) if want_shift else None
    partials, floats = None, 0
    if want_scale or want_shift:
      pixels = images * (height // 2) * (width // 2) if pool else images * height * width
      floats = _stage_partial_floats(pixels, units)
      partials = _lib.empty((floats,), torch.float32, flat.device)
    if dx is None and dscale is None and dshift is None:
      return (None,) * 7
    entry = api.emb_pool_norm_act_grad if pool else api.emb_norm_act_upsample_grad
    entry(flat.data_ptr(), _address(scale), _address(shift), gout.data_ptr(), _DTYPES[flat.dtype], images, height, width,
          units, impl, act, eps, _address(dx), _address(dscale), _address(dshift), _address(partials), floats,
          _lib.raw_stream(flat.device))
    if ctx.needs_input_grad[2] and dshift is None:      # rms does not read its shift
      dshift = torch.zeros_like(shift)
    return (None if dx is None else dx.view(shape), dscale, dshift, None, None, None, None)


def _stage(who, pool, x, scale, shift, impl, act, eps, fused):
  """The checks of `norm_act` for an `x` of (..., H, W, C), then the path."""
  _check_device(who, x)
  if x.dtype not in _DTYPES:
    raise TypeError(f'{who}: x must be float32 or bfloat16, got {x.dtype}')
  impl, eps = _eps_of(impl, eps)
  if impl not in IMPLS:
    raise ValueError(f'{who}: impl = {impl!r}, needs one of {sorted(IMPLS)}')
  if act not in ACTS:
    raise ValueError(f'{who}: act = {act!r}, needs one of {sorted(ACTS)}')
  eps = float(eps)
  if not (np.isfinite(eps) and eps >= 0):
    raise ValueError(f'{who}: eps = {eps}, needs a finite value that is not negative')
  if x.dim() < 3 or min(x.shape[-3:]) < 1:
    raise ValueError(f'{who}: x of shape {tuple(x.shape)}, needs (..., H, W, C), channels last')
  height, width, units = x.shape[-3:]
  if pool and (height % 2 or width % 2):
    raise ValueError(f'{who}: x of shape {tuple(x.shape)}, the 2x2 windows need an even H and W (rssm.py:239)')
  scale = _check_param(who, 'scale', scale, units, x)
  shift = _check_param(who, 'shift', shift, units, x)
  if impl == 'rms' and shift is not None:
    raise ValueError(f'{who}: rms takes no shift (nets.py:382-386)')
  images = int(np.prod(x.shape[:-3], dtype=np.int64))
  path = _pool_path if pool else _upsample_path
  if path(fused, images, height, width, units) and images > 0:
    return _FusedStage.apply(x, scale, shift, IMPLS[impl], ACTS[act], eps, pool)
  composed = _composed_pool_norm_act if pool else _composed_norm_act_upsample
  return composed(x, scale, shift, impl, act, eps)


def pool_norm_act(x, scale=None, shift=None, impl='rms', act='silu', eps=1e-4, fused=None):
  """The tail of an `Encoder` stage with `strided=False` (dreamerv3/rssm.py:238-241):
  after the stage's `Conv2D`, the max over 2x2 windows, `Norm` and `act`.  `x` is
  a CUDA tensor (..., H, W, C), channels last as in the reference, float32 or
  bfloat16, H and W even (the reference's reshape takes no others); the result
  is (..., H/2, W/2, C) in the dtype of `x`, differentiable once with respect to
  `x`, `scale` and `shift`.  `scale`, `shift`, `impl`, `act` and `eps` as `norm_act`.
  A non-contiguous `x` (a channels-first conv output, permuted) is copied.

  Two paths, as `norm_act`.  Composed is the definition at every size:
  `x.reshape(..., H/2, 2, W/2, 2, C).amax((-4, -2))`, then `norm_act`'s composed
  path.  Fused is `emb_pool_norm_act` / `emb_pool_norm_act_grad`, 1 .. 1024
  channels and at most 2^31 - 1 elements of `x`: ONE launch forward that reads the
  four window rows, keeps the pooled row in registers and writes the activated
  row; backward ONE launch that recomputes the pooled row from `x` (nothing is
  saved but `x`) and writes all of `dx`, two with a gradient for `scale` or
  `shift`; no atomics, the same bits run to run.  `fused=None`, True, False and
  zero images as `norm_act`.

  Ties: among the positions of a window that equal its max the gradient is
  split equally (torch.amax; jax's reduce_max rule does the same), the others
  get exactly 0.  Selecting a max is exact, so the pool adds no rounding and the
  documented difference is `norm_act`'s alone.

  Non-finite inputs.  A NaN anywhere in a window is that window's max, on both
  paths.  On the kernels a pixel whose pooled row has a NaN or an infinite
  element (a window of all -inf too) is NaN throughout, in the output and in its
  four pixels of `dx`, and no other pixel is touched."""
  return _stage('pool_norm_act', True, x, scale, shift, impl, act, eps, fused)


def norm_act_upsample(x, scale=None, shift=None, impl='rms', act='silu', eps=1e-4, fused=None):
  """The tail of a `Decoder` stage (dreamerv3/rssm.py:327, 336-338, 346):
  `act(Norm(x))` and then every pixel repeated 2x2, which feeds the next `Conv2D`.
  `x` is a CUDA tensor (..., H, W, C), channels last, float32 or bfloat16; the
  result is (..., 2H, 2W, C) with `out[..., 2h+i, 2w+j, :] = act(Norm(x))[..., h, w, :]`
  for i, j in {0, 1}, differentiable once with respect to `x`, `scale` and `shift`.
  Everything else as `pool_norm_act`.

  Composed: `norm_act`'s composed path, then `.repeat_interleave(2, -2)
  .repeat_interleave(2, -3)` (jnp's `repeat`; torch's `Tensor.repeat` would tile).
  Fused is `emb_norm_act_upsample` / `emb_norm_act_upsample_grad`, 1 .. 1024
  channels and at most 2^31 - 1 elements of the result: ONE launch forward that
  reads a row once and writes its four copies; backward ONE launch that adds the
  four rows of the incoming gradient in float32, in the fixed order
  ((0,0) + (0,1)) + ((1,0) + (1,1)), and forms `norm_act`'s gradient from the sum,
  two with a gradient for `scale` or `shift`."""
  return _stage('norm_act_upsample', False, x, scale, shift, impl, act, eps, fused)


class PoolNormAct(NormAct):
  """`pool_norm_act` with the norm's parameters: `NormAct` over `units` channels
  behind a 2x2 max pool (dreamerv3/rssm.py:238-241)."""

  def forward(self, x):
    return pool_norm_act(x, self.scale, self.shift, self.impl, self.act, self.eps, self.fused)


class NormActUpsample(NormAct):
  """`norm_act_upsample` with the norm's parameters: `NormAct` over `units`
  channels in front of a 2x2 repeat (dreamerv3/rssm.py:327, 336-338, 346)."""

  def forward(self, x):
    return norm_act_upsample(x, self.scale, self.shift, self.impl, self.act, self.eps, self.fused)


def _composed_gru_gate(x, deter, blocks):
  """rssm.py:139-140, 153-158 operation by operation, in the dtype of `x`."""
  lead, width = deter.shape[:-1], deter.shape[-1]
  grouped = x.reshape(*lead, blocks, 3 * width // blocks)                       # flat2group
  gates = torch.split(grouped, width // blocks, -1)
  reset, cand, update = [g.reshape(*lead, width) for g in gates]               # group2flat
  reset = torch.sigmoid(reset)
  cand = torch.tanh(reset * cand)
  update = torch.sigmoid(update - 1)
  return update * cand + (1 - update) * deter


class _FusedGate(torch.autograd.Function):
  """The new deter on the kernels: one launch forward, one backward."""

  @staticmethod
  def forward(ctx, x, deter, blocks):
    width = deter.shape[-1]
    xs = x.detach().reshape(-1, 3 * width).contiguous()
    ds = deter.detach().reshape(-1, width).contiguous()
    out = torch.empty_like(ds)
    api.emb_gru_gate(xs.data_ptr(), ds.data_ptr(), _DTYPES[xs.dtype], ds.shape[0], width, blocks, out.data_ptr(),
                     _lib.raw_stream(xs.device))
    ctx.saved = (xs, ds, blocks, x.shape, deter.shape)
    ctx.set_materialize_grads(False)
    return out.view(deter.shape)

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    if gout is None:
      return None, None, None
    xs, ds, blocks, xshape, dshape = ctx.saved
    want_x, want_deter = ctx.needs_input_grad[:2]
    if not (want_x or want_deter):
      return None, None, None
    gout = gout.to(ds.dtype).reshape(ds.shape).contiguous()
    dx = torch.empty_like(xs) if want_x else None
    ddeter = torch.empty_like(ds) if want_deter else None
    api.emb_gru_gate_grad(xs.data_ptr(), ds.data_ptr(), gout.data_ptr(), _DTYPES[ds.dtype], ds.shape[0], ds.shape[1],
                          blocks, _address(dx), _address(ddeter), _lib.raw_stream(ds.device))
    return (None if dx is None else dx.view(xshape), None if ddeter is None else ddeter.view(dshape), None)


def gru_gate(x, deter, blocks, fused=None):
  """The tail of `RSSM._core` (rssm.py:152-159): the new `deter`, in the shape and
  dtype of `deter`, from `x` (..., 3 * deter), the output of the `dyngru`
  BlockLinear, and the old `deter` (..., deter); `blocks` divides deter and
  h = deter / blocks.  For block k and j < h

      reset  = sigmoid(x[..., 3hk + j])
      cand   = tanh(reset * x[..., 3hk + h + j])
      update = sigmoid(x[..., 3hk + 2h + j] - 1)
      out[..., hk + j] = update * cand + (1 - update) * deter[..., hk + j]

  differentiable once with respect to `x` and `deter`.  Both are CUDA tensors of
  one dtype, float32 or bfloat16.

  Two paths, as `norm_act`.  Composed is the reference's reshape, split and
  elementwise operations in the dtype of `x`; fused is `emb_gru_gate` /
  `emb_gru_gate_grad`, float32 arithmetic rounded once at the store, ONE launch
  forward and ONE backward, the split done by index arithmetic.  Saturated gates
  give finite values and zero or tiny gradients; a NaN touches the output
  element and the gradient elements it feeds, nothing else.  No rows: the
  composed path, nothing is launched."""
  _check_device('gru_gate', x)
  _check_device('gru_gate', deter)
  if x.dtype not in _DTYPES:
    raise TypeError(f'gru_gate: x must be float32 or bfloat16, got {x.dtype}')
  if deter.dtype != x.dtype:
    raise TypeError(f'gru_gate: deter is {deter.dtype}, x is {x.dtype}: one dtype for both')
  if deter.device != x.device:
    raise ValueError(f'gru_gate: deter on {deter.device}, x on {x.device}')
  if deter.dim() < 1 or deter.shape[-1] < 1:
    raise ValueError(f'gru_gate: deter of shape {tuple(deter.shape)}, needs (..., deter)')
  width = deter.shape[-1]
  if tuple(x.shape) != (*deter.shape[:-1], 3 * width):
    raise ValueError(f'gru_gate: x of shape {tuple(x.shape)}, deter {tuple(deter.shape)} needs '
                     f'{(*deter.shape[:-1], 3 * width)}')
  blocks = int(blocks)
  if blocks < 1 or width % blocks:
    raise ValueError(f'gru_gate: blocks = {blocks} does not divide deter = {width} (rssm.py:35)')
  rows = int(np.prod(deter.shape[:-1], dtype=np.int64))
  if _gate_path(fused, rows, width, blocks) and rows > 0:
    return _FusedGate.apply(x, deter, blocks)
  return _composed_gru_gate(x, deter, blocks)


# ------------------------------------------------------------- DictConcat --
# csrc/dict_concat.h: at most 16 keys (a row's availability flags are one 16-bit
# word), a row of at most 16 384 columns, classes at most 16 384, 32-bit indices
# into `out`.  Structural limits.  Whether `fused=None` takes the kernel inside
# them is `_dict_path`'s answer, with the measured figures beside it.
DICT_MAX_KEYS = _lib.DICT_MAX_KEYS
DICT_MAX_WIDTH = 16384
DICT_MAX_CLASSES = 16384
DICT_MAX_ELEMENTS = 2 ** 31 - 1
SQUISHES = {None: _lib.DICT_NONE, 'none': _lib.DICT_NONE, 'symlog': _lib.DICT_SYMLOG}
_DICT_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.int32: _lib.I32, torch.int64: _lib.I64,
                torch.uint8: _lib.U8, torch.bool: _lib.BOOL}
_DICT_FLOATS = (torch.float32, torch.bfloat16)


def dict_concat_launches():
  """Kernel launches `emb_dict_concat` has issued in this process."""
  return _lib.launches('dict_concat')


def _dict_path(fused, fits):
  """True: the kernel, False: the composed path (`DictConcat` says when).  `fits`
  is what the kernel takes, as `_fused_path` reads it.  The kernel's median was
  below the composed path's at all 18 rows of profiles/dict_concat_bench.txt --
  two discrete and two float keys at 16 rows: 16.6 us against 194.2; 16 mixed keys
  at 1024 rows: 39.1 / 964.5; the Encoder's 8 symlog keys of 1024 columns at 65 536
  rows: f32 675.7 / 1240.8, bf16 938.3 / 1224.9 -- so `fused=None` takes it wherever
  it fits and no size constant sits here."""
  if all(holds for holds, _ in fits):
    return fused is None or bool(fused)
  return _fused_path('dict_concat', fused, *fits)


def _available(x, bdims):
  """nets.py:80-99 with `bdims`, for one tensor."""
  if x.dtype.is_floating_point:
    mask = x != -np.inf
  elif x.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
    mask = x != -1
  elif x.dtype in (torch.uint8, torch.bool):
    return torch.ones(x.shape[:bdims], dtype=torch.bool, device=x.device)
  else:
    raise NotImplementedError(x.dtype)
  return mask.flatten(bdims).all(-1) if mask.dim() > bdims else mask


def _where(condition, x, y):
  """nets.py:67-73 for one tensor: the condition's trailing axes are added."""
  assert condition.dtype == torch.bool, condition.dtype
  return torch.where(condition.reshape(*condition.shape, *([1] * (x.dim() - condition.dim()))), x, y)


def _mask(x, mask):
  """nets.py:76-77."""
  return _where(mask, x, torch.zeros_like(x))


def _symlog(x):
  """nets.py:59-60."""
  return torch.sign(x) * torch.log1p(torch.abs(x))


def _composed_dict_concat(xs, keys, spaces, classes, fdims, squish, dtype, reset, unit):
  """nets.py:476-500 operation by operation, then rssm.py:76-79 and rssm.py:137.
  `jax.nn.one_hot` is its definition, a comparison against arange(classes): an
  index outside [0, classes) gives zeros (torch's own one_hot refuses one)."""
  bdims = xs[keys[0]].dim() - len(spaces[keys[0]].shape)
  ys = []
  for key in keys:
    x = xs[key]
    m = _available(x, bdims)
    x = _mask(x, m)
    if spaces[key].discrete:
      x = x.to(torch.int32)
      x = (x.unsqueeze(-1) == torch.arange(classes[key], dtype=torch.int32, device=x.device)).to(dtype)
    else:
      if squish == 'symlog':
        x = _symlog(x)
      x = x.to(dtype)
    x = _mask(x, m)
    ys.append(x.reshape(*x.shape[:bdims + fdims - 1], int(np.prod(x.shape[bdims + fdims - 1:], dtype=np.int64))))
  y = torch.cat(ys, -1)
  if reset is not None:                            # rssm.py:76-79: both masks are this one
    y = _mask(y, ~reset.to(torch.bool))
  if unit:                                         # rssm.py:137, in the compute dtype
    y = y / torch.maximum(torch.ones((), dtype=y.dtype, device=y.device), torch.abs(y))
  return y


class DictConcat:
  """`nn.DictConcat(spaces, fdims, squish)` (embodied/jax/nets.py:467-500): a dict
  of CUDA tensors, one per key of `spaces` in sorted order, as one `(*batch, width)`
  tensor of `dtype` (float32 or bfloat16, the reference's COMPUTE_DTYPE).  A
  discrete space becomes the one-hot of its `classes` per element, any other the
  `squish` (None or 'symlog') of its values; a row of a key with an element that is
  not available (nets.py:80-99: -inf in a float, -1 in a signed integer) is zeros
  in that key's columns.  The batch axes are those of the first key in front of
  its space's shape (nets.py:478).

      concat = nets.DictConcat(act_space)
      action = concat(prevact, reset=reset, unit=True)       # rssm.py:76-79, 137
      vector = nets.DictConcat(vspace, squish='symlog')(obs)  # rssm.py:216-220

  `reset` (`(*batch,)`, bool or uint8): rows where it is set are zeros, which is
  both masks of rssm.py:76-79.  `unit=True` stores every continuous value v as
  v / max(1, |v|) (rssm.py:137).  `out`: a tensor `(*batch, width)` of `dtype` to
  write into, or a column slice of one (unit column stride, batch axes that
  collapse into one row stride); it is returned.  The result never requires grad:
  the reference's three uses feed data or stop-gradient actions.

  Two paths.  Composed restates the reference operation by operation in torch
  (the definition, every size, CPU tensors excepted: there is no CPU fallback).
  Fused is `emb_dict_concat`: ONE launch for inputs of float32, bfloat16, int32,
  int64, uint8 or bool, at most 16 keys, 16 384 columns and 16 384 classes,
  `fdims=1`; float32 arithmetic rounded once at the store, no atomics, the same
  bits run to run.  `fused=None` takes the kernel where it fits, True / False
  force a path (True raises where it does not fit, and says why).  An input that
  requires grad does not fit.  No rows: the composed path, nothing is launched.

  The documented differences.  An int64 index beyond the int32 range is out of
  range on the kernel (zeros); composed wraps it, as `astype(int32)` would -- the
  reference never sees one, JAX runs without x64.  `symlog` of a bfloat16 input is
  float32 arithmetic on the kernel and bfloat16 arithmetic composed.  With `unit`
  the kernel divides before it rounds and the reference after: for every finite v
  the bits are the same (|v| <= 1 stores the rounded v, anything else +-1).

  The key table is built once per (shapes, dtypes) of a call and kept; a call
  only writes the addresses into it."""

  def __init__(self, spaces, fdims=1, squish=None, dtype=torch.bfloat16):
    if int(fdims) < 1:
      raise ValueError(f'DictConcat: fdims = {fdims}, needs at least 1 (nets.py:470)')
    if squish not in SQUISHES:
      raise ValueError(f'DictConcat: squish = {squish!r}, needs None or \'symlog\'')
    if dtype not in _DTYPES:
      raise TypeError(f'DictConcat: dtype must be float32 or bfloat16, got {dtype}')
    if not spaces:
      raise ValueError('DictConcat: no spaces')
    self.keys = sorted(spaces.keys())
    self.spaces, self.fdims, self.dtype = dict(spaces), int(fdims), dtype
    self.squish = None if squish in (None, 'none') else squish
    self.classes, self.spans = {}, {}
    for key in self.keys:
      space = self.spaces[key]
      if space.dtype == np.uint8 and len(space.shape) in (2, 3):
        raise NotImplementedError('Images are not supported.')
      elements = int(np.prod(space.shape, dtype=np.int64))
      if space.discrete:
        classes = np.asarray(space.classes).flatten()
        if classes.size and not (classes == classes[0]).all():
          raise ValueError(f'DictConcat: the elements of {key!r} differ in classes: {classes.tolist()} (nets.py:490)')
        self.classes[key] = int(classes[0]) if classes.size else 0
        self.spans[key] = elements * self.classes[key]
      else:
        self.spans[key] = elements
    self.width = sum(self.spans.values())
    self._tables = {}

  def _table(self, signature):
    """The ctypes key table of inputs with this (dtype per key): everything but the addresses."""
    table = self._tables.get(signature)
    if table is None:
      table = (_lib.DictEntry * len(self.keys))()
      first = 0
      for entry, key, dtype in zip(table, self.keys, signature):
        space = self.spaces[key]
        entry.dtype = _DICT_DTYPES[dtype]
        entry.kind = _lib.DICT_ONEHOT if space.discrete else SQUISHES[self.squish]
        entry.elements = int(np.prod(space.shape, dtype=np.int64))
        entry.classes = self.classes.get(key, 0)
        entry.first = first
        first += self.spans[key]
      self._tables[signature] = table
    return table

  def _fits(self, xs, rows, stride):
    """What the kernel takes, as (holds, wording) in the order it is checked."""
    fits = [
        (self.fdims == 1, f'fdims = {self.fdims}, the kernel writes one feature axis'),
        (len(self.keys) <= DICT_MAX_KEYS, f'{len(self.keys)} keys, the kernel takes at most {DICT_MAX_KEYS}'),
        (1 <= self.width <= DICT_MAX_WIDTH, f'{self.width} columns, the kernel writes a row of 1 .. {DICT_MAX_WIDTH}'),
        (max(self.classes.values(), default=1) <= DICT_MAX_CLASSES and min(self.classes.values(), default=1) >= 1,
         f'classes of {sorted(self.classes.values())}, the kernel takes 1 .. {DICT_MAX_CLASSES}'),
        (rows * max(stride, 1) <= DICT_MAX_ELEMENTS, f'{rows} rows {stride} elements apart, the kernel indexes at most 2^31 - 1'),
        (not any(xs[k].requires_grad for k in self.keys), 'an input requires grad, the kernel has no backward'),
    ]
    for key in self.keys:
      dtype, space = xs[key].dtype, self.spaces[key]
      fits.append((dtype in _DICT_DTYPES, f'{key!r} is {dtype}, the kernel reads float32, bfloat16, int32, int64, uint8 and bool'))
      fits.append((not (space.discrete and dtype in _DICT_FLOATS), f'{key!r} is a discrete space fed {dtype}, the kernel compares integers'))
      fits.append((not (self.squish and not space.discrete and dtype not in _DICT_FLOATS),
                   f'{key!r} is {dtype} under {self.squish}, the kernel squishes floats'))
    return fits

  def __call__(self, xs, reset=None, unit=False, out=None, fused=None):
    keys = self.keys
    missing = [k for k in keys if k not in xs]
    if missing:
      raise KeyError(f'DictConcat: no input for {missing} (nets.py:477)')
    for key in keys:
      _check_device('DictConcat', xs[key])
    first = xs[keys[0]]
    bdims = first.dim() - len(self.spaces[keys[0]].shape)
    if bdims < 0:
      raise ValueError(f'DictConcat: {keys[0]!r} of shape {tuple(first.shape)}, its space is {self.spaces[keys[0]].shape}')
    batch = tuple(first.shape[:bdims])
    for key in keys:
      if tuple(xs[key].shape[bdims:]) != tuple(self.spaces[key].shape) or tuple(xs[key].shape[:bdims]) != batch:
        raise ValueError(f'DictConcat: {key!r} of shape {tuple(xs[key].shape)}, batch {batch} and its space '
                         f'{tuple(self.spaces[key].shape)} need {(*batch, *self.spaces[key].shape)} (nets.py:485)')
      if xs[key].device != first.device:
        raise ValueError(f'DictConcat: {key!r} on {xs[key].device}, {keys[0]!r} on {first.device}')
    rows = int(np.prod(batch, dtype=np.int64))
    if reset is not None:
      _check_device('DictConcat', reset)
      if reset.dtype not in (torch.bool, torch.uint8) or tuple(reset.shape) != batch:
        raise ValueError(f'DictConcat: reset of {reset.dtype} {tuple(reset.shape)}, needs bool or uint8 {batch}')
    stride = self.width
    if out is not None:
      _check_device('DictConcat', out)
      stride = self._out_stride(out, batch)
    if _dict_path(fused, self._fits(xs, rows, stride)) and rows > 0:
      return self._fused(xs, batch, rows, reset, unit, out, stride)
    with torch.no_grad():
      y = _composed_dict_concat(xs, keys, self.spaces, self.classes, self.fdims, self.squish, self.dtype, reset, unit)
    if out is None:
      return y
    out.copy_(y)
    return out

  def _out_stride(self, out, batch):
    """Elements from one row of `out` to the next; refuses what is no (rows, width) view."""
    if out.dtype != self.dtype or tuple(out.shape) != (*batch, self.width) or self.fdims != 1:
      raise ValueError(f'DictConcat: out of {out.dtype} {tuple(out.shape)}, needs {self.dtype} {(*batch, self.width)}')
    if out.requires_grad:
      raise ValueError('DictConcat: out requires grad')
    strides, shape = out.stride(), out.shape
    if self.width > 1 and strides[-1] != 1:
      raise ValueError(f'DictConcat: out has a column stride of {strides[-1]}, needs 1')
    live = [i for i in range(len(batch)) if shape[i] > 1]
    if not live:
      return self.width
    for i, j in zip(live[:-1], live[1:]):
      if strides[i] != strides[j] * shape[j]:
        raise ValueError(f'DictConcat: the batch axes of out (strides {strides}) do not collapse into one row stride')
    if strides[live[-1]] < self.width:
      raise ValueError(f'DictConcat: the rows of out are {strides[live[-1]]} elements apart, fewer than {self.width}')
    return strides[live[-1]]

  def _fused(self, xs, batch, rows, reset, unit, out, stride):
    held = [xs[k].detach().contiguous() for k in self.keys]          # alive until the launch is enqueued
    table = self._table(tuple(x.dtype for x in held))
    for entry, x in zip(table, held):
      entry.x = x.data_ptr()
    device = held[0].device
    if out is None:
      out = _lib.empty((*batch, self.width), self.dtype, device)
    if reset is not None:
      reset = reset.contiguous()
    _lib.fast.emb_dict_concat(table, len(held), rows, self.width, out.data_ptr(), stride, _DTYPES[self.dtype],
                              _address(reset), int(bool(unit)), _lib.raw_stream(device))
    return out


def dict_concat(xs, spaces, fdims=1, squish=None, dtype=torch.bfloat16, reset=None, unit=False, out=None, fused=None):
  """`DictConcat(spaces, fdims, squish, dtype)(xs, reset, unit, out, fused)` as a
  function; the key table is built on every call."""
  return DictConcat(spaces, fdims, squish, dtype)(xs, reset=reset, unit=unit, out=out, fused=fused)
