"""The running return normaliser (embodied/jax/utils.py:16-91) resident on the
device: every call is ONE kernel launch (`emb_normalize`, csrc/normalize.hip)
on the current torch stream -- batch statistics, EMA step, debiasing and, if
asked for, the normalised values -- with no host synchronisation and no
allocation.

Single replica.  `distributed.Normalize` (torch ops, `comm=` / `group=`) stays the
form that agrees the statistics across data-parallel ranks; the two exchange
checkpoints through `state_dict()` / `load_state_dict()`.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import fast

_IMPLS = {'meanstd': _lib.NORM_MEANSTD, 'perc': _lib.NORM_PERC}
# state words: mean | lo, sqrs | hi, corr, offset, scale
_WORDS = {'meanstd': ('mean', 'sqrs'), 'perc': ('lo', 'hi')}


def launches():
  """Kernel launches `emb_normalize` has issued in this process."""
  return _lib.launches('normalize')


class DeviceNormalize:
  """`distributed.Normalize` for one replica with its state in device memory:
  `impl` 'none' | 'meanstd' | 'perc', same hyper-parameters and arithmetic.

  The (offset, scale) that `__call__` and `stats` return are 0-d float32 VIEWS of
  the state buffer: valid in stream order until the next call on this object,
  which overwrites them in place (clone them to keep a value).  Input that is not
  contiguous float32 is converted first with one torch op (an allocation and a
  launch of torch's own); pass contiguous float32 to stay at one launch.
  'none' returns (0.0, 1.0) and launches nothing."""

  def __init__(self, impl, rate=0.01, limit=1e-8, perclo=5.0, perchi=95.0, debias=True):
    if impl not in ('none', 'meanstd', 'perc'):
      raise NotImplementedError(impl)
    self.impl, self.rate, self.limit = impl, rate, limit
    self.perclo, self.perchi, self.debias = perclo, perchi, debias
    self._buffer = None
    self._pending = {}          # a checkpoint loaded before the device is known
    self._current = False       # words 3-4 hold (offset, scale) of words 0-2: `latest`
    if impl != 'none':
      self._config = _lib.NormalizeConfig(
          _IMPLS[impl], int(bool(debias)), float(rate), float(limit), float(perclo), float(perchi))
      self._config_ptr = C.addressof(self._config)

  # ------------------------------------------------------------------ state --

  def _state(self, device=None):
    if self._buffer is None:
      if device is None:
        if not torch.cuda.is_available():
          raise RuntimeError(
              'DeviceNormalize keeps its statistics in device memory and updates them with a HIP '
              'kernel: it needs a GPU (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())
      host = torch.zeros(5, dtype=torch.float32)
      for index, name in enumerate(_WORDS[self.impl] + ('corr',)):
        host[index] = float(self._pending.get(name, 0.0))
      self._pending = {}
      self._buffer = host.to(device)
      self._ptr = self._buffer.data_ptr()
      self._stats = (self._buffer[3], self._buffer[4])
    return self._buffer

  def _input(self, x, name='x'):
    if not (torch.is_tensor(x) and x.is_cuda):
      raise RuntimeError(
          f'DeviceNormalize runs as a HIP kernel: `{name}` must be a CUDA tensor (no CPU fallback)')
    buffer = self._state(x.device)
    if x.device != buffer.device:
      raise ValueError(f'DeviceNormalize: `{name}` is on {x.device}, the statistics on {buffer.device}')
    if x.dtype != torch.float32 or not x.is_contiguous():
      x = x.detach().to(torch.float32, memory_format=torch.contiguous_format)   # one op: cast and pack
    return x

  def _launch(self, x, update, sub=None, out=None):
    # (raw_stream also makes the buffer's device the thread's current HIP device:
    # the launch goes where the state lives, whatever device was current)
    fast.emb_normalize(
        self._config_ptr, None if x is None else x.data_ptr(), 0 if x is None else x.numel(),
        self._ptr, int(update), None if sub is None else sub.data_ptr(),
        None if out is None else out.data_ptr(), _lib.raw_stream(self._buffer.device))
    self._current = True

  # -------------------------------------------------------------- interface --

  def __call__(self, x, update=True):
    """One launch: (with `update`) the statistics take one step from `x`, then
    (offset, scale) -- views of the state buffer, see the class docstring."""
    if self.impl == 'none':
      return 0.0, 1.0
    if not update:      # x only names the device (as `like` of distributed.Normalize.stats): it is not read
      if torch.is_tensor(x) and x.is_cuda and x.device != self._state(x.device).device:
        raise ValueError(f'DeviceNormalize: `x` is on {x.device}, the statistics on {self._buffer.device}')
      return self.stats()
    self._launch(self._input(x), True)
    return self._stats

  def update(self, x):
    self(x, update=True)

  def stats(self):
    """(offset, scale) recomputed from the running statistics: one launch that
    reads no input."""
    if self.impl == 'none':
      return 0.0, 1.0
    self._state()
    self._launch(None, False)
    return self._stats

  def latest(self):
    """`stats()` without its launch where the last launch on this object already
    left (offset, scale) of the present statistics in the state buffer (every
    launch does; a loaded checkpoint or a fresh object does not: then `stats()`)."""
    if self.impl == 'none' or not self._current:
      return self.stats()
    return self._stats

  def fused(self, device):
    """(config address, state address) for a launch that runs this normaliser's
    step inside another kernel (`scans.ppo_targets`): the kernel leaves the state
    words as `emb_normalize` would, (offset, scale) included.  'none' has
    neither: (None, None), which such a launch reads as "no normaliser"."""
    if self.impl == 'none':
      return None, None
    self._state(device)
    if self._buffer.device != device:
      raise ValueError(f'DeviceNormalize: the statistics are on {self._buffer.device}, the launch on {device}')
    self._current = True
    return self._config_ptr, self._ptr

  def normalize(self, x, sub=None, out=None, update=True):
    """(x - offset) / scale, or (x - sub) / scale with `sub` (DreamerV3:
    (ret - value) / scale), written by the same launch that updates the
    statistics.  `out`: the caller's contiguous float32 tensor of x's shape (it
    may be x itself); without it the result is allocated.  'none' is x, or
    x - sub, by torch."""
    if self.impl == 'none':
      result = x if sub is None else x - sub
      if out is None:
        return result
      out.copy_(result)
      return out
    x = self._input(x)
    if sub is not None:
      sub = self._input(sub, 'sub')
      if sub.shape != x.shape:
        raise ValueError(f'DeviceNormalize.normalize: sub {tuple(sub.shape)} != x {tuple(x.shape)}')
    if out is None:
      out = torch.empty_like(x)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape
          or out.device != x.device or not out.is_contiguous()):
      raise ValueError(
          f'DeviceNormalize.normalize(out=): needs a contiguous float32 {tuple(x.shape)} tensor on {x.device}')
    self._launch(x, update, sub, out)
    return out

  # ------------------------------------------------------------ checkpoints --

  def state_dict(self):
    """The running statistics under the names of `distributed.Normalize.state`
    ('mean', 'sqrs' | 'lo', 'hi'; 'corr' with debias): 0-d float32 copies on the
    device (no synchronisation)."""
    if self.impl == 'none':
      return {}
    names = _WORDS[self.impl] + (('corr',) if self.debias else ())
    if self._buffer is None:
      return {name: torch.tensor(float(self._pending.get(name, 0.0)), dtype=torch.float32) for name in names}
    copy = self._buffer[:3].clone()
    return {name: copy[index] for index, name in enumerate(names)}

  def load_state_dict(self, state):
    """Takes `state_dict()` of this class or `distributed.Normalize.state`
    (tensors or numbers; a missing statistic starts at zero)."""
    if self.impl == 'none':
      return
    names = _WORDS[self.impl] + ('corr',)
    values = {name: state[name] for name in names if name in state}
    if self._buffer is None:
      device = next((v.device for v in values.values() if torch.is_tensor(v) and v.is_cuda), None)
      if device is None:
        self._pending = {name: float(v) for name, v in values.items()}
        return
      self._state(device)
    words = [values.get(name, 0.0) for name in names]
    self._current = False
    if all(torch.is_tensor(v) for v in words):      # device to device, in stream order
      self._buffer[:3].copy_(torch.stack([v.detach().to(self._buffer.device, torch.float32).reshape(()) for v in words]))
    else:
      self._buffer[:3].copy_(torch.tensor([float(v) for v in words], dtype=torch.float32))
