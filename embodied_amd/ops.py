"""Driver-side device ops: observation stack/transpose into the policy batch
and per-env carry rows by env id (embodied/core/driver.py:65,
embodied/jax/agent.py:173-181,230); and `stat_rows`, many small reductions in one
launch (the kernels behind `scans.imag_metrics` and `outs.total_loss`)."""
import numpy as np
import torch

from . import _lib
from ._lib import api, fast

_OUT = {torch.uint8: _lib.U8, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16,
        torch.float32: _lib.F32}


def _stream(t):
  return _lib.raw_stream(t.device)


def obs_stack(frames, env_ids=None, layout='channels_first', dtype=torch.uint8,
              scale=1.0, offset=0.0, out=None):
  """frames: uint8 (N_total, H, W, C) slab on the GPU.  Returns the policy batch
  (n, C, H, W) [channels_first] or (n, H, W, C) [same] as `dtype`, values
  `x * scale + offset` for float outputs; batch row j is env `env_ids[j]`.
  `out`: a contiguous tensor of that shape and dtype to write into (an agent
  that owns its input staging saves the allocation, ~2.5 us of host time).

  A staging buffer handed in for a frame tensor of a device env that
  `stacks_obs_in_step` may be written by that env's NEXT step launch on the same
  ring slot (emb_synth_env_step_fused builds the policy batch while it generates
  the frames): this call then returns `out` without a launch.  Do not keep other
  data in it across env steps."""
  if env_ids is None and out is not None and type(frames) is torch.Tensor:
    # The same frame tensor into the same staging tensor with the same options as
    # before (a vector env's output ring, an agent's staging buffers): both
    # passed the checks below then, and a tensor's dtype, shape, device and
    # strides do not change behind its back -- see Replay._collect.
    memo = frames.__dict__.get('_emb_stack')
    if (memo is not None and memo[0] is out and memo[1] == layout and memo[2] is dtype
        and memo[3] == scale and memo[4] == offset):
      _, _, _, scale_f, offset_f, n, pixels, c, first = memo[:9]
      tag = frames.__dict__.get('_emb_offer')
      if tag is not None:
        replay = tag()
        if replay is not None and replay._early_insert(
            frames, pixels, c, first, dtype, scale_f, offset_f, out, memo):
          return out
      fast.emb_obs_stack(
          frames.data_ptr(), None, n, pixels, c,
          _lib.LAYOUT_CHANNELS_FIRST if first else _lib.LAYOUT_SAME, _OUT[dtype],
          scale_f, offset_f, out.data_ptr(), _stream(frames))
      return out
  if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
    raise RuntimeError('obs_stack needs a uint8 CUDA tensor (no CPU fallback)')
  if not frames.is_contiguous():
    frames = frames.contiguous()
  total, h, w, c = frames.shape
  ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
  n = total if ids is None else len(ids)
  first = layout == 'channels_first'
  shape = (n, c, h, w) if first else (n, h, w, c)
  given = out is not None        # (a batch allocated here is the caller's alone: never written again)
  if out is None:
    out = _lib.empty(shape, dtype, frames.device)
  elif not (out.shape == shape and out.dtype is dtype and out.is_contiguous()
            and out.get_device() == frames.get_device()):
    raise ValueError(f'obs_stack out= must be contiguous {shape} {dtype} on {frames.device}')
  if out.numel() == 0:
    return out                       # no envs / empty frames: nothing to launch
  if ids is None and type(frames) is torch.Tensor:
    frames._emb_stack = (out, layout, dtype, float(scale), float(offset), n, h * w, c, first, given)
  tag = getattr(frames, '_emb_offer', None)
  if tag is not None and ids is None:
    # A Driver offered this step's observations to its Replay (Replay.offer):
    # the launch that builds the policy batch also writes the observation keys
    # into the step's pool rows, every frame is read once.
    replay = tag()
    if replay is not None and replay._early_insert(
        frames, h * w, c, first, dtype, float(scale), float(offset), out,
        frames.__dict__.get('_emb_stack')):
      return out
  fast.emb_obs_stack(
      frames.data_ptr(), _lib.ptr(ids), n, h * w, c,
      _lib.LAYOUT_CHANNELS_FIRST if first else _lib.LAYOUT_SAME, _OUT[dtype],
      float(scale), float(offset), out.data_ptr(), _stream(frames))
  return out


def rows_gather(table, ids):
  """out[j] = table[ids[j]] (rows are whatever follows the first axis)."""
  table = table.contiguous()
  ids = np.ascontiguousarray(ids, np.int32)
  out = torch.empty((len(ids), *table.shape[1:]), dtype=table.dtype, device=table.device)
  rowbytes = table.element_size() * int(np.prod(table.shape[1:], dtype=np.int64))
  if out.numel() == 0:
    return out
  api.emb_rows_gather(table.data_ptr(), rowbytes, _lib.ptr(ids), len(ids),
                      out.data_ptr(), _stream(table))
  return out


def rows_scatter(table, ids, rows):
  """table[ids[j]] = rows[j], in place."""
  assert table.is_contiguous()
  ids = np.ascontiguousarray(ids, np.int32)
  rows = rows.to(table.device, table.dtype).contiguous()
  rowbytes = table.element_size() * int(np.prod(table.shape[1:], dtype=np.int64))
  if rows.numel() == 0:
    return table
  api.emb_rows_scatter(table.data_ptr(), rowbytes, _lib.ptr(ids), len(ids),
                       rows.data_ptr(), _stream(table))
  return table


STAT_MODES = {None: _lib.STAT_NONE, 'none': _lib.STAT_NONE, 'mul_add': _lib.STAT_MUL_ADD,
              'sub_div': _lib.STAT_SUB_DIV}
STAT_COLUMNS = ('mean', 'std', 'absmean', 'min', 'max', 'rate')


def stat_rows_launches():
  """Kernel launches `emb_stat_rows` and `emb_mean_fill` have issued in this process."""
  return _lib.launches('stat_rows')


def stat_view(x):
  """(rows, cols, row stride) of `x` as `emb_stat_rows` reads it, or None where it
  is no such view: any contiguous tensor is one row; a 2-D tensor whose elements
  follow each other along its rows (`x[:, :-1]` of a contiguous matrix) keeps its
  rows and their stride."""
  n = x.numel()
  if x.is_contiguous():
    return 1, n, n
  if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]:
    return x.shape[0], x.shape[1], x.stride(0)
  return None


def stat_rows(entries, out=None):
  """Six statistics of every entry, one launch per `_lib.STAT_MAX_ENTRIES` of them
  (`emb_stat_rows`): -> (len(entries), 6) float32 with the columns `STAT_COLUMNS`
  = mean, std (population), mean |x|, min, max and rate = count(|x| >= 1) / n.

  An entry is a float32 CUDA tensor `x` that `stat_view` takes, or `(x, mode,
  pair)` with mode 'mul_add' | 'sub_div' and `pair` a float32 CUDA tensor whose
  first two elements are (offset, scale): the statistics are then those of
  x * scale + offset or (x - offset) / scale, and the pair is read on the device
  at the time the kernel runs (`DeviceNormalize`'s state words 3-4 go in as
  `state[3:]`).  min and max return a NaN that is there, rate never counts one.
  `out`: the caller's contiguous float32 (len(entries), 6) tensor."""
  items = []
  for entry in entries:
    x, mode, pair = entry if isinstance(entry, (tuple, list)) else (entry, None, None)
    if not (torch.is_tensor(x) and x.is_cuda):
      raise RuntimeError('stat_rows runs as a HIP kernel: pass CUDA tensors (no CPU fallback)')
    if mode not in STAT_MODES:
      raise ValueError(f"stat_rows: mode {mode!r}, needs 'none', 'mul_add' or 'sub_div'")
    view = stat_view(x)
    if x.dtype != torch.float32 or view is None:
      raise ValueError(
          f'stat_rows: needs float32 tensors that are contiguous or 2-D with unit column stride, got {x.dtype} '
          f'{tuple(x.shape)} with strides {tuple(x.stride())}')
    mode = STAT_MODES[mode]
    if mode != _lib.STAT_NONE and not (
        torch.is_tensor(pair) and pair.device == x.device and pair.dtype == torch.float32 and pair.numel() >= 2
        and pair.is_contiguous()):
      raise ValueError('stat_rows: an affine entry needs its (offset, scale) as a contiguous float32 tensor on '
                       "the entry's device")
    items.append((x, view, mode, pair))
  if not items:
    raise ValueError('stat_rows: no entries')
  dev = items[0][0].device
  if any(x.device != dev for x, _, _, _ in items):
    raise ValueError('stat_rows: the entries are on more than one device')
  shape = (len(items), _lib.STAT_VALUES)
  if out is None:
    out = _lib.empty(shape, torch.float32, dev)
  elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape
            and out.device == dev and out.is_contiguous()):
    raise ValueError(f'stat_rows(out=): needs a contiguous float32 {shape} tensor on {dev}')
  table = (_lib.StatEntry * len(items))()
  for entry, (x, (rows, cols, stride), mode, pair) in zip(table, items):
    entry.x, entry.rows, entry.cols, entry.stride, entry.mode = x.data_ptr(), rows, cols, stride, mode
    entry.affine = pair.data_ptr() if mode != _lib.STAT_NONE else None
  fast.emb_stat_rows(table, len(items), out.data_ptr(), None, _stream(out))
  return out


class CuStream:
  """A HIP stream whose kernels may use `n_cus` compute units only (from unit
  `first_cu` on; the driver deals consecutive units round-robin over the XCDs),
  as a torch stream: `with torch.cuda.stream(cs.stream): ...`.  For a learner
  whose sample gather / scans / write-back run BESIDE the Driver's latency-bound
  step kernels instead of in front of them (`emb_stream_create_on_cus`,
  include/embodied_hip.h); the replay's movers size their grids by the share."""

  def __init__(self, n_cus, first_cu=0, device=None):
    import ctypes as C
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.index is None:
      device = torch.device('cuda', torch.cuda.current_device())
    self.device, self.n_cus, self.first_cu = device, int(n_cus), int(first_cu)
    self._raw = C.c_void_p()
    with torch.cuda.device(device):
      api.emb_stream_create_on_cus(self.first_cu, self.n_cus, C.byref(self._raw))
    self.stream = torch.cuda.ExternalStream(self._raw.value, device=device)

  def close(self):
    raw, self._raw = self._raw, None
    if raw:
      self.stream.synchronize()
      api.emb_stream_destroy(raw)

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
