"""Device-resident synthetic vector env: N simulators' worth of 84x84x4 uint8
frames generated straight into HBM by one kernel (`emb_synth_env_step`), with
the episode logic of the reference's Dummy env (embodied/envs/dummy.py:38-48).
This is the benchmark/test input of SURVEY.md 8d: real simulators are CPU code
outside the hot path.  `host_step` restates the same generator in numpy so the
frames can be verified and a CPU baseline can run on identical data.
"""
import ctypes as C

import numpy as np
import torch

from ..space import Space
from .. import _lib
from .._lib import api, fast


class SyntheticBatchEnv:

  def __init__(self, n, shape=(84, 84, 4), episode_len=1000, env0=0,
               actions=6, device='cuda', ring=0, takes_unmasked_actions=False):
    self.n = n
    # True: the Driver may hand this env the policy's actions unmasked, with
    # `reset` beside them (this generator never looks at the action of an env
    # it restarts -- nor at any other): see Driver._step_device_env.
    self.takes_unmasked_actions = bool(takes_unmasked_actions)
    # The step launch masks the actions itself (base.BatchEnv): `step(acts,
    # unmasked)` stores unmasked * ~reset into acts' tensors, in one launch with
    # the frames (emb_synth_env_step_masked).  One action key, as its act_space.
    self.masks_actions_in_step = True
    # ... and, with an output ring, may write the policy batch and the replay's
    # pool rows of the step it produces as well (base.BatchEnv): `peek_fused` /
    # `commit_fused`, emb_synth_env_step_fused.
    self.stacks_obs_in_step = ring > 0
    self.shape = tuple(shape)
    self.frame_bytes = int(np.prod(shape))
    assert self.frame_bytes % 16 == 0
    self.episode_len = episode_len
    self.env0 = env0
    self.actions = actions
    self.device = torch.device(device)
    if self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    # {count, done} per env in two generations: a step reads one and writes the
    # other, so every workgroup of an env may read the state while one writes.
    self.counters = torch.zeros((2, 2 * n), dtype=torch.int32, device=self.device)
    self.generation = 0
    # ring > 0: observations are written into `ring` rotating sets of output
    # buffers instead of fresh tensors (like vector envs that own their output
    # arrays): a returned dict is overwritten `ring` steps later.
    self.ring = [self._alloc_slot() for _ in range(ring)]
    # (the ring's tensors never change: their addresses are taken once)
    self._ring_ptrs = [tuple(v.data_ptr() for v in obs.values()) for obs in self.ring]
    self._counters_ptr = self.counters.data_ptr()
    self._calls = {}
    self._fused = {}
    self._reset_keep = None
    self.turn = 0

  def __len__(self):
    return self.n

  @property
  def obs_space(self):
    return {
        'image': Space(np.uint8, self.shape),
        'reward': Space(np.float32),
        'is_first': Space(bool),
        'is_last': Space(bool),
        'is_terminal': Space(bool),
    }

  @property
  def act_space(self):
    return {
        'reset': Space(bool),
        'action': Space(np.int32, (), 0, self.actions),
    }

  def _alloc(self):
    n, dev = self.n, self.device
    return {
        'image': _lib.empty((n, *self.shape), torch.uint8, dev),
        'reward': _lib.empty((n,), torch.float32, dev),
        'is_first': _lib.empty((n,), torch.bool, dev),
        'is_last': _lib.empty((n,), torch.bool, dev),
        'is_terminal': _lib.empty((n,), torch.bool, dev),
    }

  def _alloc_slot(self):
    """A ring slot's output set: as `_alloc`, but `reward` and the three flag
    buffers are views of ONE allocation, each at a multiple of 256 bytes.  The
    fused step launch addresses the flags as 32-bit offsets from `reward`
    (csrc/synth_fused.h `offsets`); four tensors of their own lie wherever the
    caching allocator has a free block, which in a long-lived process can be
    more than 2 GiB apart -- the launch is then refused for that slot for good."""
    n, dev = self.n, self.device
    pitch = lambda size: -(-size // 256) * 256
    at_flags = pitch(4 * n)
    slab = _lib.empty((at_flags + 3 * pitch(n),), torch.uint8, dev)
    flag = lambda k: slab[at_flags + k * pitch(n): at_flags + k * pitch(n) + n].view(torch.bool)
    return {
        'image': _lib.empty((n, *self.shape), torch.uint8, dev),
        'reward': slab[:4 * n].view(torch.float32),
        'is_first': flag(0),
        'is_last': flag(1),
        'is_terminal': flag(2),
    }

  def step(self, acts, unmasked=None):
    """One step of all envs.  `unmasked` (masks_actions_in_step): the policy's
    raw actions by key -- the launch stores `unmasked[k] * ~acts['reset']` into
    `acts[k]` (the mask of driver.py:72-75, with the same flags the episode logic
    restarts on) and the env sees only that product."""
    n, dev = self.n, self.device
    reset = acts['reset']
    job = None
    if unmasked is not None:
      (name, raw), = unmasked.items()
      out = acts[name]
      code = _DTYPE_CODE[raw.dtype]
      assert (raw.dtype == out.dtype and raw.shape == out.shape and raw.shape[0] == n
              and raw.is_contiguous() and out.is_contiguous() and raw.device == out.device == dev), name
      job = (raw.data_ptr(), out.data_ptr(), raw.numel() // n * raw.element_size(), code)
    if self.ring:
      turn = self.turn
      obs = dict(self.ring[turn])
      self.turn = (turn + 1) % len(self.ring)
      # The Driver passes the previous step's is_last as `reset`: with an output
      # ring the launch's arguments repeat with the ring (and the counters'
      # generation) -- remembered per (turn, generation) while `reset` is the
      # same tensor object.  The mask job is new every step (the policy's action
      # tensor) and is added to the remembered arguments.
      cached = self._calls.get((turn, self.generation))
      if cached is not None and cached[0] is reset:
        if job is None:
          fast.emb_synth_env_step(*cached[1], _lib.raw_stream(dev))
        else:
          fast.emb_synth_env_step_masked(*cached[1], *job, _lib.raw_stream(dev))
        self.generation ^= 1
        return obs
      image, reward, is_first, is_last, is_terminal = self._ring_ptrs[turn]
    else:
      turn = -1
      obs = self._alloc()
      image, reward, is_first, is_last, is_terminal = (v.data_ptr() for v in obs.values())
    reset_ptr = reset.data_ptr()
    if reset_ptr == is_last or reset_ptr == is_first or reset_ptr == is_terminal:
      # `reset` is a flag buffer this very step writes (ring=1: the Driver passes
      # the previous is_last): the workgroups that share an env's frame would
      # read it before and after workgroup 0's store -- step on a copy (the mask
      # job reads the same copy: the flags the env logic uses).
      kept = self._reset_keep
      reset = kept[1] if kept is not None and kept[0] is reset else reset.clone()
      self._reset_keep = None
      reset_ptr = reset.data_ptr()
      turn = -1                   # (a fresh copy per step: nothing to remember)
    args = (image, reward, is_first, is_last, is_terminal, n, self.frame_bytes, self.env0,
            self.episode_len, reset_ptr, self._counters_ptr, self.generation)
    if job is None:
      fast.emb_synth_env_step(*args, _lib.raw_stream(dev))
    else:
      fast.emb_synth_env_step_masked(*args, *job, _lib.raw_stream(dev))
    if turn >= 0:
      self._calls[(turn, self.generation)] = (reset, args)
    self.generation ^= 1
    return obs


  def peek_fused(self, acts, unmasked):
    """(obs, address of the emb_synth_step_t, arm) of the step that `step(acts,
    unmasked)` would make now -- the ring's next output set and the launch's
    arguments -- without making it, or None (no ring, more than one action key).
    `arm`: None, or what to call right before the launch is asked for.
    Whoever launches it (Replay.step_fused) calls `commit_fused` afterwards."""
    if not self.ring or len(unmasked) != 1:
      return None
    (name, raw), = unmasked.items()
    out, reset = acts[name], acts['reset']
    n, dev, turn = self.n, self.device, self.turn
    assert (raw.dtype == out.dtype and raw.shape == out.shape and raw.shape[0] == n
            and raw.is_contiguous() and out.is_contiguous() and raw.device == out.device == dev), name
    cached = self._fused.get((turn, self.generation))
    if cached is None or cached[0] is not reset or cached[1] is not out:
      image, reward, is_first, is_last, is_terminal = self._ring_ptrs[turn]
      # (`reset` may be a flag buffer this very step writes, ring=1: see `step`)
      aliased = reset.data_ptr() in (is_first, is_last, is_terminal)
      block = _lib.SynthStep(
          image, reward, is_first, is_last, is_terminal, n, self.frame_bytes, self.env0, self.episode_len,
          reset.data_ptr(), self._counters_ptr, 0, out.data_ptr(), raw.numel() // n * raw.element_size(),
          self.generation, _DTYPE_CODE[raw.dtype])
      cached = self._fused[(turn, self.generation)] = (reset, out, block, C.addressof(block), aliased)
    cached[2].act = raw.data_ptr()
    self._arming = (cached[2], reset) if cached[4] else None
    return dict(self.ring[turn]), cached[3], (self._arm if cached[4] else None)

  def _arm(self):
    """`reset` is a flag buffer the step about to be launched writes: it steps on
    a copy (see `step`), made only now that the launch is all but certain -- and
    kept for `step`, should the launch be refused after all."""
    block, reset = self._arming
    copy = reset.clone()
    self._reset_keep = (reset, copy)
    block.reset = copy.data_ptr()

  def commit_fused(self):
    """The step `peek_fused` described has been launched."""
    self.turn = (self.turn + 1) % len(self.ring)
    self.generation ^= 1
    if self._reset_keep is not None:
      self._reset_keep = (None, self._reset_keep[1])     # used up (kept alive for the launch)


_DTYPE_CODE = {
    torch.uint8: _lib.U8, torch.int8: _lib.I8, torch.int16: _lib.I16,
    torch.int32: _lib.I32, torch.int64: _lib.I64, torch.float16: _lib.F16,
    torch.bfloat16: _lib.BF16, torch.float32: _lib.F32,
    torch.float64: _lib.F64, torch.bool: _lib.BOOL,
}

_RAMPS = {}


def host_frame(env, count, frame_bytes):
  """Byte i of env `env`'s frame at episode step `count`:
  (env*131 + count*7 + i) & 0xFF -- a uint8 ramp plus a uint8 salt (uint8
  addition wraps modulo 256)."""
  ramp = _RAMPS.get(frame_bytes)
  if ramp is None:
    ramp = _RAMPS[frame_bytes] = (np.arange(frame_bytes, dtype=np.int64) & 0xFF).astype(np.uint8)
  salt = np.uint8((env * 131 + count * 7) & 0xFF)
  return ramp + salt


class HostSyntheticEnv:
  """One env of the same generator on the host (numpy), `Env` protocol."""

  def __init__(self, env, shape=(84, 84, 4), episode_len=1000, actions=6):
    self.env = env
    # The step launch masks the actions itself (base.BatchEnv): `step(acts,
    # unmasked)` stores unmasked * ~reset into acts' tensors, in one launch with
    # the frames (emb_synth_env_step_masked).  One action key, as its act_space.
    self.masks_actions_in_step = True
    self.shape = tuple(shape)
    self.frame_bytes = int(np.prod(shape))
    self.length = episode_len + (env % 8) * 13
    self.actions = actions
    self.count = 0
    self.done = False

  obs_space = property(lambda self: SyntheticBatchEnv.obs_space.fget(self))
  act_space = property(lambda self: SyntheticBatchEnv.act_space.fget(self))

  def step(self, action):
    restart = bool(action['reset']) or self.done
    if restart:
      self.count, self.done = 0, False
    else:
      self.count += 1
      self.done = self.count >= self.length
    return {
        'image': host_frame(self.env, self.count, self.frame_bytes).reshape(self.shape),
        'reward': np.float32(0 if restart else self.count % 7),
        'is_first': restart,
        'is_last': self.done,
        'is_terminal': self.done,
    }

  def close(self):
    pass
