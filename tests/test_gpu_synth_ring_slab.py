"""`SyntheticBatchEnv` with an output ring: `reward` and the three flag buffers of a
ring slot are views of ONE allocation (`_alloc_slot`), so the fused step launch,
which addresses the flags as 32-bit offsets from `reward` (csrc/synth_fused.h
`offsets`), can never be refused for where the caching allocator happened to put
four tensors of their own -- in a long-lived process (a whole test session) those
can lie more than 2 GiB apart, and the slot then stays on two launches for good.
The layout, and that it changes nothing a step writes.  Need a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NARROW = ('reward', 'is_first', 'is_last', 'is_terminal')


def _env(ring, n=3, **kw):
  from embodied_amd.envs import synthetic
  return synthetic.SyntheticBatchEnv(n, shape=(8, 8, 4), episode_len=3, ring=ring, **kw)


@pytest.mark.parametrize('n', [1, 3, 64, 257])
def test_ring_slot_keeps_reward_and_flags_in_one_allocation(n):
  env = _env(4, n)
  space = env.obs_space
  spans = []
  for slot in env.ring:
    assert tuple(slot) == tuple(space)                             # the keys and their order: `_ring_ptrs` relies on it
    base = slot['reward'].untyped_storage().data_ptr()
    for name in NARROW:
      t = slot[name]
      assert t.shape == (n,) and t.is_contiguous() and t.device == env.device
      assert t.dtype == (torch.float32 if name == 'reward' else torch.bool)
      assert t.untyped_storage().data_ptr() == base, name          # one allocation
      assert t.data_ptr() % 256 == 0, name                         # each as aligned as a tensor of its own
      assert abs(t.data_ptr() - slot['reward'].data_ptr()) < 2 ** 31
      spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
    assert slot['image'].shape == (n, 8, 8, 4) and slot['image'].dtype == torch.uint8
    assert slot['image'].data_ptr() % 16 == 0
  spans.sort()
  assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))       # no two buffers of any slot overlap
  assert env._ring_ptrs == [tuple(v.data_ptr() for v in slot.values()) for slot in env.ring]
  fresh = env._alloc()                                             # without a ring: tensors of their own, as ever
  assert all(fresh[name].storage_offset() == 0 for name in fresh)


def test_ring_steps_write_what_fresh_tensors_get():
  """The same env with and without the ring, the same actions: every output of
  every step byte for byte (episode_len 3: resets and restarts occur)."""
  n = 5
  ringed, plain = _env(4, n), _env(0, n)
  for t in range(9):
    outs = []
    for env in (ringed, plain):
      acts = {'reset': torch.zeros(n, dtype=torch.bool, device='cuda'),
              'action': (torch.arange(n, dtype=torch.int32, device='cuda') * 3 + t) % 6}
      if t == 4:
        acts['reset'][1] = True
      outs.append({k: v.contiguous().view(torch.uint8).cpu().numpy().copy() for k, v in env.step(acts).items()})
    assert sorted(outs[0]) == sorted(outs[1])
    for key in outs[0]:
      assert np.array_equal(outs[0][key], outs[1][key]), (t, key)
