"""The action mask inside the device env's step launch
(emb_synth_env_step_masked, Driver + `masks_actions_in_step`): the env still
receives `value * ~is_last` (embodied/core/driver.py:72-75), no launch of its
own makes that copy, and the stored action is the Replay's carried publish.
Everything against the numpy oracle driven by the same envs and policy, as
tests/test_gpu_early_insert.py does for the unmasked form.  Need a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests.conftest import assert_same
from tests.test_gpu_early_insert import _host, _run_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emb():
  import embodied_amd
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  return embodied_amd


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint8)


def _loop(emb, steps, act_dtype=np.float32, width=(), ring=4, episode_len=3, n=6, read_every=3,
          reset_at=(), block=1, capacity=300, extra_out=False, expect_form=True):
  """Driver + Replay + SyntheticBatchEnv in the masked form next to the oracle.
  Every `read_every`-th call `driver.acts` is read right after the call (the
  Driver settles the pending mask); on the other calls the masked buffer is left
  to the env's next step launch and looked at afterwards.  Either way the bytes
  must be raw * ~is_last in the action's dtype."""
  from embodied_amd.envs import synthetic
  shape = (8, 8, 4)
  env = synthetic.SyntheticBatchEnv(n, shape=shape, episode_len=episode_len, ring=ring)
  rep = emb.Replay(length=3, capacity=capacity, chunksize=8, seed=0)
  ref = np_oracle.Replay(3, capacity, 8, False, seed=0)
  oracle = np_oracle.Driver([synthetic.HostSyntheticEnv(e, shape=shape, episode_len=episode_len) for e in range(n)])
  oracle.on_step(ref.add)
  driver = emb.Driver(batch_env=env, device='cuda')
  driver.on_step(rep.add)
  tick = {'dev': 0, 'host': 0}
  last = {}
  stats = {'negative_zeros': 0}

  def acts_at(t):
    base = (np.arange(n * max(1, int(np.prod(width)))).reshape(n, *width) * 3 + t * 5) % 7 - 3
    return base.astype(act_dtype)           # negative values: -x * 0 = -0.0 for floats

  def policy(carry, obs, **kw):
    t = tick['dev']
    tick['dev'] += 1
    emb.ops.obs_stack(obs['image'], layout='channels_first', dtype=torch.bfloat16, scale=1 / 255)
    last['flags'] = obs['is_last'].clone()
    last['raw'] = acts_at(t)
    outs = {'feat': torch.full((n, 6), float(t), device='cuda')} if extra_out else {}
    return carry, {'action': torch.as_tensor(last['raw']).cuda()}, outs

  def host_policy(carry, obs):
    t = tick['host']
    tick['host'] += 1
    outs = {'feat': np.full((n, 6), float(t), np.float32)} if extra_out else {}
    return carry, {'action': acts_at(t)}, outs

  def expected():
    keep = ~last['flags'].cpu().numpy()
    keep = keep.reshape(keep.shape + (1,) * len(width))
    return last['raw'] * keep.astype(act_dtype)

  driver.reset()
  left = None                      # (buffer, expected bytes) the env's next launch has to produce
  pendings = 0
  for call in range(steps // block):
    if call in reset_at:
      driver.reset()
      oracle.reset()
      left = None
    driver(policy, steps=n * block)
    for _ in range(block):
      oracle.step(host_policy)
    if left is not None and block == 1:
      torch.cuda.synchronize()
      assert np.array_equal(_bits(left[0].cpu().numpy()), _bits(left[1])), f'env input after call {call}'
      left = None
    want = expected()
    if want.dtype.kind == 'f':
      stats['negative_zeros'] += int((np.signbit(want) & (want == 0)).sum())
    pendings += driver._pending is not None
    if call % read_every == 0:
      got = driver.acts['action'].cpu().numpy()
      assert got.dtype == want.dtype
      assert np.array_equal(_bits(got), _bits(want)), f'driver.acts after call {call}'
      assert driver._pending is None
    elif driver._pending is not None:
      left = (driver._acts['action'], want)
    assert len(rep) == len(ref)
    if len(ref) and call % 5 == 0:
      assert_same(_host(rep.sample(4)), ref.sample(4), f'call {call}')
  assert (pendings >= steps // block - 1) == expect_form, pendings
  assert_same(_host(rep.sample(8)), ref.sample(8), 'final')
  driver.stats = stats
  return rep, ref, driver


@pytest.mark.parametrize('online', [False, True])
@pytest.mark.parametrize('sample_every', [1, 7])
def test_env_masked_step_matches_oracle(emb, online, sample_every):
  """Every sampled batch equals the oracle's, and every publish behind an early
  insert was carried: the third launch is gone."""
  n, steps = 5, 90
  rep, ref, _ = _run_pair(emb, n, (8, 8, 4), length=4, capacity=60, chunksize=8, steps=steps,
                          online=online, stack=True, sample_every=sample_every)
  assert rep.early_inserts == steps - 1
  inline, total = rep.profile_report('carried')[:2]
  assert total >= steps - 2
  got, want = rep.stats(), ref.stats()
  for k in ('items', 'chunks', 'streams', 'inserts', 'samples'):
    assert got[k] == want[k], k
  assert_same(_host(rep.sample(6)), ref.sample(6), 'final')


@pytest.mark.parametrize('act_dtype', [np.float32, np.float16, np.int64, np.uint8])
def test_driver_acts_and_env_input_are_masked_bit_for_bit(emb, act_dtype):
  rep, ref, driver = _loop(emb, 60, act_dtype=act_dtype)
  got, want = _host(rep.sample(9)), ref.sample(9)
  assert np.array_equal(_bits(got['action']), _bits(want['action']))
  if np.dtype(act_dtype).kind == 'f':
    # -x * 0 = -0.0 was among the values compared bit for bit (the loop's own
    # expectation, numpy's multiply, produced them; a 9-window sample may miss them)
    assert driver.stats['negative_zeros'] > 0


@pytest.mark.parametrize('ring', [0, 1, 2, 4])
def test_env_output_rings(emb, ring):
  """Env e's episodes last 3 + 13 * (e % 8) steps: flags of the wrong step would
  mask the wrong action.  ring=1: `reset` aliases the flag buffer the step
  writes (the env steps on a copy, and masks with that copy)."""
  _loop(emb, 80, ring=ring, episode_len=3)
  steps = 80
  rep, ref, _ = _run_pair(emb, 6, (8, 8, 4), length=3, capacity=300, chunksize=8, steps=steps, online=False,
                          stack=True, sample_every=9, episode_len=3, ring=ring)
  assert rep.profile_report('carried')[1] >= steps - 2
  for _ in range(5):
    got, want = _host(rep.sample(16)), ref.sample(16)
    assert (want['action'][want['is_last']] == 0).all() and (want['action'] != 0).any()
    assert_same(got, want, f'ring {ring}')


def test_reset_blocks_growth_wide_rows_and_agent_outputs(emb):
  _loop(emb, 60, reset_at=(17, 18, 40))
  _loop(emb, 60, block=3, read_every=2)
  _loop(emb, 120, capacity=None)                                   # the pool grows under carried publishes
  _loop(emb, 40, width=(4, 8), act_dtype=np.float16)               # 32 elements per env: 32 lanes
  _loop(emb, 40, width=(256,), act_dtype=np.int64)                 # the widest row the launch takes
  rep, _, _ = _loop(emb, 60, extra_out=True)                       # more than one key left: nothing to carry
  assert rep.profile_report('carried')[1] == 0


def test_unsupported_action_rows_take_the_three_launch_path(emb):
  """257 elements per env: carry_supported refuses, the Driver masks as before."""
  rep, _, driver = _loop(emb, 40, width=(257,), expect_form=False)
  assert driver._env_masks and driver._pending is None
  assert rep.profile_report('carried')[1] == 0


def test_launcher_rejects_a_bad_job(emb):
  from embodied_amd import _lib
  from embodied_amd.envs import synthetic
  n = 4
  env = synthetic.SyntheticBatchEnv(n, shape=(8, 8, 4), ring=1)
  obs = env.ring[0]
  raw = torch.ones((n, 300), dtype=torch.float32, device='cuda')
  out = torch.zeros_like(raw)
  reset = torch.zeros(n, dtype=torch.bool, device='cuda')
  args = [obs[k].data_ptr() for k in ('image', 'reward', 'is_first', 'is_last', 'is_terminal')]
  args += [n, env.frame_bytes, 0, 5, reset.data_ptr(), env.counters.data_ptr(), 0]
  stream = _lib.raw_stream(env.device)
  for job, word in (((raw.data_ptr(), out.data_ptr(), 300 * 4, _lib.F32), b'256 elements'),
                    ((raw.data_ptr(), out.data_ptr(), 6, _lib.F32), b'256 elements'),       # not a whole element
                    ((raw.data_ptr(), out.data_ptr(), 4, 99), b'dtype'),
                    ((0, out.data_ptr(), 4, _lib.F32), b'mask job'),
                    ((raw.data_ptr(), 0, 4, _lib.F32), b'mask job')):
    with pytest.raises(ValueError):
      _lib.fast.emb_synth_env_step_masked(*args, *job, stream)
    assert word in _lib.lib.emb_last_error(), (job, _lib.lib.emb_last_error())
  with pytest.raises(ValueError):                      # the flags are part of the job
    _lib.fast.emb_synth_env_step_masked(*args[:9], 0, *args[10:], raw.data_ptr(), out.data_ptr(), 4, _lib.F32, stream)
  torch.cuda.synchronize()
  assert float(out.abs().sum()) == 0                   # nothing was launched
  assert _lib.api.emb_env_mask_supported.raw(256 * 8, _lib.I64) == 1
  assert _lib.api.emb_env_mask_supported.raw(257, _lib.U8) == 0


def test_far_flag_buffers(emb):
  """Flag buffers more than 2 GiB from `reward`: no 32-bit offsets, the far
  kernel takes the job by value.  Same outputs as the near form."""
  from embodied_amd import _lib
  n, frame = 5, 8 * 8 * 4
  big = torch.zeros((1 << 31) + (1 << 20), dtype=torch.uint8, device='cuda')
  far = (1 << 31) + 4096
  stream = _lib.raw_stream(big.device)
  raw = torch.tensor([-1.5, 2.0, -3.0, 4.0, -5.0], device='cuda')
  reset = torch.tensor([0, 1, 1, 0, 0], dtype=torch.bool, device='cuda')
  results = []
  for flags_at in (8192, far):
    image = torch.zeros((n, frame), dtype=torch.uint8, device='cuda')
    counters = torch.zeros((2, 2 * n), dtype=torch.int32, device='cuda')
    out = torch.full((n,), 7.0, device='cuda')
    base = big.data_ptr()
    _lib.fast.emb_synth_env_step_masked(
        image.data_ptr(), base, base + flags_at, base + flags_at + 256, base + flags_at + 512, n, frame, 0, 5,
        reset.data_ptr(), counters.data_ptr(), 0, raw.data_ptr(), out.data_ptr(), 4, _lib.F32, stream)
    torch.cuda.synchronize()
    flags = big[flags_at: flags_at + 768].clone().cpu().numpy().reshape(3, 256)[:, :n]
    results.append((image.cpu().numpy(), big[:4 * n].clone().view(torch.float32).cpu().numpy(), flags,
                    counters.cpu().numpy(), out.cpu().numpy()))
    big[flags_at: flags_at + 768].zero_()
  for a, b in zip(*results):
    assert np.array_equal(_bits(a), _bits(b))
  masked = results[1][4]
  assert np.array_equal(_bits(masked), _bits(raw.cpu().numpy() * (~reset.cpu().numpy()).astype(np.float32)))   # 2 * 0 = 0.0, -3 * 0 = -0.0
  assert results[1][2][0].tolist() == [0, 1, 1, 0, 0]              # is_first: the envs that were reset


def test_carry_knob_off_runs_the_three_launch_path():
  """EMB_CARRY_PUBLISH=0 (read once per process: a child): same results, no
  carried publish, no pending mask."""
  code = '''
import torch
import embodied_amd as emb
from tests.test_gpu_early_insert import _host, _run_pair
from tests.conftest import assert_same
rep, ref, _ = _run_pair(emb, 5, (8, 8, 4), length=4, capacity=60, chunksize=8, steps=60, online=True, stack=True)
assert rep.early_inserts == 59
assert rep.profile_report('carried')[1] == 0
assert_same(_host(rep.sample(6)), ref.sample(6), 'final')
print('ok')
'''
  out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, EMB_CARRY_PUBLISH='0'))
  assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-3000:]


def test_two_action_keys_take_the_three_launch_path(emb):
  """The env's launch masks one key: a policy with two keeps the Driver's own
  mask on every step (also once the ring of masked buffers exists)."""
  from embodied_amd.envs import synthetic
  n = 5
  env = synthetic.SyntheticBatchEnv(n, shape=(8, 8, 4), episode_len=3, ring=4)
  rep = emb.Replay(length=3, capacity=200, chunksize=8, seed=0)
  driver = emb.Driver(batch_env=env, device='cuda')
  driver.on_step(rep.add)
  last = {}

  def policy(carry, obs, **kw):
    emb.ops.obs_stack(obs['image'], layout='channels_first', dtype=torch.bfloat16, scale=1 / 255)
    last['flags'] = obs['is_last'].clone()
    last['acts'] = {'action': torch.full((n,), -2.5, device='cuda'),
                    'aux': torch.arange(1, n + 1, dtype=torch.int32, device='cuda')}
    return carry, dict(last['acts']), {}

  driver.reset()
  for _ in range(30):
    driver(policy, steps=n)
    assert driver._pending is None
    keep = ~last['flags'].cpu().numpy()
    for k, v in last['acts'].items():
      want = v.cpu().numpy() * keep.astype(v.cpu().numpy().dtype)
      assert np.array_equal(_bits(driver.acts[k].cpu().numpy()), _bits(want)), k
  assert rep.profile_report('carried')[1] == 0
