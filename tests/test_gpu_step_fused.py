"""The device env's step, the obs stack and the early insert in one launch
(emb_synth_env_step_fused; Driver + `stacks_obs_in_step`) against the same
Driver with EMB_STEP_FUSED=0, the two-launch form: every policy batch, every env
output, sampled batches drawn with equal seeds (the stored actions among them),
byte for byte.  The reference runs once, in a child process (knobs are read once
per process), for all cases.  Need a GPU.

    python -m tests.test_gpu_step_fused OUT.npz      the child: every case -> OUT.npz
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 16          # episode_len=3: resets, masked and carried actions all occur; chunksize=4: rows roll over
TWICE, SKIP, OTHER = 9, 10, 11      # steps at which the policy stacks twice / not at all / into another tensor

# name: (envs, frame shape, policy dtype, env ring, sink[, layout])
CASES = {
    'one_block_bf16': (3, (8, 8, 4), torch.bfloat16, 4, 'replay'),
    'one_block_f16_same_layout': (3, (8, 8, 4), torch.float16, 4, 'replay', 'same'),
    'seven_blocks_bf16': (2, (84, 84, 4), torch.bfloat16, 4, 'replay'),
    'seven_blocks_f32_ring1': (2, (84, 84, 4), torch.float32, 1, 'replay'),
    'one_block_u8_ring1': (3, (8, 8, 4), torch.uint8, 1, 'replay'),
    'one_block_f32': (3, (8, 8, 4), torch.float32, 4, 'replay'),
    'no_replay': (3, (8, 8, 4), torch.bfloat16, 4, 'none'),
    'other_sink': (3, (8, 8, 4), torch.bfloat16, 4, 'callable'),
}


def _bytes(t):
  return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def run_case(name):
  """-> ({array name: bytes}, fused steps per step index)."""
  import embodied_amd as emb
  from embodied_amd.envs import synthetic
  n, shape, dtype, ring, sink = CASES[name][:5]
  layout = CASES[name][5] if len(CASES[name]) > 5 else 'channels_first'
  from embodied_amd import _lib
  env = synthetic.SyntheticBatchEnv(n, shape=shape, episode_len=3, ring=ring)
  driver = emb.Driver(batch_env=env, device='cuda')
  rep = None
  seen = []
  if sink == 'replay':
    rep = emb.Replay(length=3, capacity=64, chunksize=4, seed=0)
    driver.on_step(rep.add)
  elif sink == 'callable':
    driver.on_step(lambda tran, worker, **kw: seen.append(int(tran['action'])))
  h, w, c = shape
  scale = 1.0 if dtype is torch.uint8 else 1 / 255
  bshape = (n, c, h, w) if layout == 'channels_first' else (n, h, w, c)
  staging = [torch.zeros(bshape, dtype=dtype, device='cuda') for _ in range(2)]
  other = torch.zeros(bshape, dtype=dtype, device='cuda')
  out, fused, tick = {}, [], [0]
  # Every launch of a Driver step goes through one of these entry points, one
  # launch per call: counted at the binding (with the library's own counters of
  # fused steps and obs_stack_insert launches beside them).
  calls = {}
  names = ('emb_synth_env_step', 'emb_synth_env_step_masked', 'emb_obs_stack', 'emb_mask_actions')
  saved = {k: getattr(_lib.fast, k) for k in names}

  def counted(k):
    def call(*args):
      calls[k] = calls.get(k, 0) + 1
      return saved[k](*args)
    return call
  for k in names:
    setattr(_lib.fast, k, counted(k))
  launches = []

  def policy(carry, obs, **kw):
    t = tick[0]
    tick[0] += 1
    stack = lambda dst: emb.ops.obs_stack(
        obs['image'], layout=layout, dtype=dtype, scale=scale, out=dst)
    if t == SKIP:
      batch = None
    elif t == OTHER:
      batch = stack(other)
    else:
      # (one staging tensor per ring slot, as an agent that owns its staging has)
      batch = stack(staging[t % ring & 1])
      if t == TWICE:
        assert stack(staging[t % ring & 1]) is batch
    if batch is not None:
      out[f'batch{t}'] = _bytes(batch)
    for key, value in obs.items():
      out[f'{key}{t}'] = _bytes(value)
    act = (torch.arange(n, dtype=torch.int32, device='cuda') * 3 + t * 5) % 7 - 3
    return carry, {'action': act}, {}

  driver.reset()
  try:
    for t in range(STEPS):
      calls.clear()
      # (per step the Replay's own tallies: a call on the library handle between two
      # steps would void the predicted rows; the library's counters are read at the end)
      before = (rep.fused_steps, rep.early_inserts) if rep is not None else (0, 0)
      driver(policy, steps=n)
      after = (rep.fused_steps, rep.early_inserts) if rep is not None else (0, 0)
      lib = (after[0] - before[0], after[1] - before[1] - (after[0] - before[0]))
      fused.append(int(lib[0]))
      launches.append({'fused': int(lib[0]), 'insert': int(lib[1]),
                       'env': calls.get('emb_synth_env_step', 0) + calls.get('emb_synth_env_step_masked', 0),
                       'stack': calls.get('emb_obs_stack', 0), 'mask': calls.get('emb_mask_actions', 0)})
  finally:
    for k in names:
      setattr(_lib.fast, k, saved[k])
  out['acts'] = _bytes(driver.acts['action'])
  if rep is not None:
    # the library's launch counters: fused step launches, obs_stack_insert launches
    report = rep.profile_report('fused')
    assert (int(report[0]), int(report[1])) == (sum(fused), sum(l['insert'] for l in launches)), report
    for draw in range(3):
      for key, value in rep.sample(4).items():
        out[f'sample{draw}/{key}'] = _bytes(value)
  if seen:
    out['seen'] = np.asarray(seen, np.int64)
  return out, fused, launches


@pytest.fixture(scope='module')
def reference(tmp_path_factory):
  path = tmp_path_factory.mktemp('step_fused') / 'two_launches.npz'
  env = dict(os.environ, EMB_STEP_FUSED='0')
  res = subprocess.run([sys.executable, '-m', 'tests.test_gpu_step_fused', str(path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stderr[-3000:]
  return np.load(path)


@pytest.mark.parametrize('name', list(CASES))
def test_fused_step_stores_what_two_launches_store(reference, name):
  got, fused, launches = run_case(name)
  ring, sink = CASES[name][3], CASES[name][4]
  want = {k.split('|', 1)[1]: reference[k] for k in reference.files if k.startswith(name + '|')}
  assert int(want.pop('fused_total')) == 0            # the knob: the child never fused
  assert sorted(got) == sorted(want)
  for key in want:
    assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
  if sink != 'replay':
    assert sum(fused) == 0                            # no Replay to plan the rows: two launches as ever
    assert all(l['fused'] == 0 and l['insert'] == 0 and l['env'] == 1 for l in launches)
    return
  want_fused = expected_fused(ring)
  assert fused == [int(t in want_fused) for t in range(STEPS)], (fused, sorted(want_fused))
  assert {TWICE, SKIP, OTHER} <= want_fused        # the three odd policies meet a fused launch
  for t, l in enumerate(launches):
    if t in want_fused:
      # ONE launch: no env launch of its own, no obs_stack_insert, no obs stack --
      # but for the step whose policy stacks into another tensor: the plain kernel.
      assert (l['fused'], l['env'], l['insert']) == (1, 0, 0), (t, l)
      assert l['stack'] == (1 if t == OTHER else 0), (t, l)
    elif t >= 1:
      # TWO launches: the env's masked step (the plain one before the first
      # action) and the early insert with the obs stack.
      assert (l['fused'], l['env'], l['insert'], l['stack']) == (0, 1, 1, 0), (t, l)
    assert l['mask'] == 0, (t, l)


def expected_fused(ring):
  """The steps of `run_case` that the rules of the fused launch make ONE launch
  (defer_gate.h `Predicted`), worked out here and not taken from a run:
    * step t writes ring slot t % ring and, with chunksize 4 and every worker in
      lock step from row 0, pool row t % 4 of its chunk;
    * a slot has a step record once it went through the early insert with the
      staging tensor it is stacked into: its first visit after step 0 (step 0 has
      no early insert, the workers' chunks are not open yet);
    * the rows of step t are predicted iff step t - 1 had an early insert (fused
      or not) and did not fill its chunk's last row, (t - 1) % 4 != 3;
    * the record goes stale when the policy stacks the slot's frames into another
      tensor (step OTHER): the slot's next visit takes two launches and makes a
      new record.  A step without obs_stack (SKIP) is fused like any other -- the
      launch is made before the policy runs."""
  recorded, stale, had_insert, out = set(), set(), {}, set()
  for t in range(STEPS):
    slot = t % ring
    predicted = t >= 1 and had_insert.get(t - 1, False) and (t - 1) % 4 != 3
    if slot in recorded and slot not in stale and predicted:
      out.add(t)
      had_insert[t] = True
      if t == OTHER:
        stale.add(slot)
      continue
    had_insert[t] = t >= 1 and t != SKIP
    if had_insert[t]:
      recorded.add(slot)
      stale.discard(slot)
      if t == OTHER:
        stale.add(slot)
  return out

if __name__ == '__main__':
  arrays = {}
  for case in CASES:
    result, steps_fused, _ = run_case(case)
    for k, v in result.items():
      arrays[f'{case}|{k}'] = v
    arrays[f'{case}|fused_total'] = np.asarray(sum(steps_fused))
  np.savez(sys.argv[1], **arrays)
