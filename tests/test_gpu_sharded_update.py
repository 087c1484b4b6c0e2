"""ShardedReplay.update / .stats: agent outputs and priorities
written back across ranks (replay.py:129-149, 58-74).  World 2 and 4 run in
one process on one GPU next to ONE Replay over all envs and the oracle, all
with the same seed and history; the shards' sample all-reduce is emulated by
summing their packed buffers, the sliced update's all-gather by a hook that
concatenates the slices in rank order.  Every later sample must be bit-identical
across all of them."""
import concurrent.futures
import threading

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import scenarios
from tests.conftest import assert_same

pytestmark = pytest.mark.gpu

N_ENVS, L, CHUNK, CAP, B = 8, 5, 6, 48, 8
WIDE = 1024                      # float32: 4 KiB rows (the 16-byte wide path)


@pytest.fixture(scope='module')
def emb():
  import embodied_amd
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  return embodied_amd


def _bf16_bits(x):
  """float32 array -> the int16 bit patterns of its bfloat16 rounding (toward 0)."""
  return (np.asarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def _step(t, w):
  s = scenarios.synth_step(t, w)
  s['lat'] = (np.arange(WIDE) * 1e-3 + t + 100 * w).astype(np.float32)
  s['dyn'] = _bf16_bits(np.arange(8) * 0.25 - t + w)
  s['flag'] = np.array([(t + w) % 3, t % 7, w], np.uint8)
  return s


def _stacked(t):
  steps = [_step(t, w) for w in range(N_ENVS)]
  out = {k: torch.as_tensor(np.stack([s[k] for s in steps])).cuda() for k in steps[0]}
  out['dyn'] = out['dyn'].view(torch.bfloat16)
  return steps, out


def _np(batch):
  out = {}
  for k, v in batch.items():
    v = v.detach()
    out[k] = (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).cpu().numpy()
  return out


def _decode(stepid):
  """(B, T, 20) step ids -> (B, T) chunk uids and (B, T) indices."""
  raw = np.asarray(stepid, np.uint8)
  uid = np.zeros(raw.shape[:2], object)
  idx = np.zeros(raw.shape[:2], np.int64)
  for b in range(raw.shape[0]):
    for t in range(raw.shape[1]):
      uid[b, t] = int.from_bytes(raw[b, t, :16].tobytes(), 'big')
      idx[b, t] = int.from_bytes(raw[b, t, 16:].tobytes(), 'big')
  return uid, idx


class _Shards:
  """`world` ShardedReplays of one process; sample() merges their packed
  buffers the way the all-reduce(sum) does."""

  def __init__(self, D, world, kw):
    self.D, self.world, self.per = D, world, N_ENVS // world
    self.flats = {}
    self.shards = [
        D.ShardedReplay(L, CAP, self.per, rank=r, world=world,
                        reduce=lambda flat, r=r: self.flats.__setitem__(r, flat.clone()), **kw(r))
        for r in range(world)]

  def add(self, stacked):
    for r, shard in enumerate(self.shards):
      shard.add_batch({k: v[r * self.per:(r + 1) * self.per] for k, v in stacked.items()})

  def sample(self, batch):
    for shard in self.shards:
      shard.sample(batch)
    merged = sum(self.flats[r] for r in range(self.world))
    layout = self.D.PackedLayout(
        [(k.name, k.dtype, k.shape) for k in self.shards[0].replay._keys], batch, L)
    return layout.views(merged)

  def update_replicated(self, data):
    for shard in self.shards:
      shard.update(data)

  def update_sliced(self, data):
    n, part = self.world, len(data['stepid']) // self.world
    parts, barrier = [None] * n, threading.Barrier(n, timeout=60)

    def gather_of(r):
      def gather(flat):
        parts[r] = flat
        barrier.wait()
        return torch.cat(parts)          # rank order
      return gather

    def run(r):
      mine = {k: v[r * part:(r + 1) * part] for k, v in data.items()}
      self.shards[r].update(mine, sliced=True, gather=gather_of(r))

    with concurrent.futures.ThreadPoolExecutor(n) as pool:
      for f in [pool.submit(run, r) for r in range(n)]:
        f.result()


@pytest.mark.parametrize('prioritized', [False, True], ids=['uniform', 'prioritized'])
@pytest.mark.parametrize('world', [2, 4])
def test_sharded_update_equals_single_replay_and_oracle(emb, world, prioritized):
  from embodied_amd import distributed as D

  def selector(ns):
    if prioritized:
      return dict(selector=ns.Prioritized(exponent=0.8, initial=1.0, seed=5))
    return {}

  kw = lambda r: dict(chunksize=CHUNK, seed=5, **selector(emb.selectors))
  replicated, sliced = _Shards(D, world, kw), _Shards(D, world, kw)
  single = emb.Replay(L, CAP, **kw(0))
  ref = np_oracle.Replay(L, CAP, CHUNK, seed=5, **selector(np_oracle))
  tick = 0

  def advance(ticks):
    nonlocal tick
    for _ in range(ticks):
      steps, stacked = _stacked(tick)
      single.add_batch(stacked, list(range(N_ENVS)))
      replicated.add(stacked)
      sliced.add(stacked)
      for w, s in enumerate(steps):
        ref.add(s, w)
      tick += 1

  def draw(tag):
    want = ref.sample(B)
    s = single.sample(B)
    assert_same(_np(s), want, f'single-vs-oracle {tag}')
    a, b = replicated.sample(B), sliced.sample(B)
    assert_same(_np(a), want, f'replicated-vs-oracle {tag}')
    assert_same(_np(b), want, f'sliced-vs-oracle {tag}')
    return want, s, a, b

  advance(12)
  gen = np.random.default_rng(world)
  seen = dict(overlap=0, crossing=0, evicted=0)
  for r in range(8):
    want, s, a, b = draw(f'r{r}')
    T = L if r % 2 == 0 else L - 1                 # T = L - 1: stepid[:, 1:] (dreamerv3/agent.py:333)
    cut = L - T
    uid, idx = _decode(want['stepid'][:, cut:])
    steps = [set(zip(uid[i], idx[i])) for i in range(B)]
    seen['overlap'] += any(steps[i] & steps[j] for i in range(B) for j in range(i))
    seen['crossing'] += int(sum(len(set(u)) > 1 for u in uid))
    upd = {
        'lat': gen.standard_normal((B, T, WIDE)).astype(np.float32),
        'dyn': _bf16_bits(gen.standard_normal((B, T, 8))),
        'flag': gen.integers(0, 255, (B, T, 3), dtype=np.uint8),
        'reward': gen.standard_normal((B, T)).astype(np.float32),
    }
    if r % 3 == 2:
      upd = {'flag': upd['flag']}                  # a narrow key alone
    if prioritized:
      upd['priority'] = gen.random((B, T)).astype(np.float32) + 0.1
    if r % 3 == 1:
      advance(3)                                   # some sampled targets are evicted before the update
      seen['evicted'] += int(sum(u not in ref.blocks for u in uid[:, 0]))

    def dev(stepid):
      out = {'stepid': stepid[:, cut:]}
      for k, v in upd.items():
        v = torch.as_tensor(v).cuda()
        out[k] = v.view(torch.bfloat16) if k == 'dyn' else v
      return out

    ref.update({'stepid': want['stepid'][:, cut:], **upd})
    single.update(dev(s['stepid']))
    replicated.update_replicated(dev(a['stepid']))
    sliced.update_sliced(dev(b['stepid']))
    advance(1)
  assert seen['overlap'] and seen['crossing'] and seen['evicted'], seen
  for i in range(5):                               # later draws: the selector state agrees too
    draw(f'after{i}')
  one = single.stats()
  assert one['updates'] == ref.stats()['updates']
  for s in (replicated.shards[0].stats(), sliced.shards[-1].stats()):
    for k in ('items', 'chunks', 'streams', 'inserts', 'samples', 'updates'):
      assert s[k] == one[k], (k, s[k], one[k])
  # ram_gb: this rank's chunks only; over all ranks, the single replay's
  total = sum(sh.stats()['ram_gb'] for sh in replicated.shards)
  assert 0 < replicated.shards[0].stats()['ram_gb'] < total
  assert np.isclose(total, one['ram_gb'])


def _twin(emb, **kw):
  rep = emb.Replay(L, CAP, chunksize=CHUNK, seed=9, **kw)
  for t in range(14):
    _, stacked = _stacked(t)
    rep.add_batch(stacked, list(range(N_ENVS)))
  return rep


@pytest.mark.parametrize('overlap', [False, True], ids=['spans', 'last_writer'])
def test_grouped_update_matches_dense_update(emb, overlap):
  """emb_replay_update_grouped from a grouped buffer writes the same pool bytes
  as emb_replay_update from a dense copy: non-overlapping windows take the
  persistent span mover, repeated windows the flat mover with a row table."""
  import ctypes as C
  from embodied_amd import _lib
  dense, grouped = _twin(emb), _twin(emb)
  for a, b in zip(dense._keys, grouped._keys):
    b.pool.copy_(a.pool)                 # (rows never written hold whatever the allocator left)
  batch = dense.sample(16)
  grouped.sample(16)
  uid, idx = _decode(batch['stepid'].cpu().numpy())
  pick, used = [], set()
  for i in range(16):
    steps = set(zip(uid[i], idx[i]))
    if not steps & used:
      pick.append(i)
      used |= steps
  assert len(pick) >= 4, pick
  pick = pick[:4]
  if overlap:
    pick = [pick[0], pick[1], pick[0], pick[2]]     # window 0 twice: the later one wins
  sid = batch['stepid'][pick]
  n, T, group = len(pick), L, 2
  gen = np.random.default_rng(1)
  values = {
      'lat': torch.as_tensor(gen.standard_normal((n, T, WIDE)).astype(np.float32)).cuda(),
      'dyn': torch.as_tensor(_bf16_bits(gen.standard_normal((n, T, 8)))).cuda().view(torch.bfloat16),
      'flag': torch.as_tensor(gen.integers(0, 255, (n, T, 3), dtype=np.uint8)).cuda(),
  }
  dense.profile(True)
  grouped.profile(True)
  dense.update({'stepid': sid, **values})
  # grouped source: groups of `group` sequences, each a packed block of all keys
  from embodied_amd import distributed as D
  layout = D.PackedLayout([(k, v.dtype, v.shape[2:]) for k, v in values.items()], group, T)
  buf = torch.full((n // group, layout.nbytes), 0xCD, dtype=torch.uint8, device='cuda')
  for k, v in values.items():
    layout.view(buf, k).copy_(v.view(n // group, group, T, *v.shape[2:]))
  keys = list(values)
  ids = (C.c_int32 * 3)(*[grouped._keyid[k] for k in keys])
  ptrs = (C.c_void_p * 3)(*[buf.data_ptr() + layout.index[k][3] for k in keys])
  first = np.ascontiguousarray(sid[:, 0].cpu().numpy())
  _lib.api.emb_replay_update_grouped(
      grouped._handle, n, T, _lib.ptr(first), 3, ids, ptrs, group, layout.nbytes, grouped._stream())
  torch.cuda.synchronize()
  for k in keys:
    a, b = dense._keys[dense._keyid[k]].pool, grouped._keys[grouped._keyid[k]].pool
    assert torch.equal(a, b), k
  kernel = grouped.profile_report('update')[2]
  assert kernel == dense.profile_report('update')[2]
  assert ('flat' if overlap else 'span') in kernel, kernel
  got = {k: v.cpu() for k, v in grouped.sample(16).items()}
  want = {k: v.cpu() for k, v in dense.sample(16).items()}
  for k in want:
    assert torch.equal(got[k].view(torch.uint8) if got[k].dtype == torch.bfloat16 else got[k],
                       want[k].view(torch.uint8) if want[k].dtype == torch.bfloat16 else want[k]), k


def test_bound_owner_plans_no_foreign_window(emb):
  """A bound sharded handle skips windows outside its slot range in the gathers
  and write-backs it plans: their destination bytes stay as they were."""
  import ctypes as C
  from embodied_amd import _lib
  from embodied_amd import distributed as D
  if not hasattr(_lib.lib, 'emb_replay_bind_owner'):
    pytest.skip('the library does not export emb_replay_bind_owner')
  world, per = 2, N_ENVS // 2
  shard = D.ShardedReplay(L, CAP, per, rank=1, world=world, reduce=lambda flat: flat,
                          chunksize=CHUNK, seed=3)
  single = emb.Replay(L, CAP, chunksize=CHUNK, seed=3)
  for t in range(14):
    _, stacked = _stacked(t)
    single.add_batch(stacked, list(range(N_ENVS)))
    shard.add_batch({k: v[per:] for k, v in stacked.items()})
  rep = shard.replay
  want = single.sample(12)
  mine = (want['worker'][:, 0] // per == 1).cpu().numpy()
  assert mine.any() and not mine.all()
  # planned gather (emb_replay_sample) into sentinel-filled buffers
  outs = [torch.full((12, L, k.rowbytes), 0xAB, dtype=torch.uint8, device='cuda') for k in rep._keys]
  ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
  _lib.api.emb_replay_sample(rep._handle, 12, _lib.MODES['train'], ptrs, None, None, rep._stream())
  torch.cuda.synchronize()
  for k, o in zip(rep._keys, outs):
    w = want[k.name].contiguous().view(torch.uint8).reshape(12, L, k.rowbytes)
    assert torch.equal(o[mine], w[mine]), k.name
    assert bool((o[~mine] == 0xAB).all()), k.name
  # write-back of the whole batch: only this rank's windows land, in its own pool
  new = torch.full((12, L), -5.0, device='cuda')
  before = rep._keys[rep._keyid['reward']].pool.clone()
  shard.update({'stepid': want['stepid'], 'reward': new})
  single.update({'stepid': want['stepid'], 'reward': new})
  after = rep._keys[rep._keyid['reward']].pool
  assert not torch.equal(before, after)
  got = shard.sample(12)
  ref = single.sample(12)
  mine = (ref['worker'][:, 0] // per == 1).cpu().numpy()
  for k in ref:
    assert torch.equal(got[k][mine].cpu(), ref[k][mine].cpu()), k
