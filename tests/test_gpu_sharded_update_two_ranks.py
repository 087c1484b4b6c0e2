"""ShardedReplay.update(sliced=True) with a REAL all-gather: two ranks (gloo,
127.0.0.1) sharing the test box's one GPU, each passing its DP slice of the
write-back.  Later samples must equal those of one replay over all envs that
was given the whole batch."""
import hashlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


def _digest(batch):
  h = hashlib.sha256()
  for key in sorted(batch):
    h.update(key.encode() + batch[key].contiguous().view(torch.uint8).cpu().numpy().tobytes())
  return h.hexdigest()


def _worker(rank, world, port, out):
  os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                    MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  import embodied_amd as emb
  from embodied_amd import distributed as D
  from tests import scenarios
  torch.cuda.set_device(0)
  D.init('gloo')
  try:
    n, L, B = 3, 5, 6
    kw = dict(chunksize=8, seed=4)
    shard = D.ShardedReplay(L, 40, n, **kw)
    single = emb.Replay(L, 40, **kw) if rank == 0 else None

    def add(t):
      steps = [scenarios.synth_step(t, w) for w in range(n * world)]
      stacked = {k: torch.as_tensor(np.stack([s[k] for s in steps])).cuda() for k in steps[0]}
      stacked['lat'] = (torch.arange(n * world * 512, device='cuda', dtype=torch.float32)
                        .view(n * world, 512) + t)
      shard.add_batch({k: v[rank * n:(rank + 1) * n] for k, v in stacked.items()})
      if single is not None:
        single.add_batch(stacked, list(range(n * world)))

    for t in range(30):
      add(t)
    result = []
    gen = np.random.default_rng(0)                  # the same updates on every rank
    for r in range(4):
      got = shard.sample(B)
      want = single.sample(B) if single is not None else None
      T = L if r % 2 == 0 else L - 1
      upd = {'lat': torch.as_tensor(gen.standard_normal((B, T, 512)).astype(np.float32)).cuda(),
             'reward': torch.as_tensor(gen.standard_normal((B, T)).astype(np.float32)).cuda()}
      part = B // world
      shard.update({'stepid': got['stepid'][rank * part:(rank + 1) * part, L - T:],
                    **{k: v[rank * part:(rank + 1) * part] for k, v in upd.items()}}, sliced=True)
      if single is not None:
        single.update({'stepid': want['stepid'][:, L - T:], **upd})
      add(30 + r)
      got = shard.sample(B)
      want = single.sample(B) if single is not None else None
      result.append((_digest(got), _digest(want) if want is not None else None))
    out[rank] = result
  finally:
    torch.distributed.destroy_process_group()


def test_sliced_update_two_ranks_one_gpu():
  manager = mp.Manager()
  out = manager.dict()
  mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
  for i in range(4):
    want = out[0][i][1]
    assert want is not None
    assert out[0][i][0] == want, i        # rank 0 == single replay
    assert out[1][i][0] == want, i        # rank 1 holds the same batch
