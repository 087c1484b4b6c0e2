"""The owner binding and grouped write-back entry points refuse bad arguments
with a status code (no GPU needed: nothing here launches)."""
import ctypes as C

import numpy as np


def _replay(owners):
  from embodied_amd import _lib
  rep = C.c_void_p()
  cfg = _lib.ReplayConfig(4, 10, 8, 16, 0, 0, 0, owners, 2 if owners > 1 else 0)
  assert _lib.lib.emb_replay_create(C.byref(cfg), None, C.c_uint64(0), C.byref(rep)) == 0
  return rep


def test_bind_owner_checks_the_owner():
  from embodied_amd import _lib
  raw = _lib.lib
  assert raw.emb_replay_bind_owner(None, C.c_int64(0)) < 0            # null handle
  sharded, plain = _replay(2), _replay(1)
  try:
    for owner in (0, 1, -1):                                          # -1 unbinds
      assert raw.emb_replay_bind_owner(sharded, C.c_int64(owner)) == 0
    for owner in (2, -2):
      assert raw.emb_replay_bind_owner(sharded, C.c_int64(owner)) < 0
      assert b'owner' in raw.emb_last_error()
    assert raw.emb_replay_bind_owner(plain, C.c_int64(0)) == 0
    assert raw.emb_replay_bind_owner(plain, C.c_int64(1)) < 0
  finally:
    raw.emb_replay_destroy(sharded)
    raw.emb_replay_destroy(plain)


def test_grouped_update_checks_its_layout():
  from embodied_amd import _lib
  raw = _lib.lib
  rep = _replay(1)
  sid = np.zeros((2, _lib.STEPID_BYTES), np.uint8)
  ids = (C.c_int32 * 1)(0)
  src = (C.c_void_p * 1)(sid.ctypes.data)
  try:
    def call(B, T, stepids, group, stride):
      return raw.emb_replay_update_grouped(
          rep, C.c_int64(B), C.c_int64(T), stepids, 1, ids, src, group, C.c_int64(stride), None)
    assert call(2, 0, C.c_void_p(sid.ctypes.data), 1, 256) < 0       # T < 1
    assert call(2, 3, None, 1, 256) < 0                              # no step ids
    for group, stride in ((1, 100), (-1, 256), (1, -16)):
      assert call(2, 3, C.c_void_p(sid.ctypes.data), group, stride) < 0
      assert b'groups' in raw.emb_last_error()
    assert call(0, 3, C.c_void_p(sid.ctypes.data), 1, 256) == 0     # nothing to write
  finally:
    raw.emb_replay_destroy(rep)
