"""`embodied_amd.optim.SlowModel`, `emb_slow_table`, `emb_slow_update` and the two
`_slow` update entry points as far as they go without a GPU: the declarations
and the binding, the host plan against a restatement, the refusals that happen
before any launch, how `omm` is formed, and the constructor.  CPU only."""
import ctypes as C
import itertools
import pathlib
import re

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ('emb_slow_table', 'emb_slow_update', 'emb_optim_update_slow', 'emb_optim_adam_update_slow')
COUNTS = (0, 1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 7)
BASE = 0x7f0000000000


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  from embodied_amd.optim import SlowModel                 # fails without the feature
  from tests.test_abi_symbols import declared_symbols
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES:
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [8, 6, 20, 18]
  # the 16 and 14 arguments of the plain entry points before `stream`, then slow, mix, omm, stream
  for plain, slow in (('emb_optim_update', 'emb_optim_update_slow'), ('emb_optim_adam_update', 'emb_optim_adam_update_slow')):
    assert _lib.SIGNATURES[slow][:-4] == _lib.SIGNATURES[plain][:-1]
    assert _lib.SIGNATURES[slow][-4:] == [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
  assert 'embodied/jax/utils.py:94-127' in text
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  count = len(declared_symbols())
  assert f'it exports ({count} functions)' in text
  assert f'the C ABI ({count} entry points' in (ROOT / 'README.md').read_text()
  assert emb.SlowModel is SlowModel
  kernel = (ROOT / 'embodied_amd' / 'csrc' / 'optim.hip').read_text()
  assert 'atomicAdd' not in kernel
  assert 'slow_update_kernel' in kernel
  assert emb.optim.SLOW_RECORD_BYTES == 32


def _table(addrs, counts, capacity=None, want_chunks=True):
  """emb_slow_table through the raw binding: (status, records, chunk map, n_chunks);
  the buffers come back as they were left, sentinels where nothing was written."""
  from embodied_amd import _lib
  raw = _lib.lib.emb_slow_table
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_slow_table'], C.c_int32
  addrs, counts = np.asarray(addrs, np.int64).reshape(-1, 2), np.asarray(counts, np.int64)
  need = int(sum(-(-max(int(n), 0) // 8192) for n in counts if n < 2 ** 31))
  capacity = need if capacity is None else capacity
  table = np.full((len(counts), 8), -7, np.int32)
  chunks = np.full((max(capacity, 1), 2), -7, np.int32)
  n, record = C.c_int64(-7), C.c_int64(-7)
  status = raw(addrs.ctypes.data, counts.ctypes.data, len(counts), table.ctypes.data,
               chunks.ctypes.data if want_chunks else None, capacity, C.byref(n), C.byref(record))
  assert record.value == 32
  return status, table, chunks[:capacity], n.value


def _restated(addrs, counts):
  """The plan, said again: records (dst, src, n, first_chunk, flags, head) and the chunk map."""
  records, chunks = [], []
  for i, ((dst, src), n) in enumerate(zip(addrs, counts)):
    head = ((16 - dst % 16) % 16) // 4
    vector = n > 0 and (src + 4 * head) % 16 == 0
    records.append((dst, src, n, len(chunks), 4 if vector else 0, head if vector else 0))
    chunks += [[i, off] for off in range(0, n, 8192)]
  return records, chunks


def test_table_builder_over_every_alignment():
  from embodied_amd import _lib, optim
  assert optim.CHUNK == 8192
  seen = set()
  for doff, soff in itertools.product((0, 4, 8, 12), repeat=2):
    addrs = [(BASE + 0x100000 * k + doff, 2 * BASE + 0x100000 * k + soff) for k in range(len(COUNTS))]
    status, table, chunks, n = _table(addrs, COUNTS)
    assert status == 0, _lib.lib.emb_last_error()
    records, want_chunks = _restated(addrs, COUNTS)
    assert n == len(want_chunks) == sum(-(-c // 8192) for c in COUNTS)
    assert chunks.tolist() == want_chunks
    for i, (dst, src, count, first, flags, head) in enumerate(records):
      assert table[i][:4].view(np.int64).tolist() == [dst, src]
      assert table[i][4:].tolist() == [count, first, flags, head], (doff, soff, i)
      assert bool(flags) == (count > 0 and doff == soff)
      assert head == ((16 - doff) % 16 // 4 if flags else 0)
      seen.add((bool(flags), head))
  assert seen == {(False, 0), (True, 0), (True, 1), (True, 2), (True, 3)}
  # the sizes alone, and a table without a chunk map
  status, table, chunks, n = _table([(BASE, 2 * BASE)], [8193], want_chunks=False)
  assert status == 0 and n == 2 and (chunks == -7).all() and table[0][4:].tolist() == [8193, 0, 4, 0]
  assert _table([(0, 0)], [0])[0] == 0                     # a tensor of none needs no address
  assert _table([], [])[::3] == (0, 0)


def test_table_refusals_write_nothing():
  from embodied_amd import _lib
  good = (BASE, 2 * BASE)
  bad = [('a null address', dict(addrs=[good, (0, BASE)], counts=[5, 5])),
         ('a null address', dict(addrs=[(BASE, 0)], counts=[5])),
         ('not aligned to its element', dict(addrs=[good, (BASE + 2, 2 * BASE)], counts=[5, 5])),
         ('not aligned to its element', dict(addrs=[(BASE, 2 * BASE + 1)], counts=[5])),
         ('dst and src are the same tensor', dict(addrs=[good, (BASE + 64, BASE + 64)], counts=[5, 5])),
         ('more than 2^31 - 1 elements', dict(addrs=[good, good], counts=[5, 1 << 31])),
         ('more than 2^31 - 1 elements', dict(addrs=[good], counts=[-1])),
         ('the chunk map is too small', dict(addrs=[good, (3 * BASE, 4 * BASE)], counts=[8193, 5], capacity=2))]
  for message, kw in bad:
    status, table, chunks, n = _table(**kw)
    assert status == _lib.ERR_INVALID and message.encode() in _lib.lib.emb_last_error(), message
    assert b'slow_table' in _lib.lib.emb_last_error()
    assert (table == -7).all() and (chunks == -7).all() and n == -7, message
  # the largest tensor is taken
  status, _, chunks, n = _table([good], [(1 << 31) - 1])
  assert status == 0 and n == (1 << 31) // 8192 and chunks[-1].tolist() == [0, (1 << 31) - 8192]


def test_launch_refusals_before_any_launch():
  from embodied_amd import _lib, optim
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES[1:]:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def alone(table=x, chunks=x, n=3, slow=None, mix=0.02, omm=0.98):
    return raws['emb_slow_update'](table, chunks, n, mix, omm, None)

  def laprop(slow=x, mix=0.02, omm=0.98, **kw):
    a = dict(table=x, chunks=x, n=3, partials=x, lr=1e-3, beta1=0.9, omb1=0.1, c1=0.1, beta2=0.999, omb2=0.001, c2=0.001,
             eps=1e-20, agc=0.3, pmin=1e-3, wd=0.0, nesterov=0)
    a.update(kw)
    return raws['emb_optim_update_slow'](*a.values(), slow, mix, omm, None)

  def adam(slow=x, mix=0.02, omm=0.98, **kw):
    a = dict(table=x, chunks=x, n=3, partials=x, lr=1e-3, beta1=0.9, omb1=0.1, c1=0.1, beta2=0.999, omb2=0.001, c2=0.001,
             eps=1e-7, clip=10.0, wd=0.0)
    a.update(kw)
    return raws['emb_optim_adam_update_slow'](*a.values(), slow, mix, omm, None)

  before = optim.optimizer_launches()
  nan, inf = float('nan'), float('inf')
  shared = [('mix is outside [0, 1]', dict(mix=-0.01)), ('mix is outside [0, 1]', dict(mix=1.5)),
            ('mix is outside [0, 1]', dict(mix=nan)), ('omm must be finite and in [0, 1]', dict(omm=nan)),
            ('omm must be finite and in [0, 1]', dict(omm=inf)), ('omm must be finite and in [0, 1]', dict(omm=-0.5)),
            ('omm must be finite and in [0, 1]', dict(omm=1.25))]
  for who, call, more in (
      ('slow_update', alone, [('a pointer is null', dict(table=None)), ('a pointer is null', dict(chunks=None)),
                              ('chunks is outside 0 ..', dict(n=-1)), ('chunks is outside 0 ..', dict(n=1 << 31))]),
      ('optim_update_slow', laprop, [('slow is null', dict(slow=None)), ('a pointer is null', dict(table=None)),
                                     ('lr must be finite', dict(lr=nan)), ('a beta outside', dict(beta1=1.0)),
                                     ('nesterov must be 0 or 1', dict(nesterov=2)),
                                     ('must be finite and not negative', dict(agc=-1.0))]),
      ('optim_adam_update_slow', adam, [('slow is null', dict(slow=None)), ('a pointer is null', dict(partials=None)),
                                        ('chunks is outside 1 ..', dict(n=0)), ('lr must be finite', dict(lr=inf)),
                                        ('1 - beta outside', dict(omb2=0.0)),
                                        ('must be finite and not negative', dict(clip=nan))])):
    for message, kw in shared + more:
      status = call(**kw)
      assert status == _lib.ERR_INVALID, (who, message, kw, status)
      error = _lib.lib.emb_last_error()
      assert error.startswith((who + ': ').encode()) and message.encode() in error, (who, message, error)
  # nothing to do is no error, and no launch; the bounds of mix and omm themselves are taken
  assert alone(table=None, chunks=None, n=0) == _lib.OK
  assert alone(n=0, mix=1.0, omm=0.0) == _lib.OK and alone(n=0, mix=0.0, omm=1.0) == _lib.OK
  assert laprop(n=0, table=None, chunks=None, partials=None) == _lib.OK
  assert optim.optimizer_launches() == before


def test_omm_is_formed_in_float32():
  from embodied_amd import optim
  mix, omm = optim.slow_mix(0.02)
  assert mix.dtype == omm.dtype == np.float32
  assert mix == np.float32(0.02) and omm == np.float32(1) - np.float32(0.02)
  assert (omm != np.float32(1 - 0.02)) == bool(np.float32(1) - np.float32(0.02) != np.float32(1 - 0.02))
  # over the rates a user would pick the two roundings do differ somewhere, and slow_mix is the float32 one everywhere
  rates = [k / 1000 for k in range(1, 500)] + [1.0]
  differ = 0
  for rate in rates:
    mix, omm = optim.slow_mix(rate)
    assert mix == np.float32(rate) and omm == np.float32(1) - np.float32(rate)
    assert float(np.float32(float(omm))) == float(omm)       # exact as the Python float handed to the entry points
    differ += bool(omm != np.float32(1 - rate))
  assert differ == sum(bool(np.float32(1) - np.float32(r) != np.float32(1 - r)) for r in rates) and differ > 0
  assert optim.slow_mix(1.0) == (np.float32(1), np.float32(0))


@pytest.fixture
def on_host(monkeypatch):
  """The facade over host tensors: the device check is lifted, so the composed
  path and every refusal behind it can run without a device."""
  from embodied_amd import optim
  monkeypatch.setattr(optim, '_check_param', lambda index, param: None)
  return optim


def test_constructor_refusals(on_host):
  from embodied_amd import optim
  a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
  for rate in (0.5, 1.5, -0.1, float('nan')):
    with pytest.raises(ValueError, match='rate = .* must be 1 or in'):
      on_host.SlowModel(a, b, rate=rate)
  for every in (0, -1, 2.5):
    with pytest.raises(ValueError, match='every = .* must be a whole number'):
      on_host.SlowModel(a, b, every=every)
  other = torch.nn.Sequential(torch.nn.Linear(3, 2))
  with pytest.raises(ValueError, match='differ in their parameters'):
    on_host.SlowModel(a, other)
  with pytest.raises(ValueError, match='differ in their parameters'):
    on_host.SlowModel([torch.zeros(3)], [torch.zeros(3), torch.zeros(2)])
  with pytest.raises(ValueError, match=r"parameter 0 \('weight'\) is \(2, 3\) in model and \(4, 3\) in source"):
    on_host.SlowModel(a, torch.nn.Linear(3, 4))
  with pytest.raises(ValueError, match='IS the source'):
    on_host.SlowModel(a, a)
  with pytest.raises(TypeError, match='not a torch.nn.Module or a sequence'):
    on_host.SlowModel(torch.zeros(3), torch.zeros(3))


def test_constructor_refuses_other_dtypes_and_host_tensors():
  from embodied_amd import optim
  with pytest.raises(TypeError, match='parameter 0 must be float32.*no CPU fallback'):
    optim.SlowModel(torch.nn.Linear(3, 2).double(), torch.nn.Linear(3, 2).double())
  with pytest.raises(TypeError, match='parameter 0 must be float32'):
    optim.SlowModel([torch.zeros(3)], [torch.zeros(3, dtype=torch.float64)])
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    optim.SlowModel(torch.nn.Linear(3, 2), torch.nn.Linear(3, 2))


def test_composed_path_over_host_tensors(on_host):
  """The definition, `dst.mul_(omm).add_(src * mix)`, bit for bit numpy's float32
  `mix * src + omm * dst`; the schedule; what the object forwards and carries."""
  rng = np.random.default_rng(5)
  model, source = torch.nn.Linear(7, 5), torch.nn.Linear(7, 5)
  slow = on_host.SlowModel(model, source, rate=0.02, every=2)
  assert slow.fused is True and on_host.SlowModel(model, source, fused=False).fused is False
  slow = on_host.SlowModel(model, source, rate=0.02, every=2, fused=False)
  assert all(torch.equal(d, s) for d, s in zip(model.parameters(), source.parameters()))      # _initonce
  assert slow.count == 0 and (slow.mix, slow.omm) == tuple(map(float, on_host.slow_mix(0.02)))
  mix, omm = on_host.slow_mix(0.02)
  for step in range(5):
    with torch.no_grad():
      for p in source.parameters():
        p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)))
    before = [d.detach().numpy().copy() for d in model.parameters()]
    slow.update()
    assert slow.count == step + 1
    for d, s, b in zip(model.parameters(), source.parameters(), before):
      want = mix * s.detach().numpy() + omm * b if step % 2 == 0 else b
      assert want.dtype == np.float32 and np.array_equal(d.detach().numpy().view(np.int32), want.view(np.int32)), step
  x = torch.ones(2, 7)
  assert torch.equal(slow(x), model(x)) and slow.weight is model.weight and slow.in_features == 7
  with pytest.raises(AttributeError):
    slow.no_such_thing
  state = slow.state_dict()
  assert state == {'count': 5, 'rate': 0.02, 'every': 2}
  again = on_host.SlowModel(torch.nn.Linear(7, 5), source, fused=False)
  again.load_state_dict(state)
  assert (again.count, again.rate, again.every, again.omm) == (5, 0.02, 2, slow.omm)
  # rate 1: a copy, as long as the old values are finite
  copy = on_host.SlowModel(torch.nn.Linear(7, 5), source, fused=False)
  with torch.no_grad():
    copy.model.weight.fill_(3.0)
  copy.update()
  assert torch.equal(copy.model.weight, source.weight)
