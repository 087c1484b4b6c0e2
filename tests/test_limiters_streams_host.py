"""Host-side pieces: limiters and numpy streams (no GPU)."""
import threading

import numpy as np
import pytest

from embodied_amd import limiters, streams
from oracle import np_oracle, refload
from tests import reference_record


def drive(lim):
  log = []
  log.append((lim.want_insert(), lim.want_sample()))
  for _ in range(3):
    lim.insert()
  while lim.want_sample():
    lim.sample()
    log.append(('s', lim.avail))
  while lim.want_insert():
    lim.insert()
    log.append(('i', lim.avail))
  log.append(lim.save())
  return log


def test_samples_per_insert_limiter():
  lim = limiters.SamplesPerInsert(samples_per_insert=2, tolerance=4, minsize=3)
  log = drive(lim)
  assert log[0] == (True, False)
  assert [x for x in log if isinstance(x, tuple) and x[0] == 's'] == [('s', -2), ('s', -3), ('s', -4)]
  assert lim.avail >= lim.max_avail
  other = limiters.SamplesPerInsert(2, 4, 3)
  other.load(lim.save())
  assert (other.avail, other.size) == (lim.avail, lim.size)


@reference_record.recorded('limiter')
def _reference_limiter():
  return drive(refload.load().limiters.SamplesPerInsert(2, 4, 3))


@pytest.mark.reference
def test_limiter_matches_reference():
  """The same drive through the reference's SamplesPerInsert (afresh where its
  tree is readable, recorded elsewhere)."""
  want = reference_record.check('limiter')
  assert reference_record.plain(drive(limiters.SamplesPerInsert(2, 4, 3))) == want


def test_wait_returns_when_predicate_turns_true():
  flag = []
  threading.Timer(0.05, lambda: flag.append(1)).start()
  waited = limiters.wait(lambda: bool(flag), 'waiting', sleep=0.005)
  assert 0.03 < waited < 1.0
  assert limiters.wait(lambda: True, 'no wait') == 0


def test_consec_numpy_matches_oracle():
  gen = np.random.default_rng(0)
  def source():
    return {'x': gen.integers(0, 9, (2, 7, 3)), 'is_first': gen.random((2, 7)) < 0.2}
  batches = [source() for _ in range(3)]
  ours = iter(streams.Consec(iter(batches), length=3, consec=2, prefix=1, contiguous=True))
  it = iter(batches)
  want = np_oracle.Consec(lambda: next(it), 3, 2, 1)
  for _ in range(6):
    a, b = next(ours), next(want)
    assert set(a) == set(b)
    for k in a:
      assert np.array_equal(a[k], b[k]) and a[k].flags['C_CONTIGUOUS']
  with pytest.raises(AssertionError):
    next(iter(streams.Consec(iter([source()]), length=3, consec=1, prefix=1, strict=True)))


def test_prefetch_propagates_errors_and_state():
  class Source:
    def __init__(self):
      self.n = 0
    def __iter__(self):
      return self
    def __next__(self):
      self.n += 1
      if self.n == 4:
        raise ValueError('boom')
      return {'n': self.n}
    def save(self):
      return self.n
    def load(self, n):
      self.n = n
  pre = iter(streams.Prefetch(Source(), lambda d: {**d, 'seen': True}))
  assert [next(pre)['n'] for _ in range(3)] == [1, 2, 3]
  assert pre.save() == 3
  with pytest.raises(RuntimeError, match='boom'):
    next(pre)


class Counting:
  """A source with state: yields {'n': 1}, {'n': 2}, ..."""

  def __init__(self):
    self.n = 0
    self.drawn = []

  def __iter__(self):
    return self

  def __next__(self):
    self.n += 1
    self.drawn.append(self.n)
    return {'n': self.n}

  def save(self):
    return self.n

  def load(self, n):
    self.n = n


@pytest.mark.parametrize('amount', [1, 3])
def test_prefetch_runs_at_most_amount_ahead_and_restores(amount):
  import time
  src = Counting()
  pre = streams.Prefetch(src, amount=amount)
  with pytest.raises(AssertionError):
    next(pre)                                   # not started
  it = iter(pre)
  assert [next(it)['n'] for _ in range(4)] == [1, 2, 3, 4]
  time.sleep(0.05)                              # let the producer run as far as it may
  assert src.drawn[-1] == 4 + amount            # exactly `amount` batches ahead
  assert pre.save() == 4                        # state of the last batch handed out
  pre.load(2)                                   # rewind: prepared batches are dropped
  assert pre.save() == 2
  assert [next(it)['n'] for _ in range(3)] == [3, 4, 5]
  assert pre.save() == 5
  with pytest.raises(AssertionError):
    iter(pre)                                   # one consumer


def test_stateless_takes_functions_and_iterators():
  calls = []
  def draw(batch, mode='train'):
    calls.append((batch, mode))
    return len(calls)
  s = streams.Stateless(draw, 16, mode='report')
  assert iter(s) is s and [next(s), next(s)] == [1, 2]
  assert calls == [(16, 'report')] * 2
  assert s.save() is None and s.load(None) is None
  assert list(zip(range(3), streams.Stateless(iter('abc')))) == [(0, 'a'), (1, 'b'), (2, 'c')]
  with pytest.raises(TypeError):
    streams.Stateless(3)
  # the shipped mains bind the arguments first (ppo/main.py:262-263): same stream
  import functools
  import embodied_amd
  bound = streams.Stateless(functools.partial(draw, 8, mode='eval'))
  assert bound.fn is draw and bound.args == (8,) and bound.kwargs == {'mode': 'eval'}
  assert next(bound) == 3 and calls[-1] == (8, 'eval')
  # ... and reach the selectors through the replay module (ppo/main.py:202)
  assert embodied_amd.replay.selectors is embodied_amd.selectors
  assert embodied_amd.replay.Replay is embodied_amd.Replay


def test_recency_selector_prefers_recent_items():
  """(The exact draws are pinned by golden `sel_recency`.)  The intent:
  draw frequency follows uprobs over age, deleted items are never returned."""
  from embodied_amd import selectors
  n = 300
  uprobs = 1.0 / np.arange(1, n + 1) ** 1.0
  sel = selectors.Recency(uprobs, seed=0)
  for key in range(n):
    sel[key] = None
  del sel[n - 1]                      # newest item evicted
  draws = np.array([sel() for _ in range(4000)])
  assert (draws != n - 1).all() and len(sel) == n - 1
  ages = (n - 1) - draws
  assert (ages == 1).mean() > (ages == 10).mean() > (ages >= 200).mean() / 100
  expected = uprobs[1] / (uprobs.sum() - uprobs[0])
  assert abs((ages == 1).mean() - expected) < 0.03
  # partially filled: ages are rescaled onto the live range
  small = selectors.Recency(uprobs, seed=1)
  for key in range(5):
    small[key] = None
  assert set(small() for _ in range(200)) <= set(range(5))


class _Numbered:
  """A restorable stream of {'x': [[k, tag]] * rows} batches."""

  def __init__(self, tag, rows=2):
    self.tag, self.rows, self.k = tag, rows, 0

  def __iter__(self):
    return self

  def __next__(self):
    self.k += 1
    return {'x': np.full((self.rows, 2), (self.k, self.tag)), 'nest': {'y': np.full(self.rows, self.k)}}

  def save(self):
    return self.k

  def load(self, k):
    self.k = k


def _zip_and_map(ns):
  zipped = iter(ns.Zip([_Numbered(10), _Numbered(20, rows=3)]))
  mapped = iter(ns.Map(_Numbered(30), lambda batch, k, scale=1: {'x': batch['x'] * scale + k}, 5, scale=2))
  out = [next(zipped) for _ in range(3)]
  state = zipped.save()
  out += [next(zipped) for _ in range(2)]
  zipped.load(state)
  out.append(next(zipped))
  out += [next(mapped), next(mapped)]
  held = mapped.save()
  next(mapped)
  mapped.load(held)
  out.append(next(mapped))
  return out, state, held


@reference_record.recorded('zip_and_map')
def _reference_zip_and_map():
  import importlib
  refload.load()
  want, wstate, wheld = _zip_and_map(importlib.import_module('embodied.core.streams'))
  return {'x': [b['x'] for b in want], 'state': wstate, 'held': wheld}


def test_zip_and_map_against_the_reference_classes():
  """streams.py:153-201.  Zip concatenates one batch per source leaf by leaf;
  Map applies a function; both checkpoint through their sources.  The same
  sequence through the reference's own classes (afresh where its tree is
  readable, recorded elsewhere)."""
  got, state, held = _zip_and_map(streams)
  assert state == [3, 3] and held == 2
  assert got[0]['x'].tolist() == [[1, 10]] * 2 + [[1, 20]] * 3 and got[0]['nest']['y'].tolist() == [1] * 5
  assert got[5]['x'][0].tolist() == [4, 10]                       # after load: the 4th batch again
  assert got[6]['x'].tolist() == [[7, 65]] * 2 and got[8]['x'][0].tolist() == [11, 65]
  want = reference_record.check('zip_and_map')
  assert want['state'] == reference_record.plain(state) and want['held'] == held
  assert len(want['x']) == len(got)
  for a, b in zip(got, want['x']):
    assert (a['x'] == np.array(b)).all()
  # torch batches are concatenated as tensors
  import torch
  class _Tensors(_Numbered):
    def __next__(self):
      return {k: (torch.from_numpy(v) if not isinstance(v, dict) else v) for k, v in super().__next__().items()}
  both = next(iter(streams.Zip([_Tensors(1), _Tensors(2)])))
  assert torch.is_tensor(both['x']) and both['x'].shape == (4, 2)
  with pytest.raises(ValueError):
    streams.Zip([_Numbered(1)])


MIXER_WEIGHTS = {'b': 3.0, 'a': 1.0}


def test_mixer_draws_sources_by_weight_and_restores():
  """streams.py:204-243 (cannot run upstream: see the class docstring): the
  source of step s is `default_rng([seed, s]).choice(p=weights / sum)` over the
  sorted keys; save / load restore the step and every source."""
  weights = dict(MIXER_WEIGHTS)
  mixer = streams.Mixer({'a': _Numbered(1), 'b': _Numbered(2)}, weights, seed=7)
  tags = [int(next(mixer)['x'][0, 1]) for _ in range(200)]
  want = [1 + int(np.random.default_rng(seed=[7, s]).choice(2, p=np.array([0.25, 0.75], np.float32)))
          for s in range(200)]
  assert tags == want and 120 < tags.count(2) < 180
  state = mixer.save()
  assert state['step'] == 200 and state['sources'] == {'a': tags.count(1), 'b': tags.count(2)}
  ahead = [next(mixer)['x'][0].tolist() for _ in range(5)]
  mixer.load(state)
  assert [next(mixer)['x'][0].tolist() for _ in range(5)] == ahead
  with pytest.raises(ValueError):
    streams.Mixer({'a': _Numbered(1)}, {'b': 1.0})
  # the reference's own Mixer (afresh where its tree is readable, recorded elsewhere)
  assert reference_record.check('mixer') == tags


@reference_record.recorded('mixer')
def _reference_mixer():
  """The reference's own Mixer with ONE token of `__next__` repaired (`np.ranodm`
  -> `np.random`, from its source at run time) and the `started` flag it asserts
  on but never sets switched on: the sources it draws, in order."""
  import importlib
  import inspect
  import textwrap
  refload.load()
  ref_streams = importlib.import_module('embodied.core.streams')
  source = textwrap.dedent(inspect.getsource(ref_streams.Mixer.__next__))
  assert source.count('np.ranodm') == 1
  scope = {}
  exec(source.replace('np.ranodm', 'np.random'), {'np': np}, scope)
  Repaired = type('RepairedMixer', (ref_streams.Mixer,), {'__next__': scope['__next__']})
  theirs = Repaired({'a': _Numbered(1), 'b': _Numbered(2)}, dict(MIXER_WEIGHTS), seed=7)
  theirs.started = True
  return [int(next(theirs)['x'][0, 1]) for _ in range(200)]


class _LendingReplay:
  """What the stream checks look at on a Replay, without a GPU."""

  def __init__(self, numpy=False, reuse=0):
    self.numpy, self._reuse, self.returned = numpy, reuse, []

  def sample(self, batch, mode='train'):
    return {'is_first': np.zeros((batch, 4), bool)}

  def recycle(self, batch):
    self.returned.append(batch)


def test_streams_refuse_setups_that_would_alias_live_batches():
  """Batches that are handed out again -- `Stateless(recycle=K)`, a replay that
  rotates `reuse_outputs=K` sets -- under a Prefetch that holds more of them
  than K allows; `recycle` over a replay that returns host copies."""
  with pytest.raises(TypeError):
    streams.Stateless(_LendingReplay(numpy=True).sample, 3, recycle=2)
  lending = streams.Stateless(_LendingReplay().sample, 3, recycle=2)
  with pytest.raises(ValueError):
    streams.Prefetch(lending, amount=1)                       # needs recycle >= 3
  streams.Prefetch(streams.Stateless(_LendingReplay().sample, 3, recycle=3), amount=1)
  rotating = streams.Stateless(_LendingReplay(reuse=2).sample, 3)
  with pytest.raises(ValueError):
    streams.Prefetch(streams.Consec(rotating, length=4, consec=1), amount=1)   # seen through Consec
  streams.Prefetch(streams.Stateless(_LendingReplay(reuse=3).sample, 3), amount=1)
  streams.Prefetch(streams.Stateless(_LendingReplay(reuse=0).sample, 3), amount=4)


def test_consec_refuses_to_window_context_only_keys():
  """`Replay(heads=)` keys hold the first K steps of the whole sampled sequence:
  cutting them per window would be wrong, silently."""
  def source():
    while True:
      yield {'is_first': np.zeros((2, 9), bool), 'obs': np.zeros((2, 9, 3)), 'dyn/deter': np.zeros((2, 1, 5))}
  stream = iter(streams.Consec(streams.Stateless(source()), length=4, consec=2, prefix=1))
  with pytest.raises(AssertionError, match='context-only'):
    next(stream)
  whole = iter(streams.Consec(streams.Stateless(source()), length=8, consec=1, prefix=1))
  assert next(whole)['dyn/deter'].shape == (2, 1, 5)        # one window = the batch: nothing is cut
