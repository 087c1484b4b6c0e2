"""`embodied_amd.outs.Normal`, `normal_policy_loss`, `philox_normal` on the GPU:
both paths against the fixture (the reference's own float64 run of imag_loss) and
against `cases.reference64`, whose autograd is the gradient oracle.  The bars are
written in tests/normal_policy_cases.py and in the host test, which measures the
float32 definition against them."""
import functools
import pathlib
import re

import numpy as np
import pytest
import torch

import embodied_amd as emb
from embodied_amd.outs import Normal, normal_policy_launches, normal_policy_loss, philox_normal
from tests import normal_policy_cases as cases

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'normal_policy.npz'
DEVICE = 'cuda'
LO, HI = cases.MINSTD, cases.MAXSTD


def to_device(array, bf16=False, grad=False):
  tensor = torch.from_numpy(np.ascontiguousarray(array)).to(DEVICE)
  if bf16:
    tensor = tensor.to(torch.bfloat16)          # exact: the array is bfloat16-rounded
  return tensor.requires_grad_() if grad else tensor


def host(tensor):
  return tensor.detach().to(torch.float32).cpu().numpy()


def run_loss(mean_raw, std_raw, act, adv, weight, kind, dims, drop, fused, gout=None, bf16=False, shape=None):
  """One call of the facade on device copies of numpy inputs (n, t[, A]); `shape`
  reshapes the leading (n, t) axes to a lead of another rank.  Numpy results."""
  lead = lambda x: x if shape is None else x.reshape(*shape, *x.shape[2:])
  m, s = (to_device(lead(x), bf16, grad=gout is not None) for x in (mean_raw, std_raw))
  kept = mean_raw.shape[1] - drop
  if shape is not None:
    adv = adv.reshape(*shape[:-1], kept) if drop else adv.reshape(shape)
    weight = weight.reshape(*shape[:-1], weight.shape[-1]) if drop else weight.reshape(shape)
    if gout is not None:
      gout = gout.reshape(adv.shape)
  out = normal_policy_loss(m, s, to_device(lead(act)), to_device(adv), to_device(weight), cases.ACTENT, kind,
                           LO, HI, dims, bool(drop), fused)
  result = {key: host(value).reshape(mean_raw.shape[0], kept) for key, value in out.items()}
  assert all(value.dtype == torch.float32 for value in out.values())
  if gout is not None:
    (out['loss'] * to_device(gout)).sum().backward()
    assert m.grad.dtype == m.dtype and s.grad.dtype == s.dtype
    result['grad_mean'], result['grad_std'] = (host(x.grad).reshape(mean_raw.shape) for x in (m, s))
  return result


def check(got, want, adv, weight, gout, drop, bf16, where):
  """Both bars; `weight` is (n, t - drop) here."""
  ratio = cases.forward_ratios(got, want, adv, weight, cases.ACTENT)
  assert ratio <= 1.0, (where, 'forward', ratio)
  worst = ratio
  if gout is not None:
    kept = got['grad_mean'].shape[1] - drop
    s = cases.row_scale(gout, weight, adv, cases.ACTENT)
    for name in ('grad_mean', 'grad_std'):
      assert not got[name][:, kept:].any(), (where, name, 'a dropped step carries a gradient')
      ratio = cases.grad_ratio(got[name][:, :kept], want[name][:, :kept], s, bf16)
      assert ratio <= 1.0, (where, name, ratio)
      worst = max(worst, ratio)
  return worst


@functools.lru_cache(maxsize=None)
def fixture_case(case, rounded):
  """(inputs, adv, weight, gout, fixture float64 outputs, reference64 with gradients) of one case."""
  c = cases.CASES[case]
  with np.load(GOLDEN) as f:
    name = cases.tag(case)
    want, adv, weight = f[f'out64_{name}'], f[f'adv_{name}'], f[f'weight_{name}']
  inp = cases.inputs(case)
  if rounded:
    inp.update(mean_raw=cases.bf16_round(inp['mean_raw']), std_raw=cases.bf16_round(inp['std_raw']))
  gout = np.random.default_rng(case).standard_normal(adv.shape).astype(np.float32)
  ref = cases.reference64(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, cases.ACTENT, c.kind,
                          1 if c.actions else 0, 1, gout)
  return inp, adv, weight, gout, want, ref


@pytest.mark.parametrize('actions', (0,) + cases.ACTIONS)
def test_fixture_cases_on_both_paths(actions):
  """Every case of the fixture, float32 and bfloat16-rounded inputs, the kernels
  and the composed path: forward against the reference's own float64 run (and
  `reference64` for the rounded inputs), gradients against `reference64`."""
  paths = (False,) if actions == 257 else (True, False)
  worst = 0.0
  for case in cases.cases_of(actions):
    c = cases.CASES[case]
    for rounded in (False, True):
      inp, adv, weight, gout, want, ref = fixture_case(case, rounded)
      if not rounded:
        ref = dict(ref, **dict(zip(cases.FIELDS, want)))         # the fixture's own values are the forward oracle
      for fused in paths:
        got = run_loss(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, c.kind, 1 if actions else 0, 1, fused,
                       gout, bf16=rounded)
        worst = max(worst, check(got, ref, adv, weight[:, :-1], gout, 1, rounded, (cases.tag(case), rounded, fused)))
  print(f'A = {actions}: {worst:.3g} of the bars')
  if actions == 257:                       # fused=None composes what the kernels do not take
    before = normal_policy_launches()
    inp, adv, weight, _, _, _ = fixture_case(cases.cases_of(257)[0], False)
    c = cases.CASES[cases.cases_of(257)[0]]
    a = run_loss(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, c.kind, 1, 1, None)
    b = run_loss(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, c.kind, 1, 1, False)
    assert all(np.array_equal(a[k], b[k]) for k in cases.FIELDS) and normal_policy_launches() == before


GEOMETRIES = ((1, 2), (3, 2), (2, 3), (37, 2), (5, 16))


def lead_shape(n, t, index):
  """Rank 1 where there is one sequence, else rank 2 and rank 3 in turn."""
  if n == 1:
    return (t,)
  return (n, 1, t) if index % 2 else None


@pytest.mark.parametrize('actions', cases.FUSED_ACTIONS)
def test_geometries_on_both_paths(actions):
  """Geometries the fixture does not hold, with and without drop_last, both
  dtypes, `weight` as (n, t) and (n, t - 1), leads of rank 1, 2 and 3, both
  heads: both paths against `reference64`."""
  rng = np.random.default_rng([actions, 5])
  combos, worst = set(), 0.0
  for g, (n, t) in enumerate(GEOMETRIES):
    for drop in (1, 0):
      turn = g + actions                  # five consecutive turns: every (dtype, layout) with a drop, both dtypes without
      bf16, cut = (bool(turn % 2), bool((turn // 2) % 2)) if drop else (not turn % 2, False)
      kind, scale = cases.HEADS[(2 * g + drop + actions) % len(cases.HEADS)]
      combos.add((bf16, cut, drop))
      mean_raw, std_raw, act = cases.raw_of(n, t, actions, kind, scale, rng)
      if bf16:
        mean_raw, std_raw = cases.bf16_round(mean_raw), cases.bf16_round(std_raw)
      kept = t - drop
      adv = rng.standard_normal((n, kept)).astype(np.float32)
      weight = (rng.random((n, kept if cut or not drop else t)) * (rng.random((n, 1)) > 0.2)).astype(np.float32)
      gout = rng.standard_normal((n, kept)).astype(np.float32)
      want = cases.reference64(mean_raw, std_raw, act, adv, weight, cases.ACTENT, kind, 1, drop, gout)
      shape = lead_shape(n, t, g)
      for fused in (True, False):
        got = run_loss(mean_raw, std_raw, act, adv, weight, kind, 1, drop, fused, gout, bf16, shape)
        worst = max(worst, check(got, want, adv, weight[:, :kept], gout, drop, bf16, (n, t, drop, kind, scale, fused)))
  assert len(combos) == 6
  print(f'A = {actions}: {worst:.3g} of the bars')


def off_alignment(tensor):
  """The same values as a contiguous view one element off the allocation's start."""
  flat = torch.empty(tensor.numel() + 1, dtype=tensor.dtype, device=tensor.device)
  view = flat[1:].view(tensor.shape)
  view.copy_(tensor)
  assert view.is_contiguous() and view.data_ptr() % 16 == tensor.element_size()
  return view


@pytest.mark.parametrize('bf16', (False, True))
@pytest.mark.parametrize('actions', (5, 65))
def test_views_one_element_off_alignment_give_the_same_bits(actions, bf16):
  rng = np.random.default_rng([actions, 9])
  n, t = 7, 3
  mean_raw, std_raw, act = cases.raw_of(n, t, actions, 'bounded', 1.0, rng)
  tensors = [to_device(cases.bf16_round(x), bf16) for x in (mean_raw, std_raw)] + [to_device(act)]
  adv, weight, gout = (to_device(rng.standard_normal(s).astype(np.float32)) for s in ((n, t - 1), (n, t), (n, t - 1)))
  assert all(x.data_ptr() % 16 == 0 for x in tensors)

  def run(inputs, adv, weight, gout):
    m, s = inputs[0].detach().requires_grad_(), inputs[1].detach().requires_grad_()
    out = normal_policy_loss(m, s, inputs[2], adv, weight, cases.ACTENT, 'bounded', LO, HI, fused=True)
    (out['loss'] * gout).sum().backward()
    return [out[k] for k in cases.FIELDS] + [m.grad, s.grad]

  aligned = run(tensors, adv, weight, gout)
  shifted = run([off_alignment(x) for x in tensors], off_alignment(adv), off_alignment(weight), off_alignment(gout))
  for a, b in zip(aligned, shifted):
    assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                       b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))
  sample = lambda inputs, eps: Normal(inputs[0], inputs[1], 'bounded', LO, HI, fused=True).sample(3, 1, eps)
  eps = philox_normal(9, 0, 0, n * t * actions).view(n, t, actions)
  assert torch.equal(sample(tensors, None), sample([off_alignment(x) for x in tensors], None))
  assert torch.equal(sample(tensors, eps), sample([off_alignment(x) for x in tensors], off_alignment(eps)))


def test_one_row_more_than_a_pass_of_the_capped_grid():
  """A = 1: 64 rows per wave, 4 waves per workgroup, `kNormalMaxBlocks` workgroups;
  one row more, so the grid stride runs and its last pass holds a single row."""
  header = (ROOT / 'embodied_amd' / 'csrc' / 'normal_policy.h').read_text()
  cap = int(re.search(r'kNormalMaxBlocks = (\d+);', header).group(1))
  n = cap * 4 * 64 + 1
  rng = np.random.default_rng(21)
  mean_raw, std_raw, act = cases.raw_of(n, 1, 1, 'bounded', 1.0, rng)
  adv, weight, gout = (rng.standard_normal((n, 1)).astype(np.float32) for _ in range(3))
  want = cases.reference64(mean_raw, std_raw, act, adv, weight, cases.ACTENT, 'bounded', 1, 0, gout)
  before = normal_policy_launches()
  got = run_loss(mean_raw, std_raw, act, adv, weight, 'bounded', 1, 0, True, gout)
  assert normal_policy_launches() == before + 2
  check(got, want, adv, weight, gout, 0, False, 'past the grid')
  assert got['loss'][-1, 0] != 0 and got['grad_std'][-1, 0, 0] != 0


@pytest.mark.parametrize('kind', ('bounded', 'logstd'))
@pytest.mark.parametrize('dims', (1, 0))
def test_logp_and_entropy_of_the_head(kind, dims):
  rng = np.random.default_rng([dims, 3])
  n, t, actions = 4, 3, 6 if dims else 0
  mean_raw, std_raw, act = cases.raw_of(n, t, actions, kind, 1.0, rng)
  ones = np.ones((n, t), np.float32)
  gout = rng.standard_normal((n, t)).astype(np.float32)
  want_lp = cases.reference64(mean_raw, std_raw, act, None, None, 0.0, kind, dims, 0, gout)      # loss = -logpi
  want_en = cases.reference64(mean_raw, std_raw, None, None, None, -1.0, kind, dims, 0, gout)    # loss = ent
  for fused in (True, False):
    both = normal_policy_loss(to_device(mean_raw), to_device(std_raw), to_device(act), to_device(ones), to_device(ones),
                              cases.ACTENT, kind, LO, HI, dims, False, fused)
    for which, want in (('logp', want_lp), ('entropy', want_en)):
      m, s = to_device(mean_raw, grad=True), to_device(std_raw, grad=True)
      head = Normal(m, s, kind, LO, HI, dims, fused)
      assert head.fused is fused
      before = normal_policy_launches()
      value = head.logp(to_device(act).double()) if which == 'logp' else head.entropy()
      (value * to_device(gout)).sum().backward()
      assert normal_policy_launches() == before + (2 if fused else 0)
      assert value.shape == (n, t) and value.dtype == torch.float32
      twin = both['logpi' if which == 'logp' else 'ent']
      if fused:
        assert torch.equal(value.detach(), twin)
      key = 'logpi' if which == 'logp' else 'ent'
      assert cases.forward_ratio(host(value), want[key], want['S']) <= 1.0
      assert cases.forward_ratio(host(twin), want[key], want['S']) <= 1.0
      sign = -1.0 if which == 'logp' else 1.0                   # d logp = -d (the oracle's loss)
      s_row = np.abs(gout.astype(np.float64))
      for name, x in (('grad_mean', m), ('grad_std', s)):
        if x.grad is None:                  # composed: the entropy does not read the mean
          assert (which, fused, name) == ('entropy', False, 'grad_mean')
          continue
        assert cases.grad_ratio(host(x.grad), sign * want[name], s_row) <= 1.0, (which, fused, name)
    head = Normal(to_device(mean_raw), to_device(std_raw), kind, LO, HI, dims, fused)
    mean64 = cases.moments64(mean_raw, std_raw, kind)[0]
    assert np.all(np.abs(host(head.pred()) - mean64) <= 1e-5 * (1 + np.abs(mean64)))
  if kind == 'bounded' and dims:
    entropy = lambda std: (0.5 * np.log(2 * np.pi * std * std) + 0.5) * actions
    assert head.minent == pytest.approx(entropy(LO)) and head.maxent == pytest.approx(entropy(HI))


def test_philox_normal_is_the_box_muller_of_the_philox_words():
  seed, offset, first, count = 0x1234_5678_9abc_def0, (1 << 40) + 5, (1 << 32) - 7, 4099
  got = host(philox_normal(seed, offset, first, count, DEVICE)).astype(np.float64)
  want = cases.box_muller64(seed, offset, first, count)
  assert np.all(np.abs(got - want) <= 1e-5 * (1 + np.abs(want)))
  assert torch.equal(philox_normal(seed, offset, first, count), philox_normal(seed, offset, first, count))
  assert torch.equal(philox_normal(seed, offset, first + 5, 16), philox_normal(seed, offset, first, 21)[5:])
  assert philox_normal(1, count=0).shape == (0,)
  draws = host(philox_normal(2024, 1, 0, 1 << 16)).astype(np.float64)
  # five and four standard errors: 1 / sqrt(2^16) = 0.0039 and sqrt(2 / 2^16) = 0.0055
  assert np.isfinite(draws).all() and abs(draws.mean()) <= 0.02 and abs(draws.var() - 1) <= 0.03


@pytest.mark.parametrize('kind,scale', (('bounded', 1.0), ('bounded', 30.0), ('logstd', 1.0)))
@pytest.mark.parametrize('actions', (0, 6, 65, 257))
def test_sample(kind, scale, actions):
  rng = np.random.default_rng([actions, 13])
  n, t = 9, 5
  mean_raw, std_raw, _ = cases.raw_of(n, t, actions, kind, scale, rng)
  mean_raw, std_raw = cases.bf16_round(mean_raw), cases.bf16_round(std_raw)      # equal in both dtypes
  dims = 1 if actions else 0
  head = lambda bf16, fused: Normal(to_device(mean_raw, bf16), to_device(std_raw, bf16), kind, LO, HI, dims, fused)
  paths = (False,) if actions == 257 else (True, False)
  mean, std = cases.moments64(mean_raw, std_raw, kind)
  # the caller's noise
  eps = rng.standard_normal(mean_raw.shape).astype(np.float32)
  want = mean + std * eps
  for fused in paths:
    for bf16 in (False, True):
      got = head(bf16, fused).sample(eps=to_device(eps))
      assert got.dtype == torch.float32 and got.shape == mean_raw.shape and not got.requires_grad
      assert np.all(np.abs(host(got) - want) <= 1e-5 * (1 + np.abs(mean) + np.abs(std * eps))), (fused, bf16)
  # the counter: one draw whatever the dtype, the path and the run
  first = head(False, paths[0]).sample(seed=77, offset=3)
  noise = host(philox_normal(77, 3, 0, mean_raw.size)).reshape(mean_raw.shape)
  assert np.all(np.abs(host(first) - (mean + std * noise)) <= 1e-5 * (1 + np.abs(mean) + np.abs(std * noise)))
  for fused in paths:
    for bf16 in (False, True):
      before = normal_policy_launches()
      again = head(bf16, fused).sample(seed=77, offset=3)
      assert normal_policy_launches() == before + 1           # fused: the sample; composed: the noise
      assert torch.equal(again, first), (fused, bf16)
  assert not torch.equal(head(False, paths[0]).sample(seed=77, offset=4), first)
  assert not torch.equal(head(False, paths[0]).sample(seed=78, offset=3), first)


POISONS = (('mean_raw', np.nan), ('std_raw', np.nan), ('act', np.nan), ('std_raw', np.inf))


def _bits(array):
  return np.ascontiguousarray(array, np.float32).view(np.int32)


@pytest.mark.parametrize('fused', (True, False))
@pytest.mark.parametrize('kind', ('bounded', 'logstd'))
def test_poisoned_rows(kind, fused):
  rng = np.random.default_rng(31)
  n, t, actions = 3, 4, 6
  mean_raw, std_raw, act = cases.raw_of(n, t, actions, kind, 1.0, rng)
  adv, gout = (rng.standard_normal((n, t - 1)).astype(np.float32) for _ in range(2))
  weight = (0.5 + rng.random((n, t))).astype(np.float32)
  base = dict(mean_raw=mean_raw, std_raw=std_raw, act=act)
  run = lambda inp: run_loss(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, kind, 1, 1, fused, gout)
  clean = run(base)
  others = np.ones((n, t - 1), bool)
  others[1, 1] = False
  for field, value in POISONS:
    for step in (1, t - 1):                                     # a kept step, the dropped step
      inp = {k: v.copy() for k, v in base.items()}
      inp[field][1, step, 2] = value
      got = run(inp)
      where = (field, value, step)
      if step == t - 1:                                         # no bit changes anywhere
        for key in cases.FIELDS + ('grad_mean', 'grad_std'):
          assert np.array_equal(_bits(got[key]), _bits(clean[key])), (where, key)
        continue
      for key in cases.FIELDS:                                  # no other row is touched
        assert np.array_equal(_bits(got[key])[others], _bits(clean[key])[others]), (where, key)
      for key in ('grad_mean', 'grad_std'):
        assert np.array_equal(_bits(got[key])[:, :-1][others], _bits(clean[key])[:, :-1][others]), (where, key)
        assert not got[key][:, -1].any()
      row = {key: got[key][1, 1] for key in cases.FIELDS}
      if np.isnan(value):
        assert np.isnan(row['logpi']) and np.isnan(row['loss']), where
        if fused:                                               # the kernels: all three and the gradient rows
          assert np.isnan(row['ent']) and np.isnan(got['grad_mean'][1, 1]).all() and np.isnan(got['grad_std'][1, 1]).all()
        else:                                                   # the definition: the entropy reads std alone
          assert np.isnan(row['ent']) == (field == 'std_raw'), where
      elif kind == 'bounded':                                   # s = +inf: std = hi, everything finite
        want = cases.reference64(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, cases.ACTENT, kind, 1, 1, gout)
        check(got, want, adv, weight[:, :-1], gout, 1, False, where)
        assert got['grad_std'][1, 1, 2] == 0
      else:                                                     # exp overflows: what the float32 definition returns
        composed = run_loss(inp['mean_raw'], inp['std_raw'], inp['act'], adv, weight, kind, 1, 1, False)
        assert row['logpi'] == -np.inf and row['ent'] == np.inf and not np.isfinite(row['loss']), (where, row)
        for key in cases.FIELDS:
          assert np.array_equal(got[key][1, 1], composed[key][1, 1], equal_nan=True), (where, key)


@pytest.mark.parametrize('fused', (True, False))
def test_bounded_stays_finite_at_raw_values_of_ten_thousand(fused):
  rng = np.random.default_rng(41)
  n, t, actions = 3, 3, 6
  mean_raw = (1e4 * rng.choice([-1.0, 1.0], (n, t, actions))).astype(np.float32)
  std_raw = (1e4 * rng.choice([-1.0, 1.0], (n, t, actions))).astype(np.float32)
  act = rng.uniform(-1, 1, (n, t, actions)).astype(np.float32)
  adv, gout = (rng.standard_normal((n, t - 1)).astype(np.float32) for _ in range(2))
  weight = np.ones((n, t), np.float32)
  want = cases.reference64(mean_raw, std_raw, act, adv, weight, cases.ACTENT, 'bounded', 1, 1, gout)
  got = run_loss(mean_raw, std_raw, act, adv, weight, 'bounded', 1, 1, fused, gout)
  assert all(np.isfinite(got[key]).all() for key in got)
  check(got, want, adv, weight[:, :-1], gout, 1, False, 'ten thousand')
  if fused:
    assert not got['grad_mean'].any()
  std = host(Normal(to_device(mean_raw), to_device(std_raw), 'bounded', LO, HI, fused=fused).sample(eps=to_device(
      np.ones_like(act)))) - np.sign(mean_raw)
  low, high = np.float32(LO), np.float32(HI - LO) + np.float32(LO)
  assert np.all(np.where(std_raw < 0, np.abs(std - low), np.abs(std - high)) <= 2e-7)


def test_launch_accounting_and_refusals():
  rng = np.random.default_rng(51)
  n, t, actions = 4, 3, 6
  mean_raw, std_raw, act = cases.raw_of(n, t, actions, 'bounded', 1.0, rng)
  adv, weight = np.ones((n, t - 1), np.float32), np.ones((n, t), np.float32)
  for fused, forward, backward in ((True, 1, 1), (None, 1, 1), (False, 0, 0)):
    m, s = to_device(mean_raw, grad=True), to_device(std_raw, grad=True)
    before = normal_policy_launches()
    out = normal_policy_loss(m, s, to_device(act), to_device(adv), to_device(weight), fused=fused)
    assert normal_policy_launches() == before + forward
    out['loss'].sum().backward()
    assert normal_policy_launches() == before + forward + backward
  # empty outputs: nothing launched, the gradient is zeros
  before = normal_policy_launches()
  m, s = to_device(mean_raw[:, :1], grad=True), to_device(std_raw[:, :1], grad=True)
  out = normal_policy_loss(m, s, to_device(act[:, :1]), to_device(adv[:, :0]), to_device(weight[:, :1]), fused=True)
  out['loss'].sum().backward()
  assert out['loss'].shape == (n, 0) and not m.grad.any() and not s.grad.any()
  none = normal_policy_loss(to_device(mean_raw[:0]), to_device(std_raw[:0]), to_device(act[:0]), to_device(adv[:0]),
                            to_device(weight[:0]))
  assert none['loss'].shape == (0, t - 1) and normal_policy_launches() == before
  # non-contiguous inputs are made contiguous; actions of any floating dtype
  wide = to_device(np.concatenate([mean_raw, std_raw], -1))
  split = normal_policy_loss(wide[..., :actions], wide[..., actions:], to_device(act).to(torch.float16).double(),
                             to_device(adv), to_device(weight), fused=True)
  whole = normal_policy_loss(to_device(mean_raw), to_device(std_raw), to_device(act).to(torch.float16).float(),
                             to_device(adv), to_device(weight), fused=True)
  assert torch.equal(split['loss'], whole['loss'])
  with pytest.raises(TypeError, match='must be floating point'):
    normal_policy_loss(to_device(mean_raw), to_device(std_raw), to_device(act).to(torch.int32), to_device(adv),
                       to_device(weight))
  too_wide = torch.zeros(2, 3, 257, device=DEVICE)
  with pytest.raises(ValueError, match=r'fused=True.*257 action dimensions'):
    normal_policy_loss(too_wide, too_wide, too_wide, torch.zeros(2, 2, device=DEVICE), torch.zeros(2, 3, device=DEVICE),
                       fused=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 action dimensions'):
    Normal(too_wide, too_wide, fused=True)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.normal_policy_loss(torch.zeros(2, 3, 6), torch.zeros(2, 3, 6), torch.zeros(2, 3, 6), torch.zeros(2, 2),
                           torch.zeros(2, 3))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.Normal(torch.zeros(2, 3, 6), torch.zeros(2, 3, 6))
