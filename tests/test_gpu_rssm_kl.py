"""`embodied_amd.outs.rssm_kl` / `OneHot`: the KL pair of RSSM.loss
(dreamerv3/rssm.py:123-132) on the kernels of csrc/onehot_kl.hip and as composed
torch ops, against the float64 run of the reference's own methods and classes
(tests/golden/rssm_kl.npz) and, for other shapes, bfloat16-rounded inputs and
the gradients, against `tests.rssm_kl_cases.reference64` (which the host test
holds against that fixture).  Need a GPU.

Bars: kl, dyn, rep and the entropies within 1e-5 + 1e-5 |want| of float64; a
gradient element within 1e-5 |g| (1 + |want|), g the row's upstream gradient
(a bfloat16 gradient: plus 2^-8 |want|, its own rounding).  The float32
definition sits inside both (tests/test_rssm_kl_host.py) except for the
gradient with unimix = 0 at logit scales >= 5, where it multiplies by
log p - log q of order 1e2 .. 1e5: there the forward bars and finite gradients
are asserted, nothing more.  tools/bench_rssm_kl.py records the kernels' worst
ratios in profiles/rssm_kl_accuracy.txt."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from embodied_amd.outs import OneHot, onehot_kl_launches, rssm_kl      # every test here fails without the feature
from embodied_amd import _lib
from tests import rssm_kl_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'rssm_kl.npz'
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
# every shape on both paths, 257 classes on the composed path alone
SHAPE_PATHS = [pytest.param(shape, fused, id=f'{shape[0]}x{shape[1]}-{"fused" if fused else "composed"}')
               for shape in cases.SHAPES for fused in (True, False) if not (fused and shape[1] > 256)]
OUTPUTS = ('dyn', 'rep', 'dyn_ent', 'rep_ent')


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def _tensor(values, kind='f32'):
  t = torch.from_numpy(np.ascontiguousarray(values)).cuda()
  return t if kind == 'f32' else t.to(torch.bfloat16)


def _host(t):
  return t.detach().float().cpu().numpy()


_DATA = {}


def _data(stoch, classes, rows, scale, kind='f32'):
  """Seeded inputs (bfloat16-rounded for kind 'bf16') and upstream gradients, made once and left unchanged."""
  key = (stoch, classes, rows, scale, kind)
  if key not in _DATA:
    rng = np.random.default_rng([stoch, classes, rows, int(scale * 10)])
    post, prior = cases.logits_of(rows, stoch, classes, scale, rng)
    if kind == 'bf16':
      post, prior = cases.bf16_round(post), cases.bf16_round(prior)
    g_dyn, g_rep = rng.standard_normal((2, rows)).astype(np.float32)
    for a in (post, prior, g_dyn, g_rep):
      a.setflags(write=False)
    _DATA[key] = dict(post=post, prior=prior, g_dyn=g_dyn, g_rep=g_rep, ref={})
  return _DATA[key]


def _ref(d, unimix, free):
  if (unimix, free) not in d['ref']:
    d['ref'][unimix, free] = cases.reference64(d['post'], d['prior'], unimix, free, d['g_dyn'], d['g_rep'])
  return d['ref'][unimix, free]


def _run(d, unimix, free, fused, kind='f32', lead=None, backward=True):
  """rssm_kl over `d` -> (outputs as numpy, grad_post, grad_prior)."""
  shape = d['post'].shape if lead is None else (*lead, *d['post'].shape[1:])
  post = _tensor(d['post'], kind).view(shape).requires_grad_()
  prior = _tensor(d['prior'], kind).view(shape).requires_grad_()
  out = rssm_kl(post, prior, unimix=unimix, free_nats=free, fused=fused)
  assert sorted(out) == sorted(OUTPUTS)
  for key in OUTPUTS:
    assert out[key].dtype == torch.float32 and out[key].shape == shape[:-2], key
  assert not out['dyn_ent'].requires_grad and not out['rep_ent'].requires_grad
  if not backward:
    return {k: _host(v).reshape(-1) for k, v in out.items()}, None, None
  g_dyn, g_rep = (_tensor(d[k]).view(shape[:-2]) for k in ('g_dyn', 'g_rep'))
  (out['dyn'] * g_dyn + out['rep'] * g_rep).sum().backward()
  assert post.grad.dtype == post.dtype and post.grad.shape == post.shape
  return ({k: _host(v).reshape(-1) for k, v in out.items()}, _host(post.grad).reshape(d['post'].shape),
          _host(prior.grad).reshape(d['post'].shape))


def _forward_ratio(out, ref):
  return max(cases.forward_ratio(out['dyn'], ref['dyn']), cases.forward_ratio(out['rep'], ref['rep']),
             cases.forward_ratio(out['dyn_ent'], ref['ent_prior']), cases.forward_ratio(out['rep_ent'], ref['ent_post']))


@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_fixture_parity(golden, shape, fused):
  """Every case of the fixture at this shape (five logit scales, unimix 0.01 and
  0) with free_nats 1 and 0, against the reference's own float64 run."""
  worst = 0.0
  for case, c in enumerate(cases.CASES):
    if (c.stoch, c.classes) != shape:
      continue
    name = cases.tag(case)
    inp = cases.inputs(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(inp))
    want = dict(zip(cases.FIELDS, golden[f'out64_{name}']))
    post, prior = _tensor(inp['post']), _tensor(inp['prior'])
    for free in cases.FREE_NATS:
      out = rssm_kl(post, prior, unimix=c.unimix, free_nats=free, fused=fused)
      loss = want['dyn_f1'] if free else want['kl']
      ratio = max(cases.forward_ratio(_host(out['dyn']), loss), cases.forward_ratio(_host(out['rep']), loss),
                  cases.forward_ratio(_host(out['rep_ent']), want['ent_post']),
                  cases.forward_ratio(_host(out['dyn_ent']), want['ent_prior']))
      assert ratio <= 1.0, (name, free, ratio)
      worst = max(worst, ratio)
  print(f'{shape} fused={fused}: {worst:.3g} of the forward bar')


def _lead(rows, flip):
  """(rows,) or a (B, T) of that many rows."""
  if not flip:
    return (rows,)
  return {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5), 37: (37, 1)}[rows]


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('shape,fused', SHAPE_PATHS)
def test_parity_with_gradients(shape, fused, kind):
  """Rows 1, 3, 4, 5, 37 (fewer than a workgroup's waves, not a multiple, many
  workgroups), leading shapes (rows,) and (B, T), both dtypes, unimix 0.01 and
  0, free_nats 1 and 0: the four outputs and both gradients against float64."""
  stoch, classes = shape
  worst = [0.0, 0.0]
  for n, rows in enumerate((1, 3, 4, 5, 37)):
    for unimix in cases.UNIMIX:
      scales = cases.SCALES if unimix else cases.GRAD_SCALES_NO_UNIMIX
      d = _data(stoch, classes, rows, scales[n % len(scales)], kind)
      for m, free in enumerate(cases.FREE_NATS):
        ref = _ref(d, unimix, free)
        out, grad_post, grad_prior = _run(d, unimix, free, fused, kind, _lead(rows, (n + m) % 2))
        ratios = (_forward_ratio(out, ref),
                  max(cases.grad_ratio(grad_post, ref['grad_post'], d['g_rep'], kind == 'bf16'),
                      cases.grad_ratio(grad_prior, ref['grad_prior'], d['g_dyn'], kind == 'bf16')))
        assert max(ratios) <= 1.0, (rows, unimix, free, ratios)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
  # unimix = 0 at a large scale: the forward bars and finite gradients, nothing more (the module docstring)
  for scale in (30.0, 1e4):
    d = _data(stoch, classes, 37, scale, kind)
    out, grad_post, grad_prior = _run(d, 0.0, 1.0, fused, kind)
    assert _forward_ratio(out, _ref(d, 0.0, 1.0)) <= 1.0
    assert np.isfinite(grad_post).all() and np.isfinite(grad_prior).all()
  print(f'{shape} {kind} fused={fused}: forward {worst[0]:.3g}, gradient {worst[1]:.3g} of their bars')


@PATHS
def test_gradient_routing(fused):
  """dyn reaches prior only, rep reaches post only; a row whose raw kl is below
  free_nats gets exactly zero on both sides."""
  d = _data(32, 24, 37, 1.0)
  ones, zeros = np.ones(37, np.float32), np.zeros(37, np.float32)

  def grads(loss_of):
    post, prior = _tensor(d['post']).requires_grad_(), _tensor(d['prior']).requires_grad_()
    out = rssm_kl(post, prior, unimix=0.01, free_nats=1.0, fused=fused)
    loss_of(out).backward()
    return out, post.grad, prior.grad

  want = cases.reference64(d['post'], d['prior'], 0.01, 1.0, ones, zeros)
  out, gpost, gprior = grads(lambda o: o['dyn'].sum())
  assert gpost is None or not gpost.any()
  assert cases.grad_ratio(_host(gprior), want['grad_prior'], ones) <= 1.0
  below = want['kl'] < 1.0
  assert below.any() and not below.all() and np.array_equal(below, np.arange(37) % 5 == 0)
  assert not gprior[torch.from_numpy(below).cuda()].any() and gprior[~torch.from_numpy(below).cuda()].any()
  want = cases.reference64(d['post'], d['prior'], 0.01, 1.0, zeros, ones)
  out, gpost, gprior = grads(lambda o: o['rep'].sum())
  assert gprior is None or not gprior.any()
  assert cases.grad_ratio(_host(gpost), want['grad_post'], ones) <= 1.0
  assert not gpost[torch.from_numpy(below).cuda()].any() and gpost[~torch.from_numpy(below).cuda()].any()
  want = cases.reference64(d['post'], d['prior'], 0.01, 1.0, ones, 0.1 * ones)
  out, gpost, gprior = grads(lambda o: (o['dyn'] + 0.1 * o['rep']).sum())
  assert cases.grad_ratio(_host(gpost), want['grad_post'], 0.1 * ones) <= 1.0
  assert cases.grad_ratio(_host(gprior), want['grad_prior'], ones) <= 1.0


def _abi_grad(post, prior, unimix, free, kl, g_rep, g_dyn, grad_post, grad_prior):
  rows, stoch, classes = post.shape
  address = lambda t: None if t is None else t.data_ptr()
  _lib.api.emb_onehot_kl_grad(
      post.data_ptr(), prior.data_ptr(), _lib.F32 if post.dtype == torch.float32 else _lib.BF16, rows, stoch, classes,
      unimix, free, kl.data_ptr(), address(g_rep), address(g_dyn), address(grad_post), address(grad_prior),
      _lib.raw_stream(post.device))


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_the_tie_gets_half_through_the_c_abi(kind):
  """A saved kl equal to free_nats: half of what a kl just above it gives, and
  zero just below -- the gradient of jnp.maximum and torch.maximum at a tie."""
  d = _data(3, 5, 5, 1.0, kind)
  post, prior = _tensor(d['post'], kind), _tensor(d['prior'], kind)
  g_rep, g_dyn = _tensor(d['g_rep']), _tensor(d['g_dyn'])
  free = 1.0
  got = {}
  for name, value in (('at', free), ('above', np.nextafter(np.float32(free), np.float32(2))),
                      ('below', np.nextafter(np.float32(free), np.float32(0)))):
    kl = torch.full((5,), float(value), device='cuda')
    got[name] = (torch.full_like(post, 7.0), torch.full_like(prior, 7.0))
    _abi_grad(post, prior, 0.01, free, kl, g_rep, g_dyn, *got[name])
  for side in (0, 1):
    above = got['above'][side].float()
    assert above.abs().min() > 0 and torch.isfinite(above).all()
    assert not got['below'][side].any()
    half = got['at'][side].float()
    if kind == 'f32':
      assert torch.equal(half * 2, above)
    else:       # each is one bfloat16 rounding of a float32 value and its half
      assert ((half * 2 - above).abs() <= 2.0 ** -7 * above.abs()).all()
  want = cases.reference64(d['post'], d['prior'], 0.01, 0.0, d['g_dyn'], d['g_rep'])     # no maximum: factor 1
  assert cases.grad_ratio(_host(got['above'][0]), want['grad_post'], d['g_rep'], kind == 'bf16') <= 1.0
  assert cases.grad_ratio(_host(got['above'][1]), want['grad_prior'], d['g_dyn'], kind == 'bf16') <= 1.0


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_null_outputs(kind):
  """With a null grad_post, grad_prior has the same bits as with both given and
  the buffer that was not handed over is untouched; the mirror image too."""
  d = _data(32, 24, 5, 1.0, kind)
  post, prior = _tensor(d['post'], kind), _tensor(d['prior'], kind)
  g_rep, g_dyn = _tensor(d['g_rep']), _tensor(d['g_dyn'])
  kl = _tensor(cases.reference64(d['post'], d['prior'], 0.01, 0.0)['kl'].astype(np.float32))
  both = (torch.full_like(post, 7.0), torch.full_like(prior, 7.0))
  _abi_grad(post, prior, 0.01, 1.0, kl, g_rep, g_dyn, *both)
  assert (both[0] != 7.0).any() and (both[1] != 7.0).any()
  only_prior = (torch.full_like(post, 7.0), torch.full_like(prior, 7.0))
  _abi_grad(post, prior, 0.01, 1.0, kl, None, g_dyn, None, only_prior[1])
  assert torch.equal(only_prior[1], both[1]) and (only_prior[0] == 7.0).all()
  only_post = (torch.full_like(post, 7.0), torch.full_like(prior, 7.0))
  _abi_grad(post, prior, 0.01, 1.0, kl, g_rep, None, only_post[0], None)
  assert torch.equal(only_post[0], both[0]) and (only_post[1] == 7.0).all()


@PATHS
def test_onehot_kl_and_entropy(fused):
  d = _data(32, 24, 37, 1.0)
  want = cases.reference64(d['post'], d['prior'], 0.01, 0.0, d['g_dyn'], d['g_dyn'])     # one g to both operands
  a, b = _tensor(d['post']).requires_grad_(), _tensor(d['prior']).requires_grad_()
  da, db = OneHot(a, 0.01, fused=fused), OneHot(b, 0.01, fused=fused)
  assert da.fused is fused
  kl = da.kl(db)
  assert kl.shape == (37,) and kl.dtype == torch.float32
  kl.backward(_tensor(d['g_dyn']))
  assert cases.forward_ratio(_host(kl), want['kl']) <= 1.0
  assert cases.grad_ratio(_host(a.grad), want['grad_post'], d['g_dyn']) <= 1.0
  assert cases.grad_ratio(_host(b.grad), want['grad_prior'], d['g_dyn']) <= 1.0
  entropy = da.entropy()
  assert not entropy.requires_grad and entropy.shape == (37,)
  assert cases.forward_ratio(_host(entropy), want['ent_post']) <= 1.0
  assert cases.forward_ratio(_host(db.entropy()), want['ent_prior']) <= 1.0
  same = _host(da.kl(OneHot(a, 0.01, fused=fused)))
  assert cases.forward_ratio(same, np.zeros(37)) <= 1.0
  # unimix = 0 and a (B, T) lead
  plain = OneHot(_tensor(d['post'])[:36].view(4, 9, 32, 24), fused=fused)
  want0 = cases.reference64(d['post'][:36], d['prior'][:36], 0.0, 0.0)
  assert plain.entropy().shape == (4, 9)
  assert cases.forward_ratio(_host(plain.entropy()).reshape(-1), want0['ent_post']) <= 1.0


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('stoch,classes', [(3, 5), (32, 24)])
def test_padding_lanes_do_not_see_their_neighbours(stoch, classes, kind):
  """Both tensors inside one allocation whose every other element is NaN: a lane
  past `classes` or a segment past `stoch` that read or counted a neighbour would
  show.  Offsets are odd, so the tensors are not aligned to anything wider than an element."""
  d = _data(stoch, classes, 5, 1.0, kind)
  n = d['post'].size
  dtype = torch.float32 if kind == 'f32' else torch.bfloat16
  room = torch.full((2 * n + 64,), float('nan'), dtype=dtype, device='cuda')
  post, prior = room[7:7 + n].view(d['post'].shape), room[n + 20 + 1:2 * n + 21].view(d['post'].shape)
  post.copy_(_tensor(d['post'], kind))
  prior.copy_(_tensor(d['prior'], kind))
  assert post.is_contiguous() and post.storage_offset() == 7 and torch.isnan(room[:7]).all()
  ref = _ref(d, 0.01, 0.0)
  post.requires_grad_(), prior.requires_grad_()
  out = rssm_kl(post, prior, unimix=0.01, free_nats=0.0, fused=True)
  (out['dyn'] * _tensor(d['g_dyn']) + out['rep'] * _tensor(d['g_rep'])).sum().backward()
  assert _forward_ratio({k: _host(v) for k, v in out.items()}, ref) <= 1.0
  assert cases.grad_ratio(_host(post.grad), ref['grad_post'], d['g_rep'], kind == 'bf16') <= 1.0
  assert cases.grad_ratio(_host(prior.grad), ref['grad_prior'], d['g_dyn'], kind == 'bf16') <= 1.0
  # the room around them is as it was
  inside = torch.zeros_like(room, dtype=torch.bool)
  inside[7:7 + n] = True
  inside[n + 21:2 * n + 21] = True
  assert torch.isnan(room[~inside]).all() and not torch.isnan(room[inside]).any()


@PATHS
def test_strided_and_offset_inputs(fused):
  d = _data(32, 24, 36, 1.0)
  ref = _ref(d, 0.01, 1.0)
  wide = torch.zeros(2, 36, 32, 40, device='cuda')
  wide[0, ..., 3:27] = _tensor(d['post'])
  wide[1, ..., 3:27] = _tensor(d['prior'])
  post = wide[0, ..., 3:27].view(4, 9, 32, 24).detach().requires_grad_()        # classes 40 floats apart, offset 3
  prior = wide[1, ..., 3:27].view(4, 9, 32, 24).detach().requires_grad_()
  assert not post.is_contiguous()
  out = rssm_kl(post, prior, fused=fused)
  (out['dyn'] * _tensor(d['g_dyn']).view(4, 9) + out['rep'] * _tensor(d['g_rep']).view(4, 9)).sum().backward()
  assert _forward_ratio({k: _host(v).reshape(-1) for k, v in out.items()}, ref) <= 1.0
  assert post.grad.shape == (4, 9, 32, 24)
  assert cases.grad_ratio(_host(post.grad).reshape(36, 32, 24), ref['grad_post'], d['g_rep']) <= 1.0
  assert cases.grad_ratio(_host(prior.grad).reshape(36, 32, 24), ref['grad_prior'], d['g_dyn']) <= 1.0
  # rows transposed: (T, B) seen as (B, T)
  turned = _tensor(d['post']).view(9, 4, 32, 24).transpose(0, 1)
  turned_prior = _tensor(d['prior']).view(9, 4, 32, 24).transpose(0, 1)
  out = rssm_kl(turned, turned_prior, fused=fused)
  assert cases.forward_ratio(_host(out['dyn']).T.reshape(-1), ref['dyn']) <= 1.0


def _kernel_constants():
  text = (pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc' / 'onehot_kl.hip').read_text()
  return {name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1)) for name in ('kWave', 'kWaves', 'kMaxBlocks')}


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_rows_beyond_one_sweep_of_the_capped_grid(kind):
  """Both kernels give a wave to a row: their capped grid of kMaxBlocks workgroups
  of kWaves waves (csrc/onehot_kl.hip, read here) covers 8192 rows in one sweep, so
  row 8192 is the first one of the stride loop's second iteration."""
  k = _kernel_constants()
  sweep = k['kMaxBlocks'] * k['kWaves']
  assert sweep == 8192 and k['kWave'] == 64, k
  rows = sweep + 1
  d = _data(1, 4, rows, 1.0, kind)
  ref = _ref(d, 0.01, 0.0)
  out, grad_post, grad_prior = _run(d, 0.01, 0.0, True, kind)
  seam = slice(sweep - 4, rows)
  assert _forward_ratio(out, ref) <= 1.0
  assert _forward_ratio({key: v[seam] for key, v in out.items()},
                        {key: v[seam] for key, v in ref.items() if key not in ('grad_post', 'grad_prior')}) <= 1.0
  assert cases.grad_ratio(grad_post, ref['grad_post'], d['g_rep'], kind == 'bf16') <= 1.0
  assert cases.grad_ratio(grad_prior, ref['grad_prior'], d['g_dyn'], kind == 'bf16') <= 1.0
  assert out['dyn'][-1] != 0 and np.abs(grad_post[-1]).max() > 0 and np.abs(grad_prior[-1]).max() > 0


def _poisoned(d, side, value, row=2, group=1):
  post, prior = d['post'].copy(), d['prior'].copy()
  target = post if side == 'post' else prior
  if value == 'group':
    target[row, group, :] = -np.inf
  else:
    target[row, group, 3] = value
  return post, prior


def _both_runs(d, post, prior, unimix, fused):
  """(clean, poisoned) runs of the same call, each (outputs, grad_post, grad_prior) as tensors."""
  runs = []
  for p, q in ((d['post'], d['prior']), (post, prior)):
    p, q = _tensor(p).requires_grad_(), _tensor(q).requires_grad_()
    out = rssm_kl(p, q, unimix=unimix, free_nats=1.0, fused=fused)
    (out['dyn'] * _tensor(d['g_dyn']) + out['rep'] * _tensor(d['g_rep'])).sum().backward()
    runs.append(({k: v.detach() for k, v in out.items()}, p.grad, q.grad))
  return runs


def _other_rows_unchanged(clean, dirty, row):
  keep = torch.arange(clean[1].shape[0], device='cuda') != row
  for key in OUTPUTS:
    assert torch.equal(clean[0][key][keep], dirty[0][key][keep]), key
  assert torch.equal(clean[1][keep], dirty[1][keep]) and torch.equal(clean[2][keep], dirty[2][keep])
  assert torch.isfinite(dirty[1][keep]).all() and torch.isfinite(dirty[2][keep]).all()


@PATHS
@pytest.mark.parametrize('unimix', cases.UNIMIX)
@pytest.mark.parametrize('side', ['post', 'prior'])
@pytest.mark.parametrize('value', [np.nan, np.inf, 'group'], ids=['nan', 'pinf', 'group_of_ninf'])
def test_nan_or_pinf_logit_poisons_its_row_only(value, side, unimix, fused):
  """A NaN or +inf logit, or a group of -inf: that row's dyn, rep and the
  entropy of the poisoned side are NaN (the other side's entropy is what it was),
  its gradients NaN in the poisoned group on both sides (on the kernels: over
  the whole row), and no other row changes by a bit."""
  d = _data(3, 5, 5, 1.0)
  clean, dirty = _both_runs(d, *_poisoned(d, side, value), unimix, fused)
  bad, good = ('rep_ent', 'dyn_ent') if side == 'post' else ('dyn_ent', 'rep_ent')
  for key in ('dyn', 'rep', bad):
    assert torch.isnan(dirty[0][key][2]), key
  assert torch.equal(dirty[0][good], clean[0][good])
  assert torch.isnan(dirty[1][2, 1]).all() and torch.isnan(dirty[2][2, 1]).all()
  if fused:
    assert torch.isnan(dirty[1][2]).all() and torch.isnan(dirty[2][2]).all()
  _other_rows_unchanged(clean, dirty, 2)


@PATHS
@pytest.mark.parametrize('side', ['post', 'prior'])
def test_ninf_logit_with_unimix_is_a_class_of_probability_u_over_classes(side, fused):
  d = _data(3, 5, 5, 1.0)
  post, prior = _poisoned(d, side, -np.inf)
  clean, dirty = _both_runs(d, post, prior, 0.01, fused)
  ref = cases.reference64(post, prior, 0.01, 1.0, d['g_dyn'], d['g_rep'])
  assert np.isfinite(ref['kl']).all()
  assert _forward_ratio({k: _host(v) for k, v in dirty[0].items()}, ref) <= 1.0
  assert cases.grad_ratio(_host(dirty[1]), ref['grad_post'], d['g_rep']) <= 1.0
  assert cases.grad_ratio(_host(dirty[2]), ref['grad_prior'], d['g_dyn']) <= 1.0
  was = cases.reference64(d['post'], d['prior'], 0.01, 0.0)['kl'][2]
  assert abs(ref['kl'][2] - was) > 1e-3 and torch.isfinite(dirty[1]).all() and torch.isfinite(dirty[2]).all()
  _other_rows_unchanged(clean, dirty, 2)


@PATHS
def test_ninf_logit_without_unimix(fused):
  """unimix = 0.  In post it is 0 * -inf in the definition: kl, dyn, rep and
  rep_ent of the row are NaN on both paths, dyn_ent stays finite, post's gradient
  is NaN in that group (on the kernels both gradients over the whole row).  In
  prior alone: kl, dyn and rep are +inf and dyn_ent is NaN."""
  d = _data(3, 5, 5, 1.0)
  clean, dirty = _both_runs(d, *_poisoned(d, 'post', -np.inf), 0.0, fused)
  for key in ('dyn', 'rep', 'rep_ent'):
    assert torch.isnan(dirty[0][key][2]), key
  assert torch.isfinite(dirty[0]['dyn_ent'][2]) and torch.equal(dirty[0]['dyn_ent'], clean[0]['dyn_ent'])
  assert torch.isnan(dirty[1][2, 1]).all()
  if fused:
    assert torch.isnan(dirty[1][2]).all() and torch.isnan(dirty[2][2]).all()
  _other_rows_unchanged(clean, dirty, 2)
  clean, dirty = _both_runs(d, *_poisoned(d, 'prior', -np.inf), 0.0, fused)
  assert torch.isposinf(dirty[0]['dyn'][2]) and torch.isposinf(dirty[0]['rep'][2])
  assert torch.isnan(dirty[0]['dyn_ent'][2]) and torch.equal(dirty[0]['rep_ent'], clean[0]['rep_ent'])
  keep = torch.arange(5, device='cuda') != 2
  for key in OUTPUTS:
    assert torch.equal(clean[0][key][keep], dirty[0][key][keep]), key
  assert torch.equal(clean[1][keep], dirty[1][keep]) and torch.equal(clean[2][keep], dirty[2][keep])


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_same_bits_run_to_run(kind):
  d = _data(32, 24, 37, 5.0, kind)
  first = _run(d, 0.01, 1.0, True, kind)
  again = _run(d, 0.01, 1.0, True, kind)
  for key in OUTPUTS:
    assert np.array_equal(first[0][key], again[0][key]), key
  assert np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])


def test_launch_counts():
  d = _data(32, 24, 37, 1.0)
  torch.cuda.synchronize()
  before = onehot_kl_launches()
  post, prior = _tensor(d['post']).requires_grad_(), _tensor(d['prior']).requires_grad_()
  out = rssm_kl(post, prior)                                  # fused=None takes the kernels where they fit
  assert onehot_kl_launches() == before + 1
  (out['dyn'] + out['rep']).sum().backward()
  assert onehot_kl_launches() == before + 2                   # one forward, one backward
  assert post.grad is not None and prior.grad is not None
  post.grad = prior.grad = None
  out = rssm_kl(post, prior, fused=False)
  (out['dyn'] + out['rep']).sum().backward()
  assert onehot_kl_launches() == before + 2                   # the composed path launches none of the kernels
  wide = torch.zeros(3, 2, 257, device='cuda', requires_grad=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes.*at most 256'):
    rssm_kl(wide, wide.detach(), fused=True)
  with pytest.raises(ValueError, match=r'fused=True.*257 classes'):
    OneHot(wide, fused=True)
  out = rssm_kl(wide, wide.detach())
  out['rep'].sum().backward()
  assert OneHot(wide).fused is False
  # no rows: composed, nothing launched
  for fused in (True, None, False):
    empty = torch.zeros(0, 4, 8, device='cuda', requires_grad=True)
    out = rssm_kl(empty, torch.zeros(0, 4, 8, device='cuda'), fused=fused)
    assert all(out[key].shape == (0,) and out[key].dtype == torch.float32 for key in OUTPUTS)
    out['rep'].sum().backward()
    assert empty.grad.shape == (0, 4, 8)
    assert OneHot(torch.zeros(2, 0, 4, 8, device='cuda'), fused=fused).entropy().shape == (2, 0)
  assert onehot_kl_launches() == before + 2
  # OneHot: kl forward + backward two launches, entropy one
  a = OneHot(post, 0.01, fused=True)
  a.kl(OneHot(prior, 0.01, fused=True)).sum().backward()
  assert onehot_kl_launches() == before + 4
  a.entropy()
  assert onehot_kl_launches() == before + 5


def test_refusals():
  x = torch.zeros(3, 4, 8, device='cuda')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    rssm_kl(x.cpu(), x.cpu())
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    rssm_kl(x, x.cpu())
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    OneHot(x.cpu())
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    rssm_kl(x.half(), x.half())
  with pytest.raises(TypeError, match='float32 or bfloat16'):
    OneHot(x.double())
  with pytest.raises(TypeError, match='torch.float32.*torch.bfloat16'):
    rssm_kl(x, x.bfloat16())
  with pytest.raises(ValueError, match='shapes'):
    rssm_kl(x, x[:2])
  with pytest.raises(ValueError, match='shapes'):
    OneHot(x).kl(OneHot(x.view(3, 8, 4)))
  with pytest.raises(ValueError, match='unimix 0.01 against 0.0'):
    OneHot(x, 0.01).kl(OneHot(x))
  with pytest.raises(TypeError, match='must be a OneHot'):
    OneHot(x).kl(x)
  with pytest.raises(ValueError, match='stoch, classes'):
    OneHot(x[0, 0])
  with pytest.raises(ValueError, match='unimix'):
    OneHot(x, 1.0)
  with pytest.raises(ValueError, match='free_nats'):
    rssm_kl(x, x, free_nats=-1.0)
