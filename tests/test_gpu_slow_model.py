"""`embodied_amd.optim.SlowModel` on the device: the stand-alone launch
(csrc/optim.hip: slow_update_kernel), the update folded into the update launch of
`LaProp` and `Adam`, and the composed path.  Need a GPU.

The expected value everywhere is numpy's float32 `mix * src + omm * dst`: two
rounded products and one rounded sum.  The comparison is bit equality; there is
no tolerance.  Where numpy's answer is a NaN the device's must be a NaN too, in
that element: which NaN is the one thing the two leave open (0 * inf is -NaN on
the host and +NaN on the device)."""
import numpy as np
import pytest
import torch

from embodied_amd.optim import Adam, LaProp, SlowModel, optimizer_launches, slow_mix      # fails without the feature

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 7)
DST_OFF = (0, 1, 2, 3, 0, 1, 2, 3, 0)               # element offsets of the views into their flat buffers
SRC_OFF = (0, 1, 3, 2, 1, 1, 0, 3, 2)               # co-aligned with dst at 0, 1, 5, 7; not at 2, 3, 4, 6, 8
GUARD = 8                                           # elements in front of and behind every view; a multiple of 4
DENORMAL = np.float32(1e-40)


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _same(got, want):
  """Bit equality, a NaN for a NaN."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
  nan = np.isnan(want)
  return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def _expected(rate, src, dst):
  mix, omm = slow_mix(rate)
  with np.errstate(all='ignore'):
    out = mix * src + omm * dst
  assert out.dtype == np.float32
  return out


class Views:
  """Tensors cut as views from flat buffers with guard bands, beside their numpy images."""

  def __init__(self, arrays, offsets):
    self.flat, self.image, self.views, self.where = [], [], [], []
    for values, offset in zip(arrays, offsets):
      values = np.asarray(values, np.float32)
      image = np.full(GUARD + offset + values.size + GUARD, 77.25, np.float32)
      lo = GUARD + offset
      image[lo:lo + values.size] = values.ravel()
      flat = torch.from_numpy(image.copy()).cuda()
      self.flat.append(flat)
      self.image.append(image)
      self.where.append((lo, lo + values.size))
      self.views.append(flat[lo:lo + values.size].view(values.shape))
      assert not values.size or self.views[-1].data_ptr() % 16 == 4 * (offset % 4)

  def set(self, index, values):
    lo, hi = self.where[index]
    self.image[index][lo:hi] = np.asarray(values, np.float32).ravel()
    self.views[index].copy_(torch.from_numpy(np.asarray(values, np.float32)).cuda().view(self.views[index].shape))

  def values(self, index):
    lo, hi = self.where[index]
    return self.image[index][lo:hi]

  def check(self, wants=None):
    """The device holds `wants` inside the views (the images where not given) and the images around them."""
    torch.cuda.synchronize()
    for index, (flat, image, (lo, hi)) in enumerate(zip(self.flat, self.image, self.where)):
      got = flat.cpu().numpy()
      if wants is not None:
        image[lo:hi] = wants[index]
      assert _same(got[:lo], image[:lo]) and _same(got[hi:], image[hi:]), ('guard band', index)
      assert _same(got[lo:hi], image[lo:hi]), ('values', index, hi - lo)


def _special_sets(rng):
  """src and dst values for COUNTS; from 8 elements on the specials sit at known places."""
  src = [rng.standard_normal(n).astype(np.float32) for n in COUNTS]
  dst = [rng.standard_normal(n).astype(np.float32) for n in COUNTS]
  for s, d in zip(src, dst):
    if s.size >= 8:
      s[:6] = [0.0, -0.0, DENORMAL, np.inf, -np.inf, np.nan]
      s[-1] = -DENORMAL
      d[7] = np.nan
      d[0] = -0.0
  return src, dst


@pytest.mark.parametrize('rate', [0.02, 1.0])
def test_stand_alone_update_over_sizes_and_alignments(rate):
  rng = np.random.default_rng(11)
  src_values, dst_values = _special_sets(rng)
  src = Views(src_values, SRC_OFF)
  dst = Views([np.zeros(n, np.float32) for n in COUNTS], DST_OFF)
  slow = SlowModel(dst.views, src.views, rate=rate, fused=True)
  assert slow.fused is True and slow.count == 0 and slow.table_uploads == 0
  dst.check([src.values(i) for i in range(len(COUNTS))])              # construction copied source into model
  src.check()
  for i, values in enumerate(dst_values):
    dst.set(i, values)
  for step in range(2):
    before = optimizer_launches()
    slow.update()
    assert optimizer_launches() == before + 1 and slow.count == step + 1 and slow.table_uploads == 1
    wants = [_expected(rate, src.values(i), dst.values(i)) for i in range(len(COUNTS))]
    dst.check(wants)
    src.check()
    if step == 0:
      big = wants[7].copy()
  # after the first update (the second, at rate 1, has 0 * inf in these elements) the specials are where they were
  # put, and nowhere else; at rate 1 it is 1 * src + 0 * dst as numpy gives it
  assert np.isposinf(big[3]) and np.isneginf(big[4]) and np.isnan(big[[5, 7]]).all()
  assert np.isfinite(np.delete(big, [3, 4, 5, 7])).all() and big[2] != 0 and big[-1] != 0
  if rate == 1.0:
    assert big[2] == DENORMAL and big[-1] == -DENORMAL


def test_more_tensors_than_workgroups():
  """2100 tensors of 1 .. 5 elements, one chunk each: past the 2048 workgroups of the grid."""
  rng = np.random.default_rng(12)
  sizes = [1 + i % 5 for i in range(2100)]
  starts = np.cumsum([0] + [n + 1 for n in sizes])                     # one element between neighbours stays as it is
  image_src = rng.standard_normal(starts[-1]).astype(np.float32)
  image_dst = rng.standard_normal(starts[-1]).astype(np.float32)
  flat_src, flat_dst = torch.from_numpy(image_src).cuda(), torch.from_numpy(image_dst.copy()).cuda()
  src = [flat_src[a:a + n] for a, n in zip(starts, sizes)]
  dst = [flat_dst[a:a + n] for a, n in zip(starts, sizes)]
  slow = SlowModel(dst, src, rate=0.02)
  assert slow.fused is True
  want = image_dst.copy()
  for a, n in zip(starts, sizes):
    want[a:a + n] = image_src[a:a + n]
  assert _same(flat_dst.cpu().numpy(), want)                            # _initonce
  flat_dst.copy_(torch.from_numpy(image_dst).cuda())
  before = optimizer_launches()
  slow.update()
  assert optimizer_launches() == before + 1 and slow._plan['n_chunks'] == 2100
  want = image_dst.copy()
  for a, n in zip(starts, sizes):
    want[a:a + n] = _expected(0.02, image_src[a:a + n], image_dst[a:a + n])
  assert _same(flat_dst.cpu().numpy(), want) and _same(flat_src.cpu().numpy(), image_src)


def test_every_third_update_and_a_moved_source():
  rng = np.random.default_rng(13)
  src = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() for n in (5, 8193)]
  dst = [torch.zeros(n, device='cuda') for n in (5, 8193)]
  slow = SlowModel(dst, src, rate=0.02, every=3)
  src[1][17] = float('nan')
  src[1][18] = float('inf')
  image = [d.cpu().numpy() for d in dst]
  start = optimizer_launches()
  for step in range(7):
    before = optimizer_launches()
    held = [d.cpu().numpy().view(np.int32) for d in dst]
    slow.update()
    assert slow.count == step + 1
    if step % 3 == 0:
      assert optimizer_launches() == before + 1
      image = [_expected(0.02, s.cpu().numpy(), d) for s, d in zip(src, image)]
    else:                                                               # an off-step touches nothing, NaN in src or not
      assert optimizer_launches() == before
      assert all(np.array_equal(d.cpu().numpy().view(np.int32), h) for d, h in zip(dst, held)), step
    for d, want in zip(dst, image):
      assert np.array_equal(d.cpu().numpy().view(np.int32), want.view(np.int32)) or _same(d.cpu().numpy(), want), step
    if step == 1:
      assert np.isnan(image[1][17]) and np.isinf(image[1][18]) and np.isfinite(image[1][19])
  assert optimizer_launches() == start + 3 and slow.table_uploads == 1
  # the source's storage is replaced: the table follows, once
  state = slow.state_dict()
  assert state == {'count': 7, 'rate': 0.02, 'every': 3}
  moved = torch.from_numpy(rng.standard_normal(8193).astype(np.float32)).cuda()
  src[1].data = moved
  slow.load_state_dict(dict(state, count=9))
  assert slow.count == 9
  slow.update()
  image = [_expected(0.02, s.cpu().numpy(), d) for s, d in zip(src, image)]
  assert slow.table_uploads == 2 and slow.count == 10
  for d, want in zip(dst, image):
    assert _same(d.cpu().numpy(), want)
  slow.update(), slow.update(), slow.update()
  assert slow.table_uploads == 2 and slow.count == 13


def test_composed_path_and_what_the_object_forwards():
  rng = np.random.default_rng(14)
  model, source = torch.nn.Linear(33, 7).cuda(), torch.nn.Linear(33, 7).cuda()
  slow = SlowModel(model, source, rate=0.02)
  assert slow.fused is True
  assert all(torch.equal(d, s) for d, s in zip(model.parameters(), source.parameters()))
  x = torch.ones(2, 33, device='cuda')
  assert torch.equal(slow(x), model(x)) and slow.weight is model.weight and slow.out_features == 7
  for fused in (True, False):
    slow = SlowModel(model, source, rate=0.02, fused=fused)
    with torch.no_grad():
      for p in list(model.parameters()) + list(source.parameters()):
        p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).cuda())
    wants = [_expected(0.02, s.detach().cpu().numpy(), d.detach().cpu().numpy())
             for d, s in zip(model.parameters(), source.parameters())]
    before = optimizer_launches()
    slow.update()
    assert optimizer_launches() == before + (1 if fused else 0)
    for d, want in zip(model.parameters(), wants):
      assert _same(d.detach().cpu().numpy(), want), fused
  # a parameter that is not contiguous: composed under fused=None, refused under fused=True
  strided_src = torch.from_numpy(rng.standard_normal((4, 3)).astype(np.float32)).cuda().t()
  strided_dst = torch.zeros(4, 3, device='cuda').t()
  plain_src, plain_dst = torch.ones(5, device='cuda'), torch.zeros(5, device='cuda')
  with pytest.raises(ValueError, match=r'SlowModel\(fused=True\): parameter .* is not contiguous'):
    SlowModel([plain_dst, strided_dst], [plain_src, strided_src], rate=0.02, fused=True)
  slow = SlowModel([plain_dst, strided_dst], [plain_src, strided_src], rate=0.02)
  assert slow.fused is False and torch.equal(strided_dst, strided_src)
  strided_dst.copy_(torch.from_numpy(rng.standard_normal((3, 4)).astype(np.float32)).cuda())
  want = _expected(0.02, strided_src.cpu().numpy(), strided_dst.cpu().numpy())
  before = optimizer_launches()
  slow.update()
  assert optimizer_launches() == before and _same(np.ascontiguousarray(strided_dst.cpu().numpy()), np.ascontiguousarray(want))


# ---- attached to an optimizer

SHAPES = ((8193,), (17, 5), (3,), (101,), (4, 4), (70, 3))
P_OFF = (0, 0, 2, 1, 0, 3)                          # parameters 2, 3 and 5 are views at offsets off 16 bytes
G_OFF = (0, 0, 2, 1, 0, 0)                          # gradients beside them, but 5's: that tensor goes scalar
TRACKED = (0, 1, 3)
D_OFF = {0: 0, 1: 1, 3: 1}                          # the slow copy of 1 is mis-aligned against p (1 against 0):
                                                    # 16-byte accesses of p, nu, mu and g, four scalar ones of d


def _world(opt_class, bf16, every, seed=21):
  rng = np.random.default_rng(seed)
  params = Views([rng.standard_normal(s).astype(np.float32) * 0.1 for s in SHAPES], P_OFF)
  grads = [[rng.standard_normal(s).astype(np.float32) * 0.01 for s in SHAPES] for _ in range(3)]
  slows = Views([rng.standard_normal(SHAPES[i]).astype(np.float32) for i in TRACKED], [D_OFF[i] for i in TRACKED])
  kw = dict(lr=1e-2, wd=0.01, fused=True)
  opt = opt_class(params.views, warmup=0, **kw)
  slow = SlowModel(slows.views, [params.views[i] for i in TRACKED], rate=0.02, every=every)
  return params, grads, slows, opt, slow


def _set_grads(params, grads, bf16):
  for param, g, offset in zip(params.views, grads, G_OFF):
    flat = torch.zeros(g.size + offset, dtype=torch.bfloat16 if bf16 else torch.float32, device='cuda')
    view = flat[offset:].view(g.shape)
    view.copy_(torch.from_numpy(g).cuda())
    param.grad_dtype = None
    param.grad = view


def _bits(tensor):
  return tensor.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize('every', [1, 2])
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('opt_class', [LaProp, Adam])
def test_attached_equals_step_then_update(opt_class, bf16, every):
  pa, grads, sa, opt_a, slow_a = _world(opt_class, bf16, every)
  pb, _, sb, opt_b, slow_b = _world(opt_class, bf16, every)
  slow_a.attach(opt_a)
  for step in range(3):
    _set_grads(pa, grads[step], bf16)
    _set_grads(pb, grads[step], bf16)
    held = [_bits(v).copy() for v in sa.views]
    before = optimizer_launches()
    opt_a.step()
    assert optimizer_launches() == before + 2, 'the attached step is two launches'
    assert slow_a.count == step + 1
    opt_b.step()
    slow_b.update()
    assert optimizer_launches() == before + 4 + (1 if step % every == 0 else 0)
    for i, (a, b) in enumerate(zip(pa.views, pb.views)):
      assert np.array_equal(_bits(a), _bits(b)), ('p', step, i)
      for name in ('nu', 'mu'):
        assert np.array_equal(_bits(opt_a.state[a][name]), _bits(opt_b.state[b][name])), (name, step, i)
    for i, (a, b) in enumerate(zip(sa.views, sb.views)):
      assert np.array_equal(_bits(a), _bits(b)), ('dst', step, i)
      if step % every:
        assert np.array_equal(_bits(a), held[i]), ('an off-step wrote the slow copy', step, i)
      else:                                                             # and it is the definition over the new p
        want = _expected(0.02, pa.views[TRACKED[i]].cpu().numpy(), held[i].view(np.float32))
        assert _same(a.cpu().numpy(), want), ('dst against numpy', step, i)
    ma, mb = opt_a.metrics(), opt_b.metrics()
    assert sorted(ma) == sorted(mb)
    for key in ma:
      assert float(ma[key]) == float(mb[key]), (key, step)
  # every step's gradients are new tensors, so the optimizers' tables follow them; the attached slow copies ride along
  assert opt_a.table_uploads == opt_b.table_uploads == 3 and slow_b.table_uploads == 1
  # nothing around a parameter or a slow copy was written, in either run
  for views in (pa, pb, sa, sb):
    views.check([v.cpu().numpy().ravel() for v in views.views])


def test_attach_refusals_and_detach():
  params, grads, slows, opt, slow = _world(LaProp, False, 1)
  slow.attach(opt)
  with pytest.raises(RuntimeError, match='SlowModel.update: attached'):
    slow.update()
  with pytest.raises(RuntimeError, match='already attached'):
    slow.attach(opt)
  other = SlowModel([torch.zeros(3, device='cuda')], [params.views[2]], rate=0.02)
  with pytest.raises(RuntimeError, match='one per optimizer'):
    other.attach(opt)
  slow.detach()
  assert opt._slow is None
  before = optimizer_launches()
  slow.update()
  assert optimizer_launches() == before + 1 and slow.count == 1
  with pytest.raises(RuntimeError, match='not attached'):
    slow.detach()
  outside = torch.ones(3, device='cuda')
  stranger = SlowModel([torch.zeros(3, device='cuda'), torch.zeros(3, device='cuda')], [params.views[2], outside], rate=0.02)
  with pytest.raises(ValueError, match=r'source tensor 1 of shape \(3,\) is not a parameter of the optimizer'):
    stranger.attach(opt)
  assert opt._slow is None
  composed = LaProp([torch.zeros(3, device='cuda')], fused=False)
  with pytest.raises(TypeError, match='a fused'):
    slow.attach(composed)
  # a moved slow copy is followed: one more upload, the right values
  other.attach(opt)
  _set_grads(params, grads[0], False)
  opt.step()
  uploads = opt.table_uploads
  fresh = torch.full((3,), 5.0, device='cuda')
  other._dst[0].data = fresh
  _set_grads(params, grads[1], False)
  opt.step()
  assert opt.table_uploads == uploads + 1
  want = _expected(0.02, params.views[2].cpu().numpy(), np.full(3, 5.0, np.float32))
  assert _same(fresh.cpu().numpy(), want) and other.count == 2
