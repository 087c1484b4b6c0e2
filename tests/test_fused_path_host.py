"""The fused-or-composed decision of every head and net facade, and the refusals of
the actor-loss frame, pinned word for word: what `fused` = None / True / False
returns where the kernels fit and where they do not, and the full text of every
refusal.  The expected texts are written out here, not computed by the package.
CPU only."""
import pytest
import torch

TAIL = ' (fused=None or False composes it)'
WAVE = ' in one wave\'s registers' + TAIL
FULL = 1 << 31                                  # one more than the kernels index


def _decisions():
  from embodied_amd import nets
  from embodied_amd import outs
  twohot = lambda n, rows: lambda fused: outs._path(fused, n, rows)
  kl = lambda *shape: lambda fused: outs._kl_path(fused, *shape)
  sample = lambda who, *shape: lambda fused: outs._sample_path(who, fused, *shape)
  policy = lambda *shape: lambda fused: outs._policy_path(fused, *shape)
  recon = lambda who, *shape: lambda fused: outs._recon_path(who, fused, *shape)
  normal = lambda *shape: lambda fused: outs._normal_path(fused, *shape)
  norm = lambda *shape: lambda fused: nets._norm_path(fused, *shape)
  gate = lambda *shape: lambda fused: nets._gate_path(fused, *shape)
  # (name, call, the refusal of fused=True or None where the kernels fit)
  return [
      ('twohot fits', twohot(255, 16384), None),
      ('twohot widest', twohot(1024, (FULL - 1) // 1024), None),
      ('twohot registers', twohot(1025, 5),
       'TwoHot(fused=True): 1025 bins, the kernels keep a row of at most 1024' + WAVE),
      ('twohot index', twohot(1024, FULL // 1024),
       'TwoHot(fused=True): 2097152 x 1024 logits, the kernels index at most 2^31 - 1' + TAIL),
      ('twohot both', twohot(2048, FULL // 1024),
       'TwoHot(fused=True): 2048 bins, the kernels keep a row of at most 1024' + WAVE),

      ('kl fits', kl(1024, 32, 32), None),
      ('kl widest', kl(5, 1, 256), None),
      ('kl registers', kl(5, 2, 257),
       'OneHot(fused=True): 257 classes, the kernels keep a group of at most 256' + WAVE),
      ('kl no classes', kl(5, 2, 0), 'OneHot(fused=True): 0 classes, the kernels keep a group of at most 256' + WAVE),
      ('kl index', kl(FULL // 2048, 32, 64),
       'OneHot(fused=True): 1048576 x 32 x 64 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('kl no groups', kl(5, 0, 8), 'OneHot(fused=True): 5 x 0 x 8 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('kl both', kl(5, 0, 257), 'OneHot(fused=True): 257 classes, the kernels keep a group of at most 256' + WAVE),

      ('sample fits', sample('OneHot', 16, 32, 32), None),
      ('sample fits, actor', sample('Categorical', 1024, 1, 18), None),
      ('sample registers', sample('OneHot', 5, 2, 257),
       'OneHot(fused=True): 257 classes, the kernels keep a group of at most 256' + WAVE),
      ('sample registers, actor', sample('Categorical', 5, 2, 0),
       'Categorical(fused=True): 0 classes, the kernels keep a group of at most 256' + WAVE),
      ('sample index', sample('Categorical', FULL // 2048, 32, 64),
       'Categorical(fused=True): 1048576 x 32 x 64 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('sample no groups', sample('OneHot', 5, 0, 8),
       'OneHot(fused=True): 5 x 0 x 8 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('sample both', sample('OneHot', FULL, 0, 300),
       'OneHot(fused=True): 300 classes, the kernels keep a group of at most 256' + WAVE),

      ('policy fits', policy(16384 * 16, 1, 6), None),
      ('policy widest', policy(5, 4, 256), None),
      ('policy registers', policy(5, 2, 257),
       'Categorical(fused=True): 257 classes, the kernels keep a group of at most 256' + WAVE),
      ('policy index', policy(FULL // 2048, 32, 64),
       'Categorical(fused=True): 1048576 x 32 x 64 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('policy no groups', policy(5, 0, 8),
       'Categorical(fused=True): 5 x 0 x 8 logits, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('policy both', policy(5, 0, 0),
       'Categorical(fused=True): 0 classes, the kernels keep a group of at most 256' + WAVE),

      ('recon fits', recon('ImageMSE', 1024, 64 * 64 * 3), None),
      ('recon largest', recon('MSE', 1, FULL - 1), None),
      ('recon index', recon('ImageMSE', FULL // 4096, 4096),
       'ImageMSE(fused=True): 524288 x 4096 elements, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('recon index, symlog', recon('MSE', FULL, 1),
       'MSE(fused=True): 2147483648 x 1 elements, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('recon no units', recon('Binary', 7, 0),
       'Binary(fused=True): 7 x 0 elements, the kernels index 1 .. 2^31 - 1' + TAIL),

      ('normal fits', normal(16384 * 16, 6), None),
      ('normal widest', normal(5, 256), None),
      ('normal registers', normal(5, 257),
       'Normal(fused=True): 257 action dimensions, the kernels keep a row of at most 256' + WAVE),
      ('normal no actions', normal(5, 0),
       'Normal(fused=True): 0 action dimensions, the kernels keep a row of at most 256' + WAVE),
      ('normal index', normal(FULL // 64, 64),
       'Normal(fused=True): 33554432 x 64 elements, the kernels index 1 .. 2^31 - 1' + TAIL),
      ('normal both', normal(FULL, 257),
       'Normal(fused=True): 257 action dimensions, the kernels keep a row of at most 256' + WAVE),

      ('norm fits', norm(16, 1024), None),
      ('norm widest', norm(5, 16384), None),
      ('norm registers', norm(5, 16385),
       'norm_act(fused=True): 16385 units, the kernels keep a row of at most 16384 in one workgroup\'s registers'
       + TAIL),
      ('norm no units', norm(5, 0),
       'norm_act(fused=True): 0 units, the kernels keep a row of at most 16384 in one workgroup\'s registers' + TAIL),
      ('norm index', norm(FULL // 1024, 1024),
       'norm_act(fused=True): 2097152 x 1024 elements, the kernels index at most 2^31 - 1' + TAIL),
      ('norm both', norm(FULL, 16385),
       'norm_act(fused=True): 16385 units, the kernels keep a row of at most 16384 in one workgroup\'s registers'
       + TAIL),

      ('gate fits', gate(16, 8192, 8), None),
      ('gate largest', gate((FULL - 1) // 3, 1, 1), None),
      ('gate index', gate(FULL // 3072 + 1, 1024, 8),
       'gru_gate(fused=True): 699051 x 3072 elements of x, the kernels index at most 2^31 - 1' + TAIL),
  ]


def test_every_case_is_what_it_says():
  """The table above covers all eight families, and the sizes in it are on the side
  of 2^31 - 1 that their names say."""
  names = [name for name, _, _ in _decisions()]
  assert len(set(names)) == len(names)
  for family in ('twohot', 'kl', 'sample', 'policy', 'recon', 'normal', 'norm', 'gate'):
    kinds = {name.split(' ', 1)[1].split(',')[0] for name in names if name.split(' ')[0] == family}
    assert {'fits', 'index'} <= kinds, family
    assert ('registers' in kinds) == (family not in ('recon', 'gate')), family
  assert 2097152 * 1024 == 1048576 * 32 * 64 == 524288 * 4096 == 33554432 * 64 == FULL
  assert 699050 * 3072 < FULL <= 699051 * 3072 and (FULL - 1) // 1024 * 1024 < FULL


@pytest.mark.parametrize('case', range(len(_decisions())), ids=[name for name, _, _ in _decisions()])
def test_decision(case):
  _, call, refusal = _decisions()[case]
  fits = refusal is None
  assert call(None) is fits
  assert call(False) is False
  if fits:
    assert call(True) is True
  else:
    with pytest.raises(ValueError) as raised:
      call(True)
    assert str(raised.value) == refusal


def test_any_truth_value_forces_a_path():
  """`fused` is taken by its truth value unless it is None: 1 and 0 are True and False."""
  from embodied_amd import nets
  from embodied_amd import outs
  assert outs._policy_path(1, 5, 1, 8) is True and outs._policy_path(0, 5, 1, 8) is False
  assert nets._gate_path(1, 5, 8, 1) is True and nets._gate_path(0, 5, 8, 1) is False
  with pytest.raises(ValueError) as raised:
    outs._path(1, 1025, 5)
  assert str(raised.value) == 'TwoHot(fused=True): 1025 bins, the kernels keep a row of at most 1024' + WAVE


NO_FALLBACK = 'embodied_amd.outs runs as HIP kernels: pass CUDA tensors (no CPU fallback)'


def test_host_tensors_are_refused_in_these_words():
  import numpy as np
  from embodied_amd import nets
  from embodied_amd import outs
  x = torch.zeros(3, 4, 8)
  refused = [
      lambda: outs.TwoHot(x, outs.symexp_twohot_bins(8)),
      lambda: outs.TwoHot(np.zeros((3, 8), np.float32), np.zeros(8, np.float32)),
      lambda: outs.OneHot(x), lambda: outs.rssm_kl(x, x), lambda: outs.Categorical(x),
      lambda: outs.policy_loss(x, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 4)),
      lambda: outs.MSE(x), lambda: outs.ImageMSE(x), lambda: outs.Binary(x), lambda: outs.Normal(x, x),
      lambda: outs.Normal(x.to('meta'), x),
      lambda: outs.normal_policy_loss(x, x, x, torch.zeros(3, 3), torch.zeros(3, 4)),
  ]
  for call in refused:
    with pytest.raises(RuntimeError) as raised:
      call()
    assert str(raised.value) == NO_FALLBACK
  for draw in (outs.philox_uniform, outs.philox_normal):
    with pytest.raises(RuntimeError) as raised:
      draw(1, device='cpu')
    assert str(raised.value) == 'embodied_amd.outs runs as HIP kernels: pass a CUDA device (no CPU fallback)'
  with pytest.raises(RuntimeError) as raised:
    nets.norm_act(x)
  assert str(raised.value) == 'embodied_amd.nets.norm_act runs as HIP kernels: pass CUDA tensors (no CPU fallback)'
  with pytest.raises(RuntimeError) as raised:
    nets.gru_gate(torch.zeros(3, 24), x[0, :3], 2)
  assert str(raised.value) == 'embodied_amd.nets.gru_gate runs as HIP kernels: pass CUDA tensors (no CPU fallback)'


def test_philox_refusals():
  from embodied_amd import outs
  texts = {
      outs.philox_uniform: ('philox_uniform', 'groups'),
      outs.philox_normal: ('philox_normal', 'elements'),
  }
  for draw, (who, noun) in texts.items():
    refused = [
        (TypeError, dict(seed=None), f'{who}: seed must be an integer, got NoneType'),
        (TypeError, dict(seed=True), f'{who}: seed must be an integer, got bool'),
        (ValueError, dict(seed=-1), f'{who}: seed = -1, needs 0 <= seed < 2^64'),
        (ValueError, dict(seed=1, offset=1 << 64),
         f'{who}: offset = 18446744073709551616, needs 0 <= offset < 2^64'),
        (TypeError, dict(seed=1, first=0.5), f'{who}: first must be an integer, got float'),
        (ValueError, dict(seed=1, count=-1),
         f'{who}: count = -1 from first = 0, needs 0 <= count and {noun} below 2^64'),
        (ValueError, dict(seed=1, first=(1 << 64) - 1, count=2),
         f'{who}: count = 2 from first = 18446744073709551615, needs 0 <= count and {noun} below 2^64'),
    ]
    for error, kw, text in refused:
      with pytest.raises(error) as raised:
        draw(device='cuda', **kw)
      assert str(raised.value) == text


@pytest.fixture
def on_host(monkeypatch):
  """The two loss facades on host tensors: every call below is refused before a launch."""
  from embodied_amd import outs
  monkeypatch.setattr(outs, '_check_device', lambda tensor: None)
  return outs


def _refused(call, text):
  with pytest.raises(ValueError) as raised:
    call()
  assert str(raised.value) == text


def test_policy_loss_refusals(on_host):
  loss = on_host.policy_loss
  x = torch.zeros(3, 4, 8)
  act, adv, weight = torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 4)
  for fused in (None, True, False):
    _refused(lambda: loss(x, act, adv, weight, actent=float('nan'), fused=fused),
             'policy_loss: actent = nan, needs a finite value')
    _refused(lambda: loss(x, act, adv, weight, actent=float('-inf'), fused=fused),
             'policy_loss: actent = -inf, needs a finite value')
    _refused(lambda: loss(x[0, 0], act[0, 0], adv[0, 0], weight[0, 0], fused=fused),
             'policy_loss: drop_last needs a time axis, logits of shape (8,)')
    _refused(lambda: loss(x[0], act[0], adv[0], weight[0], dims=1, fused=fused),
             'policy_loss: drop_last needs a time axis, logits of shape (4, 8)')
    _refused(lambda: loss(x, act, weight, weight, fused=fused), 'policy_loss: adv of shape (3, 4), needs (3, 3)')
    _refused(lambda: loss(x, act, adv, weight, drop_last=False, fused=fused),
             'policy_loss: adv of shape (3, 3), needs (3, 4)')
    _refused(lambda: loss(x, act, adv, weight[:, :2], fused=fused),
             'policy_loss: weight of shape (3, 2), needs (3, 3) or (3, 4)')
    _refused(lambda: loss(x, act, weight, adv, drop_last=False, fused=fused),
             'policy_loss: weight of shape (3, 3), needs (3, 4) or (3, 4)')
    _refused(lambda: loss(x, act, [0.0, 0.0, 0.0], weight, fused=fused), 'policy_loss: adv of shape (3,), needs (3, 3)')
  # the order of the refusals: actent, the time axis, the actions, adv, weight, and the path last
  _refused(lambda: loss(x[0, 0], act, weight, adv, actent=float('inf')),
           'policy_loss: actent = inf, needs a finite value')
  _refused(lambda: loss(x[0, 0], act, weight, adv), 'policy_loss: drop_last needs a time axis, logits of shape (8,)')
  _refused(lambda: loss(x, act[:, :3], weight, adv), 'policy_loss: actions of shape (3, 3), the logits need (3, 4)')
  _refused(lambda: loss(x, act, weight, adv), 'policy_loss: adv of shape (3, 4), needs (3, 3)')
  wide = torch.zeros(3, 4, 257)
  _refused(lambda: loss(wide, act, adv, weight[:, :2], fused=True),
           'policy_loss: weight of shape (3, 2), needs (3, 3) or (3, 4)')
  _refused(lambda: loss(wide, act, adv, weight, fused=True),
           'Categorical(fused=True): 257 classes, the kernels keep a group of at most 256' + WAVE)


def test_normal_policy_loss_refusals(on_host):
  loss = on_host.normal_policy_loss
  x = torch.zeros(3, 4, 6)
  adv, weight = torch.zeros(3, 3), torch.zeros(3, 4)
  for fused in (None, True, False):
    _refused(lambda: loss(x, x, x, adv, weight, actent=float('nan'), fused=fused),
             'normal_policy_loss: actent = nan, needs a finite value')
    _refused(lambda: loss(x, x, x, adv, weight, actent=float('inf'), fused=fused),
             'normal_policy_loss: actent = inf, needs a finite value')
    _refused(lambda: loss(x[0, 0, 0], x[0, 0, 0], x[0, 0, 0], adv[0, 0], weight[0, 0], dims=0, fused=fused),
             'normal_policy_loss: drop_last needs a time axis, inputs of shape ()')
    _refused(lambda: loss(x[0, 0], x[0, 0], x[0, 0], adv[0, 0], weight[0, 0], fused=fused),
             'normal_policy_loss: drop_last needs a time axis, inputs of shape (6,)')
    _refused(lambda: loss(x, x, x, weight, weight, fused=fused),
             'normal_policy_loss: adv of shape (3, 4), needs (3, 3)')
    _refused(lambda: loss(x, x, x, adv, weight, drop_last=False, fused=fused),
             'normal_policy_loss: adv of shape (3, 3), needs (3, 4)')
    _refused(lambda: loss(x, x, x, adv, weight[:, :2], fused=fused),
             'normal_policy_loss: weight of shape (3, 2), needs (3, 3) or (3, 4)')
    _refused(lambda: loss(x, x, x, weight, adv, drop_last=False, fused=fused),
             'normal_policy_loss: weight of shape (3, 3), needs (3, 4) or (3, 4)')
  # the order of the refusals: actent, the time axis, the actions, adv, weight, and the path last
  _refused(lambda: loss(x[0, 0], x[0, 0], x, weight, adv, actent=float('nan')),
           'normal_policy_loss: actent = nan, needs a finite value')
  _refused(lambda: loss(x[0, 0], x[0, 0], x, weight, adv),
           'normal_policy_loss: drop_last needs a time axis, inputs of shape (6,)')
  _refused(lambda: loss(x, x, x[:, :3], weight, adv),
           'normal_policy_loss: actions of shape (3, 3, 6), the inputs need (3, 4, 6)')
  wide = torch.zeros(3, 4, 257)
  _refused(lambda: loss(wide, wide, wide, adv, weight[:, :2], fused=True),
           'normal_policy_loss: weight of shape (3, 2), needs (3, 3) or (3, 4)')
  _refused(lambda: loss(wide, wide, wide, adv, weight, fused=True),
           'Normal(fused=True): 257 action dimensions, the kernels keep a row of at most 256' + WAVE)
