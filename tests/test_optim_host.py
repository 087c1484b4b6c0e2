"""`embodied_amd.optim.LaProp` and `emb_optim_*` as far as they go without a GPU:
the fixture, the restatement the GPU tests rely on, the bars, the declarations
and the binding, the table builder, the path decision, the refusals that happen
before any launch, the warm-up schedule.  CPU only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import optim_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'optim.npz'
NAMES = ('emb_optim_norms', 'emb_optim_update', 'emb_optim_metrics', 'emb_optim_launches')


def test_fixture_is_current():
  """Where the reference tree exists: regenerate in memory and compare."""
  from oracle import refload
  if not (refload.REFERENCE / 'embodied' / 'jax' / 'opt.py').exists():
    pytest.skip('reference tree not present (build container only)')
  import importlib.util
  spec = importlib.util.spec_from_file_location('_gen_optim', ROOT / 'tools' / 'gen_optim_golden.py')
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  fresh = tool.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(fresh)
    for key in f.files:
      assert np.array_equal(f[key], fresh[key]), key


def test_restatement_equals_the_fixture():
  """The fixture belongs to `cases.inputs`; `cases.reference64` agrees with the
  reference's own functions run in float64 to 1e-12 on every case and step."""
  with np.load(GOLDEN) as f:
    assert tuple(f['lines_clip_by_agc']) == (109, 123) and tuple(f['lines_scale_by_rms']) == (126, 143)
    assert tuple(f['lines_scale_by_momentum']) == (146, 164) and tuple(f['lines_rms']) == (120, 124)
    assert f['inputs'].shape == (len(cases.CASES), 32)
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      inp = cases.inputs(case)
      assert np.array_equal(f['inputs'][case], cases.flat_digest(inp)), name
      want = f[f'out64_{name}']
      assert want.dtype == np.float64 and f[f'out_{name}'].dtype == np.float32 and np.isfinite(want).all()
      mine = cases.packed_of(cases.reference64(inp, c.hyper, cases.LISTS[c.list]))
      assert mine.shape == want.shape == f[f'out_{name}'].shape, name
      assert np.allclose(mine, want, rtol=1e-12, atol=1e-12), name
  assert GOLDEN.stat().st_size < 900_000


def test_the_cases_cover_what_they_claim():
  c = cases.C
  sizes = [int(np.prod(s.shape)) for s in cases.LISTS['sizes']]
  assert {1, 3, c - 1, c, c + 1, 2 * c + 5, 0} <= set(sizes)
  assert [len(cases.LISTS[k]) for k in ('one', 'two', 'seventy')] == [1, 2, 70]
  assert -(-int(np.prod(cases.LISTS['wide'][0].shape)) // c) == 70
  assert {s.poff for s in cases.LISTS['views']} >= {1, 2, 3}
  assert any(s.poff % 4 != s.goff % 4 for s in cases.LISTS['views'])              # the scalar path
  assert len(cases.FULL) == 96 and len(set(cases.FULL)) == 96
  for field, values in (('lr', cases.LRS), ('agc', cases.AGCS), ('wd', cases.WDS), ('warmup', cases.WARMUPS),
                        ('nesterov', (False, True)), ('bf16', (False, True))):
    assert {getattr(h, field) for h in cases.COVER} == set(values), field
  for name, specs in cases.LISTS.items():
    if name not in ('one', 'wide'):
      assert len(set(cases.mask_of(specs))) == 2, name                            # a mixed decay mask
  inp = cases.inputs(0)
  g, p = inp['g'][0], inp['p']
  rel = [np.linalg.norm(g[i].ravel()) / (0.3 * max(cases.PMIN, np.linalg.norm(p[i].ravel()))) for i in range(3)]
  assert rel[0] < 1 < rel[1] and np.linalg.norm(p[2].ravel()) < cases.PMIN


def test_float32_definition_against_the_bars():
  """The reference's float32 run (the fixture) and this file's restatement in
  float32 on the CPU over every case, against float64: the worst ratio per list
  and quantity, printed.  A family that misses must be listed in `cases.EXEMPT`;
  nothing else may miss."""
  worst = {}
  with np.load(GOLDEN) as f:
    for case, c in enumerate(cases.CASES):
      name = cases.tag(case)
      inp = cases.inputs(case)
      want = cases.unpack(f[f'out64_{name}'])
      runs = {'reference': cases.unpack(f[f'out_{name}']),
              'restated': cases.unpack(cases.packed_of(cases.restate(inp, c.hyper, cases.LISTS[c.list], torch.float32)))}
      for who, got in runs.items():
        for key in ('p', 'nu', 'mu', 'metrics'):
          bar = cases.ratio_nu if key == 'nu' else cases.ratio
          slot = (c.list, key, who)
          worst[slot] = max(worst.get(slot, 0.0), bar(got[key], want[key]))
  for slot in sorted(worst):
    print(f'float32 {slot[2]}, list {slot[0]}, {slot[1]}: {worst[slot]:.3g} of its bar')
  missed = {slot[:2] for slot, value in worst.items() if value > 1.0}
  assert missed <= set(cases.EXEMPT), {slot: value for slot, value in worst.items() if value > 1.0}


def test_header_declares_and_binding_covers_the_new_symbols():
  import embodied_amd as emb
  from embodied_amd import _lib
  text = (ROOT / 'include' / 'embodied_hip.h').read_text()
  for name in NAMES + ('emb_optim_table',):
    assert re.search(r'int32_t\s+%s\s*\(' % name, text), name
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
  for cite in ('embodied/jax/opt.py:109-123', 'embodied/jax/opt.py:126-143', 'embodied/jax/opt.py:146-164',
               'dreamerv3/agent.py:342-379', 'embodied/jax/opt.py:64-79'):
    assert cite in text, cite
  assert [len(_lib.SIGNATURES[name]) for name in NAMES] == [5, 17, 5, 1]
  assert _lib.lib.emb_abi_version() == 5                   # additions: the version stays
  sources = __import__('embodied_amd.build', fromlist=['SOURCES']).SOURCES
  assert 'optim.hip' in sources and 'optim_abi.cpp' in sources
  kernels_abi = (ROOT / 'embodied_amd' / 'csrc' / 'kernels_abi.cpp').read_text()
  assert 'optim' not in kernels_abi                        # that file is linked into the host sanitizer soak
  assert emb.LaProp is emb.optim.LaProp and emb.optimizer_launches() == emb.optim.optimizer_launches()
  header = (ROOT / 'embodied_amd' / 'csrc' / 'optim.h').read_text()
  assert re.search(r'kOptimChunk = (\d+);', header).group(1) == str(emb.optim.CHUNK)
  assert emb.optim.RECORD_BYTES == 48 and emb.optim.CHUNK % 4 == 0
  kernel = (ROOT / 'embodied_amd' / 'csrc' / 'optim.hip').read_text()
  assert 'atomicAdd' not in kernel and 'cooperative' not in kernel.lower()


def _table(addrs, counts, flags, want_chunks=True):
  """emb_optim_table through the raw binding: (status, records, chunk map)."""
  from embodied_amd import _lib, optim
  raw = _lib.lib.emb_optim_table
  raw.argtypes, raw.restype = _lib.SIGNATURES['emb_optim_table'], C.c_int32
  addrs, counts = np.asarray(addrs, np.int64).reshape(-1, 4), np.asarray(counts, np.int64)
  flags = np.asarray(flags, np.int32)
  n = C.c_int64(-1)
  status = raw(addrs.ctypes.data, counts.ctypes.data, flags.ctypes.data, len(counts), None, None, 0, C.byref(n), None, None)
  if status:
    return status, None, None
  table = np.zeros((len(counts), optim.RECORD_BYTES // 4), np.int32)
  chunks = np.full((n.value, 2), -7, np.int32)
  status = raw(addrs.ctypes.data, counts.ctypes.data, flags.ctypes.data, len(counts), table.ctypes.data,
               chunks.ctypes.data if want_chunks else None, n.value, None, None, None)
  return status, table, chunks


def test_table_builder():
  """The chunk map and the alignment decision over the tests' own size lists."""
  from embodied_amd import _lib, optim
  c = optim.CHUNK
  base = 0x7f0000000000
  for name, specs in cases.LISTS.items():
    counts = [int(np.prod(s.shape)) for s in specs]
    for bf16 in (0, 1):
      gsize = 2 if bf16 else 4
      addrs = [[base + 4 * (s.poff or 0), 2 * base + gsize * (s.goff or 0), 3 * base + 4 * (s.poff or 0),
                4 * base + 4 * (s.poff or 0)] for s in specs]
      status, table, chunks = _table(addrs, counts, [bf16 | (2 if i % 2 else 0) for i in range(len(specs))])
      assert status == 0, (name, _lib.lib.emb_last_error())
      assert len(chunks) == sum(-(-n // c) for n in counts)
      at = 0
      for i, (n, s) in enumerate(zip(counts, specs)):
        record = table[i]
        assert record[8] == n and record[9] == at and (record[10] & 3) == (bf16 | (2 if i % 2 else 0))
        assert record[:8].view(np.int64).tolist() == addrs[i]
        same = (s.poff or 0) % 4 == (s.goff or 0) % 4
        assert bool(record[10] & 4) == (same and n > 0), (name, i)
        assert record[11] == ((4 - (s.poff or 0) % 4) % 4 if same and n > 0 else 0)
        for k in range(-(-n // c)):
          assert chunks[at + k].tolist() == [i, k * c]
        at += -(-n // c)
  # moments at another offset than the parameter: scalar
  status, table, _ = _table([[base + 4, base * 2 + 4, base * 3, base * 4 + 4]], [100], [0])
  assert status == 0 and not table[0][10] & 4
  bad = [('more than 2^31 - 1 elements', dict(counts=[1 << 31])), ('more than 2^31 - 1 elements', dict(counts=[-1])),
         ('unknown flags', dict(flags=[4])), ('a null address', dict(addrs=[[base, 0, base, base]])),
         ('not aligned to its element', dict(addrs=[[base + 2, base, base, base]])),
         ('not aligned to its element', dict(addrs=[[base, base + 2, base, base]])),
         ('not aligned to its element', dict(addrs=[[base, base + 1, base, base]], flags=[1]))]
  for message, kw in bad:
    args = dict(addrs=[[base, base, base, base]], counts=[5], flags=[0])
    args.update(kw)
    status, _, _ = _table(**args)
    assert status == _lib.ERR_INVALID and message.encode() in _lib.lib.emb_last_error(), message
  # a bfloat16 gradient at an odd element is aligned to ITS element; a tensor of none needs no address
  assert _table([[base, base + 2, base, base]], [5], [1])[0] == 0
  assert _table([[0, 0, 0, 0]], [0], [0])[0] == 0
  # the largest tensor: 2^31 - 1 elements, and a total past 2^31 elements
  status, table, chunks = _table([[base] * 4] * 2, [(1 << 31) - 1] * 2, [0, 0])
  assert status == 0 and len(chunks) == 2 * (1 << 31) // c and chunks[-1].tolist() == [1, (1 << 31) - c]


def test_refusals_before_any_launch():
  from embodied_amd import _lib, optim
  fake = np.zeros(64, np.float32)          # never dereferenced on a device: every call below is refused first
  x = C.c_void_p(fake.ctypes.data)
  raws = {}
  for name in NAMES:
    raws[name] = getattr(_lib.lib, name)
    raws[name].argtypes, raws[name].restype = _lib.SIGNATURES[name], C.c_int32

  def update(table=x, chunks=x, n=3, partials=x, lr=1e-3, beta1=0.9, omb1=0.1, c1=0.1, beta2=0.999, omb2=0.001, c2=0.001,
             eps=1e-20, agc=0.3, pmin=1e-3, wd=0.0, nesterov=0):
    return raws['emb_optim_update'](table, chunks, n, partials, lr, beta1, omb1, c1, beta2, omb2, c2, eps, agc, pmin, wd,
                                    nesterov, None)

  before = optim.optimizer_launches()
  nan, inf = float('nan'), float('inf')
  refused = [('a pointer is null', dict(table=None)), ('a pointer is null', dict(chunks=None)),
             ('a pointer is null', dict(partials=None)), ('chunks is outside', dict(n=-1)), ('chunks is outside', dict(n=1 << 31)),
             ('lr must be finite', dict(lr=nan)), ('lr must be finite', dict(lr=inf)),
             ('a beta outside', dict(beta1=1.0)), ('a beta outside', dict(beta2=-0.1)), ('a beta outside', dict(beta1=nan)),
             ('1 - beta outside', dict(omb1=0.0)), ('1 - beta outside', dict(omb2=1.5)),
             ('a bias correction outside', dict(c1=0.0)), ('a bias correction outside', dict(c2=nan)),
             ('must be finite and not negative', dict(eps=-1.0)), ('must be finite and not negative', dict(agc=-0.3)),
             ('must be finite and not negative', dict(pmin=nan)), ('must be finite and not negative', dict(wd=inf)),
             ('nesterov must be', dict(nesterov=2))]
  for message, kw in refused:
    status = update(**kw)
    assert status == _lib.ERR_INVALID, (message, kw, status)
    assert message.encode() in _lib.lib.emb_last_error(), (message, _lib.lib.emb_last_error())
  assert raws['emb_optim_norms'](None, x, 3, x, None) == _lib.ERR_INVALID
  assert raws['emb_optim_norms'](x, x, -1, x, None) == _lib.ERR_INVALID
  assert raws['emb_optim_metrics'](x, 3, 10, None, None) == _lib.ERR_INVALID
  assert raws['emb_optim_metrics'](None, 3, 10, x, None) == _lib.ERR_INVALID
  assert raws['emb_optim_metrics'](x, 3, -1, x, None) == _lib.ERR_INVALID
  assert raws['emb_optim_launches'](None) == _lib.ERR_INVALID
  # no chunks: nothing to do, nothing launched, whatever the pointers are
  assert update(n=0, table=None, chunks=None, partials=None) == _lib.OK
  assert raws['emb_optim_norms'](None, None, 0, None, None) == _lib.OK
  assert optim.optimizer_launches() == before


@pytest.fixture
def on_host(monkeypatch):
  """The facade over host tensors: the device check is lifted, so the composed
  path and every refusal behind it can run without a device."""
  from embodied_amd import optim
  monkeypatch.setattr(optim, '_check_param', lambda index, param: None)
  return optim


def test_facade_refuses_host_tensors_and_other_dtypes():
  import embodied_amd as emb
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.LaProp([torch.zeros(3)])
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    emb.LaProp([torch.zeros(3, device='meta')])
  for dtype in (torch.float64, torch.bfloat16, torch.float16, torch.int32):
    with pytest.raises(TypeError, match='parameter 0 must be float32.*no CPU fallback'):
      emb.LaProp([torch.zeros(3, dtype=dtype), torch.zeros(3)])
  with pytest.raises(TypeError, match='not a tensor'):
    emb.LaProp([np.zeros(3, np.float32)])


def test_hyper_parameter_refusals(on_host):
  params = [torch.zeros(3), torch.zeros(2, 2)]
  for kw, match in ((dict(beta1=1.0), 'beta1'), (dict(beta2=-0.1), 'beta2'), (dict(beta1=float('nan')), 'beta1'),
                    (dict(agc=-0.3), 'agc'), (dict(pmin=-1e-3), 'pmin'), (dict(eps=-1e-20), 'eps'), (dict(wd=-0.1), 'wd'),
                    (dict(wd=float('inf')), 'wd'), (dict(warmup=-1), 'warmup'), (dict(warmup=2.5), 'warmup'),
                    (dict(lr=float('nan')), 'lr'), (dict(lr=lambda count: 1.0, warmup=3), 'callable'),
                    (dict(wd_mask=[True]), 'wd_mask has 1 entries for 2'), (dict(wd_mask=[True] * 3), 'wd_mask has 3')):
    with pytest.raises(ValueError, match=match):
      on_host.LaProp(params, **kw)
  with pytest.raises(ValueError, match='one parameter group'):
    on_host.LaProp([{'params': params[:1]}, {'params': params[1:]}])
  opt = on_host.LaProp(params, fused=False)
  assert opt.wd_mask == (False, True)                    # None: dim() >= 2, the reference's /kernel$
  params[0].grad = torch.ones(3)
  with pytest.raises(ValueError, match='parameter 1 has no gradient'):
    opt.step()
  assert opt.param_groups[0]['updates'] == 0 and not params[0].any()      # refused before anything moved
  params[1].grad = torch.ones(2, 2, dtype=torch.float64).to(torch.float32)
  params[0].grad_dtype = None
  params[0].grad = torch.ones(3, dtype=torch.float16)
  with pytest.raises(TypeError, match='gradient of parameter 0 must be float32 or bfloat16'):
    opt.step()
  with pytest.raises(RuntimeError, match='no step yet'):
    opt.metrics()


def test_path_decision(on_host):
  optim = on_host
  flat = torch.zeros(12)
  plain, view, strided = torch.zeros(3, 4), flat[1:7], torch.zeros(4, 3).t()
  assert optim._path(None, [plain, view]) is True and optim._path(True, [plain, view]) is True
  assert optim._path(False, [plain, view]) is False
  assert optim._path(None, [plain, strided]) is False and optim._path(False, [strided]) is False
  with pytest.raises(ValueError, match=r'fused=True.*parameter 1 of shape \(3, 4\) is not contiguous'):
    optim._path(True, [plain, strided])
  huge = torch.empty(1 << 31, device='meta')
  assert optim._path(None, [huge]) is False and optim._path(None, [huge[:-1]]) is True
  with pytest.raises(ValueError, match=r'fused=True.*2\^31 - 1 per tensor'):
    optim._path(True, [huge])
  assert optim.LaProp([plain, strided]).fused is False and optim.LaProp([plain, view]).fused is True
  with pytest.raises(ValueError, match='fused=True'):
    optim.LaProp([strided], fused=True)


def test_warmup_schedule():
  from embodied_amd import optim
  lr, w = 4e-5, 5
  sched = optim.warmup_schedule(lr, w)
  assert [sched(count) for count in (0, 1, w - 1, w, w + 1)] == [0.0, lr / w, lr * (w - 1) / w, lr, lr]
  assert [optim.warmup_schedule(lr, 0)(count) for count in (0, 1, 100)] == [lr] * 3
  assert sched(1) == cases.schedule(lr, w, 1) and sched(w - 1) == cases.schedule(lr, w, w - 1)


def test_composed_path_is_the_restatement(on_host):
  """The composed path over host tensors equals `cases.restate` in float32 bit
  for bit (the same torch operations in the same order), a callable lr sees the
  number of updates so far, and `state_dict` carries the moments and the count."""
  for case in (0, 37, 95, len(cases.FULL) + 1):
    c = cases.CASES[case]
    specs = cases.LISTS[c.list]
    inp = cases.inputs(case)
    want = cases.restate(inp, c.hyper, specs, torch.float32)
    params = [torch.from_numpy(x.copy()) for x in inp['p']]
    seen = []

    def lr(count, h=c.hyper, seen=seen):
      seen.append(count)
      return cases.schedule(h.lr, h.warmup, count)

    opt = on_host.LaProp(params, lr=lr, agc=c.hyper.agc, wd=c.hyper.wd, nesterov=c.hyper.nesterov, fused=False)
    for step in range(cases.STEPS):
      for param, g in zip(params, inp['g'][step]):
        param.grad_dtype = None
        param.grad = torch.from_numpy(g).to(torch.bfloat16 if c.hyper.bf16 else torch.float32)
      opt.step()
      for i, param in enumerate(params):
        assert np.array_equal(param.numpy(), want[step]['p'][i]), (case, step, i)
        assert np.array_equal(opt.state[param]['nu'].numpy(), want[step]['nu'][i])
        assert np.array_equal(opt.state[param]['mu'].numpy(), want[step]['mu'][i])
      m = opt.metrics()
      got = np.array([float(m[key]) for key in cases.METRICS], np.float32)
      assert np.array_equal(got, want[step]['metrics']), (case, step)
      assert m['updates'] == step + 1 and m['param_count'] == sum(x.size for x in inp['p'])
    assert seen == [0, 1, 2, 3]
    saved = opt.state_dict()
    assert saved['param_groups'][0]['updates'] == cases.STEPS and len(saved['state']) == len(params)


# ---- the lists past the first iteration of the kernels' loops (tests/optim_sweep_cases.py)

def test_the_sweep_lists_exceed_the_constants_they_are_about():
  from tests import optim_sweep_cases as sweep
  k = sweep.K
  kernel = (ROOT / 'embodied_amd' / 'csrc' / 'optim.hip').read_text()
  for loop in ('chunk += gridDim.x', 'k += kThreads', 'k += kMetricThreads'):
    assert loop in kernel, loop
  many, deep = sweep.LISTS['many'], sweep.LISTS['deep']
  assert len(many) == 2 * k['kMaxBlocks'] + 3 and all(1 <= int(np.prod(s.shape)) <= 5 for s in many)
  assert sweep.chunks(many) == len(many) > k['kMaxBlocks'] and sweep.chunks(many) > k['kMetricThreads']
  assert len(set(cases.mask_of(many))) == 2
  sizes = [int(np.prod(s.shape)) for s in deep]
  assert sizes == [sweep.DEEP, 3, sweep.DEEP] and -(-sweep.DEEP // cases.C) == k['kThreads'] + 2 > k['kThreads']
  assert sweep.DEEP % cases.C == 7                                        # a ragged last chunk
  assert (deep[2].poff, deep[2].goff) == (1, 1) and deep[0].poff is None  # head = 3 behind the small tensor
  assert [h.agc > 0 for h in sweep.HYPERS['deep']] == [True, True]
  assert [h.bf16 for h in sweep.HYPERS['deep']] == [False, True]
  assert sweep.HYPERS['many'] == cases.COVER and sweep.STEPS == {'many': cases.STEPS, 'deep': 2}


def test_tensors_that_share_a_workgroup_differ_in_agc_regime():
  """From float64 on step 1, at agc = 0.3: tensor i < kMaxBlocks is clipped,
  tensor i + kMaxBlocks (the same workgroup's next chunk) is not, and the last
  three have pnorm below pmin."""
  from tests import optim_sweep_cases as sweep
  blocks = sweep.BLOCKS
  agc = cases.COVER[0].agc
  assert agc == 0.3
  for bf16 in (False, True):
    inp = sweep.inputs('many', bf16)
    unorm = np.array([np.sqrt(np.square(g.astype(np.float64)).sum()) for g in inp['g'][0]])
    pnorm = np.array([np.sqrt(np.square(p.astype(np.float64)).sum()) for p in inp['p']])
    factor = 1 / np.maximum(1.0, unorm / (agc * np.maximum(cases.PMIN, pnorm)))
    assert (factor[:blocks] < 1).all() and factor[:blocks].max() < 0.9
    assert (factor[blocks:2 * blocks] == 1).all()
    assert (pnorm[2 * blocks:] < cases.PMIN).all() and (pnorm[:2 * blocks] > cases.PMIN).all()
    assert len(factor) == 2 * blocks + 3


@pytest.mark.parametrize('case', __import__('tests.optim_sweep_cases', fromlist=['CASES']).CASES,
                         ids=lambda case: f'{case[0]}{case[1]}')
def test_float32_definition_against_the_bars_on_the_sweep_lists(case):
  """`restate(..., torch.float32)` on every case of the sweep lists sits inside
  `ratio` and `ratio_nu` against `reference64`, every element and the metrics."""
  from tests import optim_sweep_cases as sweep
  name, i = case
  h = sweep.HYPERS[name][i]
  inp = sweep.inputs(name, h.bf16)
  assert len(inp['g']) == sweep.STEPS[name]
  want = sweep.reference(case)
  got = cases.restate(inp, h, sweep.LISTS[name], torch.float32)
  assert len(want) == len(got) == sweep.STEPS[name]
  worst = sweep.worst_ratios(got, want)
  print(f'float32 restated, {sweep.tag(case)}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()) + ' of its bar')
  assert max(worst.values()) <= 1.0, worst
