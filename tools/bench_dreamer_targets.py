"""Cost of DreamerV3's imagination targets of one train step: the chain as the
parent commit could write it, the composed path and the fused launch.

    python tools/bench_dreamer_targets.py [--calls 2000] [--rounds 5] [--out profiles/dreamer_targets_bench.txt]

For every shape the same work -- update on, contiguous float32 inputs, the
shipped normalisers (dreamerv3/configs.yaml:111-113: retnorm 'perc', valnorm and
advnorm 'none') -- on three paths:

  parent    what the library offered before `lambda_return_cont` and
            `dreamer_targets`: torch ops, the reference's own
            `for t in reversed(range(H))` loop for the scan (there was no
            float-continuation scan), torch.cumprod, `DeviceNormalize.normalize`.
  composed  `scans.dreamer_targets(fused=False, out=...)`.
  fused     `scans.dreamer_targets(fused=True, out=...)`: one launch.

  us/call    host clock around back-to-back calls that end in a device
             synchronise, after a warm-up of the same shape; the paths alternate
             inside every round, the figure is the median round (min .. max in
             brackets).  A path's calls per round are `--calls`, or as many as
             fit into about 0.3 s by its warm-up (the parent's loop over 1023
             steps takes milliseconds per call).  Back-to-back calls cost the
             larger of the host's enqueue time and the device's time.
  launches   device operations (kernels, copies) per call in a torch.profiler
             window of its own.

The last lines name the shapes at which the fused path beats the composed one
with a median outside the spread of the rounds: what
`scans.DREAMER_TARGETS_FUSED_MAX` is set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402
from tools.pathbench import host_us  # noqa: E402

SHAPES = [(16, 16), (256, 16), (1024, 16), (1024, 17), (16, 1024), (4096, 16)]   # the last: composed (and parent) only
LAM = 0.95


def parent_chain(rew, con, pred, retnorm, valnorm, advnorm, disc=1.0, lam=LAM):
  """dreamerv3/agent.py:397-419 and :482-490 with torch ops and DeviceNormalize."""
  voffset, vscale = valnorm.latest()
  tarval = pred * vscale + voffset
  weight = torch.cumprod(disc * con, 1) / disc
  live = (1 - (1 - con))[:, 1:] * disc
  interm = rew[:, 1:] + (1 - lam) * live * tarval[:, 1:]
  rets = [tarval[:, -1]]
  for t in reversed(range(live.shape[1])):
    rets.append(interm[:, t] + live[:, t] * lam * rets[-1])
  ret = torch.stack(list(reversed(rets))[:-1], 1)
  adv = retnorm.normalize(ret, sub=tarval[:, :-1].contiguous())
  adv_normed = advnorm.normalize(adv)
  tar_normed = valnorm.normalize(ret)
  tar_padded = torch.cat([tar_normed, 0 * tar_normed[:, -1:]], 1)
  return ret, weight, adv, adv_normed, tar_padded


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=2000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'dreamer_targets_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_dreamer_targets needs a GPU'
  import embodied_amd as emb
  from embodied_amd import scans

  names = ('parent', 'composed', 'fused')
  device = (pathbench.device_line(arch=False) + '; imag_loss:397-419 with update, '
            "retnorm 'perc', valnorm and advnorm 'none', float32 contiguous inputs")
  report = pathbench.Report('bench_dreamer_targets.py', args, device, [
      '# us/call: median of rounds [min .. max], host clock over back-to-back calls + synchronise; (calls per round)',
      '# launches: device operations per call (torch.profiler window)',
      f'# {"shape":<11}{"returns":<9}' + ''.join(f'{name + " us/call":<38}' for name in names)
      + 'launches parent / composed / fused',
  ])
  gen = np.random.default_rng(0)
  wins, losses = [], []
  for N, T in SHAPES:
    rew, pred = (torch.from_numpy(gen.standard_normal((N, T)).astype(np.float32)).cuda() for _ in range(2))
    con = torch.from_numpy((0.9 + 0.1 * gen.random((N, T))).astype(np.float32)).cuda()
    fits = N * (T - 1) <= 16384
    paths, outs = {}, {}
    for name in names:
      if name == 'fused' and not fits:
        continue
      norms = [emb.DeviceNormalize(impl) for impl in ('perc', 'none', 'none')]
      if name == 'parent':
        paths[name] = lambda norms=norms: outs.__setitem__('parent', parent_chain(rew, con, pred, *norms))
      else:
        out = tuple(torch.empty(shape, device='cuda') for shape in ((N, T - 1), (N, T), (N, T - 1), (N, T - 1), (N, T)))
        outs[name] = out
        paths[name] = (lambda norms=norms, out=out, fused=name == 'fused':
                       scans.dreamer_targets(rew, con, pred, *norms, out=out, fused=fused))
    # the same results from all after one step from fresh statistics
    for call in paths.values():
      call()
    for name in paths:
      for a, b in zip(outs['composed'], outs[name]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), (N, T, name)
    calls = {}
    for name, call in paths.items():                # warm-up of this shape; sizes the rounds
      calls[name] = pathbench.sized(call, args.calls, warmup=(3, 10), budget_us=0.3e6, timer=host_us)
      host_us(call, max(calls[name] // 10, 1))
    got = pathbench.run_rounds(paths, calls, args.rounds, timer=host_us)
    seen = {name: None if args.no_profiler else pathbench.device_ops(paths[name], 5) for name in got}
    cell = lambda name: got[name].cell if name in got else 'does not fit one workgroup'
    count = lambda name: pathbench.count(seen[name]) if name in got else '-'
    if 'fused' in got:
      if pathbench.every_round_below(got['fused'], got['composed']):
        wins.append((N, T))
      elif not pathbench.median_below(got['fused'], got['composed']):
        losses.append((N, T))
    report.add(f'  {f"{N}x{T}":<11}{N * (T - 1):<9}' + ''.join(f'{cell(name):<38}' for name in names)
               + ' / '.join(count(name) for name in names))
  largest = max(wins, key=lambda shape: shape[0] * (shape[1] - 1)) if wins else None
  report.add('# fused beats composed, every round of one below every round of the other, at: '
             + (', '.join(f'{n}x{t}' for n, t in wins) or 'no measured shape')
             + (f'; largest: {largest[0]}x{largest[1]} = {largest[0] * (largest[1] - 1)} returns' if largest else ''),
             '# fused does not beat composed (median) at: ' + (', '.join(f'{n}x{t}' for n, t in losses) or 'no measured shape'))
  report.write()


if __name__ == '__main__':
  main()
