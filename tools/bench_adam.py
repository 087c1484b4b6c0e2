"""Cost of one `embodied_amd.optim.Adam` step: the kernels of csrc/optim.hip
against the composed torch ops of the same class, and against what a torch user
writes for the PPO learner's chain, `torch.nn.utils.clip_grad_norm_` followed by
`torch.optim.AdamW(fused=True)`.

    python tools/bench_adam.py [--calls 200] [--rounds 5] [--out profiles/adam_bench.txt]

Three parameter sets (those of tools/bench_optim.py), each with float32 and with
bfloat16 gradients:
  small    about 1 M parameters in 40 tensors
  ppo      the counted PPO model (tools/count_params.py), 12.2 M parameters
  dreamer  the 166 M-parameter DreamerV3 model, its tensors' shapes from the same walk

  us        time between two device events around `calls` back-to-back steps
            ending in a synchronise, after a warm-up; the paths alternate inside
            every round; median of the rounds [min .. max].
  host us   wall time of the same calls up to the last enqueue, per step, measured
            from a drained device: what the host spends per step.
  ceiling   the fused step's algorithmic bytes per parameter -- the norms launch
            reads g, the update launch reads g, p, nu, mu and writes p, nu, mu:
            32 with float32 gradients, 28 with bfloat16 ones -- over its median
            time, as a share of the copy ceiling that DESIGN.md quotes.
  torch     clip_grad_norm_(params, 10) + AdamW(fused=True).step() on parameters
            and gradients of its own (it scales its gradients in place).  It
            takes gradients of the parameters' dtype only: with bfloat16 gradients
            the row says what it answered.

Every configuration (set x gradient dtype) is measured in a process of its own
under its own time limit; the tool stops at the first one that fails or runs out
of time and writes no file.  The last lines name the rows at which the fused
median is below the composed one and below torch's: what `optim._path` is set
from.  Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import math
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools import pathbench  # noqa: E402
from tools.pathbench import COPY_CEILING_GBS  # noqa: E402

LIMITS = {'small': 240, 'ppo': 300, 'dreamer': 540}       # seconds per configuration, start-up included
CLIP = 10.0


def measure(name, kind, args):
  """One configuration, in this process: prints its rows and a `verdict` line."""
  import torch
  from embodied_amd import optim
  from tools.bench_optim import parameter_sets
  assert torch.cuda.is_available(), 'bench_adam needs a GPU'
  shapes = dict(parameter_sets())[name]
  count = sum(math.prod(s) for s in shapes)
  torch.manual_seed(0)
  dtype = torch.float32 if kind == 'f32' else torch.bfloat16
  params = [torch.randn(s, device='cuda') * 0.05 for s in shapes]
  for p in params:
    p.grad_dtype = None
    p.grad = (torch.randn(p.shape, device='cuda') * 0.01).to(dtype)      # global norm above CLIP at every set
  opts = {'fused': optim.Adam(params, clip=CLIP, fused=True), 'composed': optim.Adam(params, clip=CLIP, fused=False)}
  steps = {k: opt.step for k, opt in opts.items()}
  refused = None
  try:
    own = [p.detach().clone() for p in params]
    for p, q in zip(own, params):
      p.grad_dtype = None
      p.grad = q.grad.clone()
    adamw = torch.optim.AdamW(own, lr=3e-4, eps=1e-7, weight_decay=0.0, fused=True)

    def torch_step():
      torch.nn.utils.clip_grad_norm_(own, CLIP)
      adamw.step()

    torch_step()
    torch.cuda.synchronize()
    steps['torch'] = torch_step
  except Exception as e:                                  # reported as what it is, not as a figure
    refused = f'{type(e).__name__}: {str(e).splitlines()[0][:240]}'
  got = pathbench.measure(steps, args.calls, args.rounds, warmup=(2, 3), floor=3)
  host = {k: statistics.median(pathbench.host_us(step, got[k].calls, sync=False) for _ in range(3))
          for k, step in steps.items()}
  plan = opts['fused']._plan
  assert opts['fused'].table_uploads == 1
  median = {k: v.median for k, v in got.items()}
  row = f'{name} {kind}'
  print('device: ' + pathbench.device_line()[2:])
  print(f'row:   {row}: {count} parameters in {len(shapes)} tensors, {plan["n_chunks"]} chunks of {optim.CHUNK}')
  for k in steps:
    print(f'row:     {k:<10}{pathbench.cell(got[k].values, got[k].calls, 10, " us")}'
          f'   host {host[k]:8.1f} us')
  if refused:
    print(f'row:     torch     not measured: {refused}')
  per = 32 if kind == 'f32' else 28
  rate = per * count / median['fused'] / 1e3
  print(f'row:     fused: {per} bytes per parameter, {rate:.0f} GB/s = {rate / COPY_CEILING_GBS:.2f} of the copy ceiling '
        f'({COPY_CEILING_GBS:.0f} GB/s)')
  against_torch = 'none' if 'torch' not in median else ('below' if median['fused'] < median['torch'] else 'not below')
  print(f'verdict: {row}|{"below" if median["fused"] < median["composed"] else "not below"}|{against_torch}', flush=True)


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=200)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'adam_bench.txt'))
  parser.add_argument('--sets', default='small,ppo,dreamer')
  parser.add_argument('--child', nargs=2, metavar=('SET', 'KIND'), help='measure one configuration in this process')
  args = parser.parse_args()
  if args.child:
    measure(args.child[0], args.child[1], args)
    return
  report = pathbench.Report('bench_adam.py', args, None, [      # the device: from the first configuration
      f'# Adam(lr=3e-4, clip={CLIP:g}, eps=1e-7, wd=0), the global norm above the clip; one step()',
      '# us: time between device events over back-to-back steps, per step: median of rounds [min .. max] (steps per round)',
      '# host us: wall time up to the last enqueue, per step',
      '# torch: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True) at the same commit, on tensors of its own',
  ])
  verdicts = []
  for name in args.sets.split(','):
    for kind in ('f32', 'bf16'):
      command = [sys.executable, str(pathlib.Path(__file__).resolve()), '--child', name, kind, '--calls', str(args.calls),
                 '--rounds', str(args.rounds)]
      try:
        done = subprocess.run(command, capture_output=True, text=True, timeout=LIMITS[name], cwd=str(ROOT))
      except subprocess.TimeoutExpired:
        sys.exit(f'bench_adam: {name} {kind} ran past its {LIMITS[name]} s; stopping, nothing written')
      if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        sys.exit(f'bench_adam: {name} {kind} failed with status {done.returncode}; stopping, nothing written')
      for line in done.stdout.splitlines():
        if line.startswith('device: ') and report.lines[1] is None:
          report.lines[1] = '# ' + line[len('device: '):]
        elif line.startswith('row: '):
          report.add(line[len('row: '):])
        elif line.startswith('verdict: '):
          verdicts.append(line[len('verdict: '):].split('|'))
  for title, column in (('composed', 1), ('torch', 2)):
    report.closing(f'fused median below the {title} median at', f'fused median not below the {title} median at',
                   wins=[v[0] for v in verdicts if v[column] == 'below'],
                   losses=[v[0] for v in verdicts if v[column] == 'not below'])
  report.write()


if __name__ == '__main__':
  main()
