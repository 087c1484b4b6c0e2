"""Shapes and seeded inputs of the sweep over the three newest users of
`scan_piece4<W>` (csrc/scan_segment.h): `scans.lambda_return_cont`,
`scans.dreamer_targets` and `scans.ppo_targets`.

Shared by tests/test_gpu_target_sweeps.py (which runs the kernels at them) and
tests/test_target_reference_host.py (which shows, without a GPU, that float32
arithmetic alone stays inside the 1e-5 bar at every one of them).  Plain numpy.

Where the lists come from -- the kernels' own constants:

  * one workgroup of THREADS = 1024 lanes (kNormThreads) runs a fused launch;
  * a row of n = T - 1 steps is scanned by a segment of W lanes, four steps per
    lane, W chosen from n alone (`width` below, the ladder of launch_scan,
    launch_ppo_targets and launch_dreamer_targets);
  * so a workgroup holds SEGMENTS = THREADS / W rows at a time: one row more
    than that is a second `b0 += kSegments` sweep in which every segment but
    the first is dead;
  * a row longer than SPAN = 4 W steps is walked in pieces of SPAN steps; only
    W = 64 has such rows (n > 256), the other widths end at n = 4 W;
  * the last lane of a row owns n % 4 steps (4 when that is 0): the `valid`
    tail of load4 / store4 and of the coefficients;
  * the weight phase of the Dreamer kernel walks T = n + 1 columns: at n = 4 W
    its second piece holds exactly one column;
  * the Dreamer kernel keeps N * n <= LDS_MAX = 16384 (kNormLdsMax) keys.

Per width therefore: its first n (4 W / 2 + 1) with tails of 1, 2 and 3 steps,
its last n = 4 W (tail 4, the one-column weight piece) and the n before it; for
W = 64 also both sides of the piece boundaries at 256 and 512.  W = 4 is what
the older tests run (n <= 16); it gets the one thing they lack, a two-step tail
(n = 14) with more rows than a workgroup has segments (257 > 256).
"""
import numpy as np

f32 = np.float32

THREADS = 1024
LDS_MAX = 16384
WIDTHS = (4, 8, 16, 32, 64)


def width(n):
  return 4 if n <= 16 else 8 if n <= 32 else 16 if n <= 64 else 32 if n <= 128 else 64


LENGTHS = {
    4: (14,),
    8: (17, 18, 19, 20, 31, 32),
    16: (33, 34, 35, 63, 64),
    32: (65, 66, 67, 127, 128),
    64: (129, 130, 131, 255, 256, 257, 258, 511, 512, 513),
}


def rows(W):
  """Row counts per length: one row, a few, and one more than the workgroup has
  segments.  (Every N = 1 shape meets the host test's scale condition, so none
  had to grow.)"""
  return (3, THREADS // W + 1) if W == 4 else (1, 3, THREADS // W + 1)


def shapes(W):
  """(N, T) of one width, in the order the tests alternate their settings over."""
  return [(N, n + 1) for n in LENGTHS[W] for N in rows(W)]


def off16_shape(W):
  """The shape that also runs with every tensor one element past a 16-byte
  boundary: a two-step tail, three rows."""
  n = next(n for n in LENGTHS[W] if n % 4 == 2)
  return (3, n + 1)


def clip_shape(W):
  """The PPO shape whose `tarclip` bites: the width's longest rows, a full sweep
  of segments and one row."""
  return (rows(W)[-1], LENGTHS[W][-1] + 1)


STEPS = 3                                    # update, update, no update; state carried
UPDATES = (True, True, False)
NORM = dict(rate=0.01, limit=1e-8)           # embodied/jax/utils.py:18-19
DREAMER = dict(horizon=333, lam=0.95)        # dreamerv3/agent.py:389-390
PPO = dict(hor=200, lam=0.8)                 # ppo/agent.py:179
ALL3 = (('perc', {}), ('meanstd', {}), ('meanstd', {}))
SHIPPED = (('perc', {}), ('none', {}), ('none', {}))      # dreamerv3/configs.yaml:111-113


def dreamer_settings(index):
  """(normaliser specs, contdisc) of the index-th shape of a width: all four
  combinations come round."""
  return (ALL3 if index % 2 == 0 else SHIPPED), (index // 2) % 2 == 0


def dreamer_disc(contdisc):
  return 1.0 if contdisc else float(f32(1 - 1 / DREAMER['horizon']))


def dreamer_inputs(N, T, seed):
  """rew, pred ~ N(0, 1) f32; con ~ U[0.9, 1) f32 with about 3 % exact zeros and
  about 3 % exact ones (the generator of tests/test_gpu_dreamer_targets.py)."""
  gen = np.random.default_rng([seed, N, T])
  rew = gen.standard_normal((N, T)).astype(f32)
  con = (0.9 + 0.1 * gen.random((N, T))).astype(f32)
  pick = gen.random((N, T))
  con[pick < 0.03] = 0.0
  con[pick > 0.97] = 1.0
  pred = gen.standard_normal((N, T)).astype(f32)
  return rew, con, pred


def ppo_inputs(B, T, seed):
  """rew, pred ~ N(0, 1) f32; last ~ Bernoulli(.05), term ~ Bernoulli(.03) (the
  generator of tests/test_gpu_ppo_targets.py)."""
  gen = np.random.default_rng([seed, B, T])
  return (gen.standard_normal((B, T)).astype(f32), gen.standard_normal((B, T)).astype(f32),
          gen.random((B, T)) < 0.05, gen.random((B, T)) < 0.03)


# `lambda_return_cont` goes through launch_scan (csrc/scans.hip), which has
# three more kernels in front of the ladder: n <= 16 with B <= 8192 rows takes
# one step per lane (scan_rows_kernel<16>), n > 256 one workgroup per row
# (scan_long_rows_kernel: pieces of 64 * min(16, ceil(n / 64)) steps, 1024 from
# n = 961 on, so n = 1025 is its second piece and n = 2049 its third).  Every T
# of test_scans_at_every_row_length (tests/test_gpu_parity.py), both sides of
# those two piece boundaries, and 8193 rows at n <= 16 for scan_rows4_kernel<4>.
CONT_LENGTHS = (*range(2, 71), *range(126, 132), *range(254, 260), 300, 1025, 1026, 2049, 2050)
CONT_ROWS = (1, 3, 70)
CONT_MANY_ROWS = 8193
CONT_MANY_LENGTHS = (2, 4, 15, 16, 17)
CONT_DISCS = (1.0, float(f32(1 - 1 / 333)))
CONT_LAM = 0.95
CONT_SEED = 5


def cont_shapes(n_rows):
  return [(n_rows, T) for T in (CONT_MANY_LENGTHS if n_rows == CONT_MANY_ROWS else CONT_LENGTHS)]
