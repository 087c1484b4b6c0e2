"""bench.py --dump-outputs (dump_outputs): names, dtypes, the seeded sample of
large arrays and the size bound.  CPU only: the function takes any tensors."""
import importlib.util
import pathlib

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def bench():
  spec = importlib.util.spec_from_file_location('_bench_for_dump_test', ROOT / 'bench.py')
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def _outputs():
  gen = torch.Generator().manual_seed(0)
  batch = {'image': torch.randint(0, 256, (16, 65, 84, 84, 4), dtype=torch.uint8, generator=gen),
           'reward': torch.randn(16, 65, generator=gen),
           'is_last': torch.rand(16, 65, generator=gen) < 0.1,
           'action': torch.randint(0, 6, (16, 65), dtype=torch.int32, generator=gen),
           'dyn/deter': torch.randn(16, 65, 8, generator=gen)}
  returns = {'advantage': torch.randn(16, 64, generator=gen), 'target': torch.randn(16, 64, generator=gen)}
  policy = torch.rand(64, 4, 84, 84, generator=gen).to(torch.bfloat16)
  return policy, {'batch': batch, 'returns': returns}


def test_dump_writes_every_output_in_float32_or_float64(bench, tmp_path):
  policy, last = _outputs()
  bench.dump_outputs(str(tmp_path), policy, last)
  files = {p.name: np.load(p) for p in tmp_path.iterdir()}
  assert set(files) == {'policy_batch.npy', 'batch_image.sample.npy', 'batch_reward.npy', 'batch_is_last.npy',
                        'batch_action.npy', 'batch_dyn_deter.npy', 'train_advantage.npy', 'train_target.npy'}
  assert files['batch_action.npy'].dtype == np.float64
  assert all(a.dtype == np.float32 for n, a in files.items() if n != 'batch_action.npy')
  np.testing.assert_array_equal(files['policy_batch.npy'], policy.float().numpy())
  np.testing.assert_array_equal(files['batch_reward.npy'], last['batch']['reward'].numpy())
  np.testing.assert_array_equal(files['batch_is_last.npy'], last['batch']['is_last'].numpy())
  np.testing.assert_array_equal(files['batch_action.npy'], last['batch']['action'].numpy())
  np.testing.assert_array_equal(files['train_target.npy'], last['returns']['target'].numpy())
  # the images (29 M elements) as a seeded sample: the elements at fixed sorted flat indices
  image = last['batch']['image'].reshape(-1)
  idx = np.unique(np.random.default_rng(image.numel()).integers(0, image.numel(), bench.DUMP_MAX_ELEMENTS))
  np.testing.assert_array_equal(files['batch_image.sample.npy'], image.numpy()[idx].astype(np.float32))
  assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= bench.DUMP_BYTES


def test_dump_stays_within_its_size_bound(bench, tmp_path, monkeypatch):
  monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 10**6)
  policy, last = _outputs()
  bench.dump_outputs(str(tmp_path), policy, last)
  sizes = {p.name: p.stat().st_size for p in tmp_path.iterdir()}
  assert sum(sizes.values()) <= 4 * 10**6 + 128 * len(sizes)       # (+ the .npy headers)
  assert 'policy_batch.sample.npy' in sizes and 'batch_reward.npy' in sizes
