"""Host side of the device env's fused step (csrc/synth_fused.h) on tests/fake_hip:
every refusal of the launch behind emb_synth_env_step_fused and the layout of its
device block, checked by tests/fused_host/check.cpp.  The real table's offsets
are pinned where it is defined (static_asserts in csrc/step_device.h).  CPU only."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / 'embodied_amd' / 'csrc'


@pytest.fixture(scope='module')
def report(tmp_path_factory):
  gxx = shutil.which('g++')
  if not gxx:
    pytest.skip('no g++')
  binary = tmp_path_factory.mktemp('fused_host') / 'check'
  cmd = [gxx, '-std=c++17', '-O1', '-g', '-Wall', f'-I{ROOT / "tests" / "fake_hip" / "include"}', f'-I{CSRC}',
         str(ROOT / 'tests' / 'fake_hip' / 'fake_kernels.cpp'), str(ROOT / 'tests' / 'fused_host' / 'check.cpp'),
         '-o', str(binary)]
  res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stderr[-3000:]
  run = subprocess.run([str(binary)], capture_output=True, text=True, timeout=60)
  return run.returncode, run.stdout + run.stderr


def test_refusals_and_block_layout(report):
  status, text = report
  lines = text.strip().splitlines()
  assert status == 0 and lines[-1] == '0 failed', text
  assert sum(line.startswith('ok: ') for line in lines) >= 30, text
  for needle in ('prewrite_supported fails', 'foreign buffer', '32-bit offsets', '2-channel', 'head +0/+8',
                 'block +96'):
    assert any(needle in line for line in lines), needle


def test_launch_is_behind_the_refusal_and_the_handle_untouched():
  """replay_early_insert asks `step->refusal` before it changes the handle and
  before anything is launched; the entry point passes synth_fused_refusal."""
  text = (CSRC / 'replay_abi.cpp').read_text()
  body = text.split('void replay_early_insert(')[1]
  assert body.index('step->refusal(') < body.index('known.valid = false') < body.index('step->launch(')
  env = (CSRC / 'env_abi.cpp').read_text()
  assert 'emb::synth_fused_refusal' in env and 'knob("EMB_STEP_FUSED")' in env


def test_table_offsets_are_pinned_where_the_kernels_read_them():
  text = (CSRC / 'step_device.h').read_text()
  for name, offset in (('narrow', 16), ('carry', 208), ('words', 248)):
    assert re.search(r'static_assert\(offsetof\(PreTable, %s\) == %d' % (name, offset), text), name
