"""What the reference's own code computed, recorded for the tests that compare
against it (`tests/golden/reference_runs.json`, written by
`python -m oracle.gen_reference_runs` in the build container).

A test registers the function that runs the reference (`@recorded(name)`) and
asks `check(name)` for the result: where the reference tree is readable the
function runs afresh and must reproduce the record; elsewhere the record stands
in for it.  Results are JSON values; arrays are recorded by `digest`."""
import hashlib
import json
import pathlib

import numpy as np

PATH = pathlib.Path(__file__).resolve().parent / 'golden' / 'reference_runs.json'
RUNS = {}


def recorded(name):
  def register(fn):
    RUNS[name] = fn
    return fn
  return register


def plain(value):
  """JSON form of a result: tuples -> lists, numpy scalars / arrays -> Python."""
  if isinstance(value, dict):
    return {str(k): plain(v) for k, v in value.items()}
  if isinstance(value, (list, tuple)):
    return [plain(v) for v in value]
  if isinstance(value, np.ndarray):
    return plain(value.tolist())
  if isinstance(value, np.generic):
    return value.item()
  return value


def digest(arrays):
  """sha256 over the sorted keys of a dict of arrays: name, dtype, shape, bytes."""
  h = hashlib.sha256()
  for key in sorted(arrays):
    a = np.ascontiguousarray(np.asarray(arrays[key]))
    h.update(f'{key}|{a.dtype.str}|{a.shape}|'.encode())
    h.update(a.tobytes())
  return h.hexdigest()


def load():
  with open(PATH) as f:
    return json.load(f)


def check(name):
  from oracle import refload
  want = load()[name]
  if refload.available():
    fresh = plain(RUNS[name]())
    assert fresh == want, f'{name}: the record is stale (python -m oracle.gen_reference_runs)'
  return want
