"""Writes tests/golden/plan_layout.json, the fixture of tests/test_plan_layout.py.  Run it from the commit whose plans are to
be pinned (the parent of a change to the plan builders), never from the code under test:

  python tests/golden/make_plan_layout.py record emu emu.json      # the simulator's section
  python tests/golden/make_plan_layout.py record hip hip.json      # the MI355X's section (needs the GPU)
  python tests/golden/make_plan_layout.py merge <parent commit> emu.json hip.json tests/golden/plan_layout.json

merge puts what the two backends agree on into each case's "common" and the rest under the backend's name.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def record(backend, out):
  from object_detection_tracking_amd import _lib
  from object_detection_tracking_amd.build import build_emu
  import test_plan_layout as T
  lib = _lib.get_lib() if backend == "hip" else _lib.OdtLib(build_emu())
  snaps = {case: T.snapshot(lib, case, os.environ.__setitem__, os.environ.__delitem__) for case in sorted(T.CASES)}
  with open(out, "w") as f:
    json.dump(snaps, f, sort_keys=True)


def merge(parent, emu, hip, out):
  with open(emu) as f:
    e = json.load(f)
  with open(hip) as f:
    h = json.load(f)
  assert sorted(e) == sorted(h)
  cases = {}
  for case in sorted(e):
    assert sorted(e[case]) == sorted(h[case])
    same = [k for k in e[case] if e[case][k] == h[case][k]]
    cases[case] = {"common": {k: e[case][k] for k in same},
                   "emu": {k: v for k, v in e[case].items() if k not in same},
                   "hip": {k: v for k, v in h[case].items() if k not in same}}
  with open(out, "w") as f:
    json.dump({"parent": parent, "cases": cases}, f, sort_keys=True, separators=(",", ":"))
    f.write("\n")


if __name__ == "__main__":
  if sys.argv[1] == "record":
    record(*sys.argv[2:4])
  else:
    merge(*sys.argv[2:6])
