"""The conv policy's decisions, pinned: which kernel of the table (csrc/conv_split.hip: conv_select) runs a conv of a given
shape under a given policy and set of ODT_* knobs.

tests/golden/conv_choice.json was recorded from the commit named in its "parent" field -- the code BEFORE the kernel table
existed (conv_split_wanted -> conv_split_choose -> conv_finish), through a throwaway patch that gave that commit the same
odt_op_conv_choice entry point and printed the finished records of whole plans -- never from the code under test.  It holds
  "plans": the convs of the plans the benchmark and the full-size tests build (multi graph b = 8 / 24 and single graph b = 1
           at 1080p, families 2 and 3; EfficientDet D0 / D7), as the parent's plan builder finished them;
  "grid":  a synthetic grid across every threshold of the policy, evaluated under every entry of "settings" (default,
           the families, exact f32, every knob of conv_policy_with_knobs / conv_select at a non-default value, the exact-f32
           instantiations, the SPLIT_PIPES of test_ops.py).
A policy or kernel change shows up here as a diff of the fixture, to be reviewed.  The mapping fields -> kernel is not
in the fixture (the parent had no row names): tests/test_conv_rows.py runs every selectable row by name and checks, per
launch, that odt_op_conv_choice's fields and name are those of the record that was launched (ops.last_conv).
"""
import json
import os

import pytest

from object_detection_tracking_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "conv_choice.json")) as _f:
  FIX = json.load(_f)
FIELDS = tuple(FIX["fields"])
assert FIELDS == ops.CONV_CHOICE_OUT and tuple(FIX["shape_fields"]) == ops.CONV_CHOICE_SHAPE
# rows that no selection reaches: the fusions put them in place of a selected row (fuse_bottleneck_tails, fuse_stem)
SET_BY_FUSIONS = {"H2KF_256x64", "H2KF_256x128", "H2KF_256x256", "H2_STEM"}


def _choose(lib, monkeypatch, shape, arith, family, env):
  for k in [k for k in os.environ if k.startswith("ODT_")]:
    monkeypatch.delenv(k)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  return ops.conv_choice(shape, arith, family, lib=lib)


def _fields(d):
  return [d[f] for f in FIELDS]


@pytest.mark.parametrize("si", range(len(FIX["settings"])), ids=lambda i: "s%02d" % i)
def test_grid_choices_equal_the_recorded_ones(backend, si, monkeypatch):
  name, lib = backend
  st = FIX["settings"][si]
  bad = []
  for shape, ri in zip(FIX["shapes"], FIX["grid"][si]):
    got = _fields(_choose(lib, monkeypatch, shape, st["arith"], st["family"], st["env"]))
    if got != FIX["results"][ri]:
      bad.append((shape, FIX["results"][ri], got))
  assert not bad, "%d of %d choices differ under %r; first: %r" % (len(bad), len(FIX["shapes"]), st, bad[:3])


def test_plan_choices_equal_the_recorded_ones(backend, monkeypatch):
  name, lib = backend
  bad = []
  for p in FIX["plans"]:
    got = _fields(_choose(lib, monkeypatch, FIX["shapes"][p["shape"]], p["arith"], p["family"], {}))
    if got != FIX["results"][p["out"]]:
      bad.append((p["plan"], p["name"], FIX["results"][p["out"]], got))
  assert not bad, "%d of %d plan convs differ; first: %r" % (len(bad), len(FIX["plans"]), bad[:3])


def test_fixture_covers_the_table_and_every_knob(emu_lib, monkeypatch):
  """Conditions on the fixture itself: every row a selection can reach is chosen by some entry, every knob changes some entry,
  and a rejected record appears."""
  assert os.path.getsize(os.path.join(HERE, "golden", "conv_choice.json")) < 300 * 1024
  default = FIX["grid"][0]
  effect = {}      # knob -> one of its values changes some entry of the default policy's column
  for si, st in enumerate(FIX["settings"]):
    if len(st["env"]) == 1 and st["arith"] == 0 and st["family"] == 0:
      (knob,) = st["env"]
      effect[knob] = effect.get(knob, False) or FIX["grid"][si] != default
  # (21 knobs of conv_policy_with_knobs + H2_BK64, SPLIT_REDUCE_BLOCKS, TILE, SMALLK, STAGES, FINE of conv_select; ODT_CONV_DEBUG reaches no reported field)
  assert len(effect) == 27 and all(effect.values()), sorted(k for k, v in effect.items() if not v)
  assert any(FIX["results"][ri][0] == 2 for row in FIX["grid"] for ri in row), "no rejected record in the fixture"
  seen = set()
  for si, st in enumerate(FIX["settings"]):
    first = {}
    for shape, ri in zip(FIX["shapes"], FIX["grid"][si]):      # one call per distinct result is enough to name its row
      if ri not in first and FIX["results"][ri][0] != 2:
        first[ri] = shape
    for shape in first.values():
      seen.add(_choose(emu_lib, monkeypatch, shape, st["arith"], st["family"], st["env"])["name"])
  src = open(os.path.join(os.path.dirname(HERE), "object_detection_tracking_amd", "csrc", "odt_common.hpp")).read()
  block = src[src.index("X(F32_128x64_S1)"):src.index("enum ConvVariant : int")]      # the table's row list
  import re
  rows = set(re.findall(r"X\((\w+)\)", block))
  assert len(rows) == 40
  assert rows - seen - SET_BY_FUSIONS == set(), sorted(rows - seen - SET_BY_FUSIONS)
  assert seen <= rows
