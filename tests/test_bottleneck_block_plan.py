"""fuse_bottleneck_blocks (csrc/plan_common.hip): the res2 identity bottlenecks of a plan as one conv_block_kernel launch each,
against the same plan with ODT_FUSE_BLOCK=0 (conv1 launch + conv2 with the fused tail)."""
import copy

import numpy as np
import pytest

from common import assert_same_detections, small_config, weights_for
from object_detection_tracking_amd import models
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights

H, W = 96, 160
BLOCKS = [3, 1, 2, 3]      # res2: one stage entry + two identity blocks


def _force_fp16x2_tiles(monkeypatch):
  # (a 96 x 160 frame offers res2 four 256-row tiles: take the split kernels whatever the tile count, as the fused-tail test does)
  monkeypatch.setenv("ODT_CONV_SPLIT_MINTILES", "1"); monkeypatch.setenv("ODT_CONV_SPLIT3_MINTILES", "1")
  monkeypatch.setenv("ODT_CONV_SPLIT3_BM", "256")


def _taps(cfg):
  c = copy.copy(cfg)
  c.keep_taps = True
  return c


def _run(lib, cfg, w, frame, taps=("c2", "p2")):
  m = models.get_model(cfg, 0, weights=w, lib=lib)
  try:
    det = m.predict(frame)
    e = m.engine(1, H, W)
    t = {k: e.tap(k) for k in taps} if cfg.keep_taps else {}
    return det, t, e.describe(), [(nm, fl) for nm, fl, _, _ in e.profile_layers()]
  finally:
    m.close()


def test_res2_identity_blocks_run_as_one_kernel(backend, monkeypatch):
  """Knob on: both identity blocks of res2 are fused, their rows are named .../conv1+conv2+conv3[fp16x2] and carry the FLOPs of
  the records folded into them; detections agree with the knob-off plan at the end-to-end tolerances, c2 and p2 to 2e-5 of
  their |max|; the arena handle and the keep_taps handle are bit-identical."""
  name, lib = backend
  _force_fp16x2_tiles(monkeypatch)
  cfg = small_config(resnet_num_block=BLOCKS, conv_split_family=0)
  w = weights_for(cfg)
  fr = synthetic_frames(1, H, W, seed=5)[0]
  out = {}
  for mode in ("0", "1"):
    monkeypatch.setenv("ODT_FUSE_BLOCK", mode)
    out[mode] = _run(lib, _taps(cfg), w, fr)
  monkeypatch.delenv("ODT_FUSE_BLOCK")
  d0, d1 = out["0"][2], out["1"][2]
  assert d0["bottleneck_blocks_fused"] == 0 and d1["bottleneck_blocks_fused"] == 2, (d0, d1)
  assert d0["bottleneck_tails_fused"] == d1["bottleneck_tails_fused"] >= 2
  names1 = [nm for nm, _ in out["1"][3]]
  for b in (1, 2):
    assert "group0/block%d/conv1+conv2+conv3[fp16x2]" % b in names1, names1
    assert any(nm.startswith("group0/block%d/conv1[fused into" % b) for nm in names1), names1
    assert any(nm.startswith("group0/block%d/conv3[fused into" % b) for nm in names1), names1
  assert "group0/block0/conv1[fp16x2]" in names1            # the stage entry keeps its launches
  fl0, fl1 = sum(f for _, f in out["0"][3]), sum(f for _, f in out["1"][3])
  assert fl0 == fl1 > 0, (fl0, fl1)
  for k in ("c2", "p2"):
    a, b = out["1"][1][k], out["0"][1][k]
    err = float(np.abs(a - b).max() / np.abs(b).max())
    print("bottleneck blocks %s: %s differs by %.3e of its |max|" % (name, k, err))
    assert err <= 2e-5, (k, err)
  assert_same_detections(*out["1"][0], *out["0"][0], 1e-3, 1e-4, 2e-4)
  # default knob (on), production handle: the arena keeps x alive to the end of the block
  prod = _run(lib, cfg, w, fr)
  assert prod[2]["bottleneck_blocks_fused"] == 2 and prod[2]["memory"]["keep_taps"] == 0
  for a, b in zip(prod[0], out["1"][0]):
    assert np.array_equal(a, b), "arena and keep_taps handles disagree"


@pytest.mark.parametrize("variant", ["use_se", "basic_block", "bf16x3_only"])
def test_blocks_not_fused_outside_the_rule(backend, monkeypatch, variant):
  """SE bottlenecks, basic blocks and a bf16x3-only handle keep their launches."""
  name, lib = backend
  _force_fp16x2_tiles(monkeypatch)
  kw = {"use_se": dict(use_se=True, conv_split_family=0), "basic_block": dict(use_basic_block=True, conv_split_family=0),
        "bf16x3_only": dict(conv_split_family=3)}[variant]
  cfg = small_config(resnet_num_block=BLOCKS, **kw)
  m = models.get_model(cfg, 0, weights=synthetic_weights(cfg, 0), lib=lib)      # (the variant's own variables: SE gates, 3x3 conv1)
  try:
    d = m.engine(1, H, W).describe()
  finally:
    m.close()
  assert d["bottleneck_blocks_fused"] == 0, d
