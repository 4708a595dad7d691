"""What each plan is, pinned: the conv launches of a handle (name, flops, GEMM shape), the launch and fusion counts of
describe() and its memory figures, for one small handle per branch of the plan builders (csrc/plan_fpn.hip,
csrc/plan_effdet.hip).  No forward runs.

tests/golden/plan_layout.json was recorded by tests/golden/make_plan_layout.py from the commit named in its "parent" field
-- the plan builders BEFORE they were rewritten around ConvSpec and the stage functions -- on the simulator and on the
MI355X, never from the code under test.  Per case, "common" holds what the two backends agree on, "emu" / "hip" what they
do not (the kernel choice may depend on the device's CU count).  A change of a plan shows up here as a diff of the fixture,
to be reviewed.
"""
import json
import os

import pytest

from common import small_config
from object_detection_tracking_amd import models
from object_detection_tracking_amd.config import make_config
from object_detection_tracking_amd.efficientdet import arch
from object_detection_tracking_amd.weights import synthetic_weights

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "plan_layout.json")
H, W = 96, 160
EFF_S = 128          # the smallest EfficientDet frame of test_efficientnet.py
DESCRIBE = ("conv_launches", "convs_fused_into_epilogues", "exact_f32_mfma_launches", "bf16x3_split_launches",
            "fp16x2_split_launches", "bottleneck_tails_fused", "bottleneck_blocks_fused", "stem_fused", "se_blocks",
            "group_conv_launches", "deform_conv_launches", "convs_cut_into_batch_ranges")
MEMORY = ("device_bytes", "activation_arena_bytes", "arena_tensors", "dedicated_tensor_bytes")

# name -> (small_config overrides, ODT_* environment)
CASES = {
    "bottleneck": (dict(), {}),
    "bottleneck_no_dilations": (dict(use_dilations=False), {}),
    "bottleneck_b2": (dict(im_batch_size=2), {}),
    "bottleneck_b2_no_dilations": (dict(im_batch_size=2, use_dilations=False), {}),
    "separate_shortcut": (dict(), {"ODT_FUSE_SHORTCUT": "0"}),
    "keep_taps": (dict(keep_taps=True), {}),
    "se": (dict(version=6, resnet_num_block=[1, 1, 1, 1]), {}),
    "basic": (dict(resnet18=True), {}),
    "basic_no_dilations": (dict(resnet18=True, use_dilations=False), {}),
    "resnext": (dict(use_resnext=True, resnet_num_block=[1, 2, 1, 1]), {}),
    "resnext_no_dilations": (dict(use_resnext=True, resnet_num_block=[1, 2, 1, 1], use_dilations=False), {}),
    "deformable": (dict(use_deformable=True, use_dilations=False, resnet_num_block=[1, 1, 1, 1]), {}),      # test_deformable.py's
    "mask": (dict(add_mask=True, mrcnn_head_dim=64), {}),
    "split_family_3": (dict(conv_split_family=3), {}),
    "efficientdet_d0": (None, {}),
}


def snapshot(lib, case, setenv, delenv):
  """The pinned fields of the handle `case` builds on `lib`."""
  kw, env = CASES[case]
  for k in [k for k in os.environ if k.startswith("ODT_")]:
    delenv(k)
  for k, v in env.items():
    setenv(k, v)
  if kw is None:
    cfg = make_config(is_efficientdet=True, efficientdet_modelname="efficientdet-d0", short_edge_size=EFF_S, max_size=EFF_S)
    cfg.max_size = EFF_S
    m = models.get_model(cfg, 0, weights=arch.synthetic_det_weights("efficientdet-d0", 0), lib=lib)
  else:
    cfg = small_config(**kw)
    m = models.get_model(cfg, 0, weights=synthetic_weights(cfg, 0), lib=lib, is_multi=cfg.im_batch_size > 1)
  try:
    e = m.engine((EFF_S, EFF_S)) if kw is None else m.engine(cfg.im_batch_size, H, W)
    d = e.describe()
    snap = {"layers": [[name, flops, list(mnk)] for name, flops, _, mnk in e.profile_layers()]}
    snap.update({k: d[k] for k in DESCRIBE})
    snap.update({"memory." + k: d["memory"][k] for k in MEMORY})
    return snap
  finally:
    m.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_equals_the_recorded_one(backend, case, monkeypatch):
  name, lib = backend
  with open(FIXTURE) as f:
    fix = json.load(f)["cases"][case]
  want = dict(fix["common"])
  want.update(fix[name])
  got = snapshot(lib, case, monkeypatch.setenv, monkeypatch.delenv)
  assert sorted(got) == sorted(want)
  bad = [k for k in sorted(want) if got[k] != want[k] and k != "layers"]
  assert not bad, [(k, want[k], got[k]) for k in bad]
  assert len(got["layers"]) == len(want["layers"]), (len(got["layers"]), len(want["layers"]))
  diff = [(i, w, g) for i, (w, g) in enumerate(zip(want["layers"], got["layers"])) if w != g]
  assert not diff, "%d of %d conv launches differ; first: %r" % (len(diff), len(want["layers"]), diff[:3])
