"""ResNeXt-32x4d backbones (--use_resnext; reference nn.py:524-549): end to end against the oracle running the literal block
(block_reference.resnext_block: torch's grouped conv under TensorFlow's 'SAME'), and the new kernel on its own
(csrc/conv_group.hip) against a float64 evaluation.

Tolerances are the project's own (test_e2e.py / test_se.py): trunk 2e-5 of the tensor maximum, boxes 1e-3 px, scores 1e-4,
appearance features 10x the trunk tolerance, mismatch budget 0.  Seed 0 weights and the standard synthetic frames: the oracle
and the CPU simulator agree on them with nothing unmatched, so no seed had to be moved off an NMS near-tie."""
import numpy as np
import pytest
import torch

from block_reference import check_batch_swap, run_multi, run_single, same_geometry, weights
from common import small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import synthetic_frames

F = np.float32
U = 2.0 ** -24           # unit roundoff of f32


# ------------------------------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("dil", [True, False])
def test_resnext_forward_single_small(backend, dil):
  """G = 4, 8, 16, 32, stride 1 (group0) and stride 2; with use_dilations the stride-2 + dilation-2 entry of group3 on a
  6 x 8 map ('SAME' pads it (1, 2)).  Fails on a tree without the feature: get_model raises NotImplementedError."""
  name, lib = backend
  cfg = small_config(use_resnext=True, resnet_num_block=[1, 1, 1, 1], use_dilations=dil)
  assert cfg.use_resnext and cfg.use_dilations is dil
  run_single(lib, cfg, 96, 128)


def test_resnext_forward_multi_small(backend):
  """b = 2: stride-1 blocks at every width and the stride-1 dilation-2 blocks of group3; batch swap bit for bit."""
  name, lib = backend
  cfg = small_config(use_resnext=True, resnet_num_block=[1, 2, 2, 2], use_dilations=True, im_batch_size=2,
                     rpn_test_post_nms_topk=48)
  run_multi(lib, cfg, 2, 96, 128, check=check_batch_swap(["c2", "c3", "c4", "c5"]))


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_resnext_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test.  "auto" builds
  the guard's bf16x3 twin (the identical grouped kernel) and ends on fp16x2 with a healthy guard -- which conv3 can only
  where the grouped conv recorded its output's range."""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]
  cfg = small_config(use_resnext=True, resnet_num_block=[1, 1, 1, 1], **kw)

  def check(m, e, d0, d, out, fr, ref):
    if mode == "f32":
      assert d["conv_arith"] == "exact f32 MFMA" and d["fp16x2_split_launches"] == 0, d
    elif mode == "split3":
      assert d["fp16x2_split_launches"] == 0 and d["policy"]["family"] == 3, d
    else:
      auto = d["conv_split_family_auto"]
      assert "auto" in d["range_guard"] and auto["chosen"].startswith("fp16x2"), d
      assert len(auto["checks"]) == 1 and auto["calibration_forwards_left"] == 0 and not auto["incomplete"], auto
      assert auto["checks"][0]["max_rel_diff"] <= auto["tolerance"], auto

  run_single(lib, cfg, 96, 128, check=check)


def test_resnext_two_forwards_bit_identical(backend):
  name, lib = backend
  cfg = small_config(use_resnext=True, resnet_num_block=[1, 1, 1, 1])
  fr = synthetic_frames(1, 96, 128)
  m = models.get_model(cfg, 0, weights=weights(cfg), lib=lib)
  try:
    a = m.predict(fr[0]); b = m.predict(fr[0])
    assert len(a[0]) > 0
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  finally:
    m.close()


# ------------------------------------------------------------------------------------------------- op level

def _ref64(x, w, bias, stride, dil, relu):
  """float64 grouped conv under 'SAME' and, per output, sum |x w| + |bias| for the term-count bound."""
  B, H, W, C = x.shape
  keff = 2 * dil + 1
  Ho, pt, pb = same_geometry(H, stride, keff)
  Wo, pl, pr = same_geometry(W, stride, keff)

  def conv(xa, wa, ba):
    xt = torch.nn.functional.pad(torch.from_numpy(xa).double().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = torch.nn.functional.conv2d(xt, torch.from_numpy(wa).double().permute(3, 2, 0, 1), torch.from_numpy(ba).double(),
                                   stride=stride, dilation=dil, groups=32)
    return y.permute(0, 2, 3, 1).numpy()

  ref = conv(x, w, bias)
  mag = conv(np.abs(x), np.abs(w), np.abs(bias))
  assert ref.shape == (B, Ho, Wo, C)
  return (np.maximum(ref, 0.0) if relu else ref), mag, (pt, pl)


# B = 2; 9 x 13 and 8 x 12: odd and even maps, more than one pixel run per row and a partial one, a partial 16-pixel MFMA
# tile; 1 x 5: a single row, every vertical neighbour outside; 3 x 3: W shorter than a thread's run of 4 pixels (and than 2 at
# stride 2, where Wo = 2); 5 x 37: a row longer than one 32-pixel MFMA tile step
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("stride,dil", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("C", [128, 256, 512, 1024])
def test_group_conv_against_float64(backend, C, stride, dil, relu):
  """|got - ref64| <= (9 G + 3) 2^-24 (sum |x w| + |bias|) per output: 9 G products and as many additions in f32, the bias,
  and the BN-free weights as given -- a term-count bound, not a tuned one.  The recorded |max| is max |out| bit for bit, and
  a second run is bit-identical."""
  name, lib = backend
  G = C // 32
  for H, W in ((9, 13), (8, 12), (1, 5), (3, 3), (5, 37)):
    rng = np.random.default_rng(C + 10 * H + W + 100 * stride + dil)
    x = rng.standard_normal((2, H, W, C)).astype(F)
    w = (rng.standard_normal((3, 3, G, C)) * np.sqrt(2.0 / (9 * G))).astype(F)
    bias = (rng.standard_normal(C) * 0.3).astype(F)
    ref, mag, pad = _ref64(x, w, bias, stride, dil, relu)
    out, amax = ops.group_conv(x, w, bias, stride=stride, dil=dil, relu=relu, lib=lib)
    assert out.shape == ref.shape and out.dtype == F
    tol = (9 * G + 3) * U * mag
    err = np.abs(out.astype(np.float64) - ref)
    print("group_conv C=%d s=%d d=%d relu=%d %dx%d: max err / bound = %.3f" % (C, stride, dil, relu, H, W, float((err / tol).max())))
    assert np.all(err <= tol), (H, W, float((err / tol).max()))
    assert np.float32(amax) == np.abs(out).max() and amax > 0, (H, W, amax, float(np.abs(out).max()))
    if not relu:
      assert out.min() < 0
    out2, amax2 = ops.group_conv(x, w, bias, stride=stride, dil=dil, pad=pad, out_hw=ref.shape[1:3], relu=relu, lib=lib)
    assert np.array_equal(out, out2) and amax == amax2


def test_group_conv_groups_are_separate(backend):
  """An input that is non-zero in one group only moves that group's outputs only (the others are relu(bias)), and exact
  integer data comes out exactly: a wrong channel, tap or group mapping cannot hide in a tolerance."""
  name, lib = backend
  rng = np.random.default_rng(5)
  for C in (128, 256, 512, 1024):
    G = C // 32
    x = np.zeros((1, 6, 7, C), F)
    g = 3 if C < 1024 else 31
    x[..., g * G:(g + 1) * G] = rng.integers(-4, 5, (1, 6, 7, G)).astype(F)
    w = rng.integers(-3, 4, (3, 3, G, C)).astype(F)
    bias = rng.integers(-2, 3, C).astype(F)
    ref, _, _ = _ref64(x, w, bias, 1, 1, False)
    out, _ = ops.group_conv(x, w, bias, relu=False, lib=lib)
    assert np.array_equal(out.astype(np.float64), ref), C
    other = np.ones(C, bool); other[g * G:(g + 1) * G] = False
    assert np.array_equal(out[..., other], np.broadcast_to(bias[other], out[..., other].shape))


def test_group_conv_rejects_bad_sizes(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  with pytest.raises(OdtError, match="128, 256, 512 or 1024"):
    ops.group_conv(np.zeros((1, 4, 4, 64), F), np.zeros((3, 3, 2, 64), F), np.zeros(64, F), lib=emu_lib)
  with pytest.raises(OdtError, match="output larger"):
    ops.group_conv(np.zeros((1, 4, 4, 128), F), np.zeros((3, 3, 4, 128), F), np.zeros(128, F), out_hw=(6, 6), lib=emu_lib)
