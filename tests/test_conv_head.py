"""4-conv + FC box heads (--use_conv_frcnn_head; reference conv_frcnn_head, models.py:1110-1124), with and without GroupNorm:
end to end against the oracle running the literal head (conv_head_reference.head_oracle: torch; under use_gn nested with
gn_reference.gn_oracle), and the ROI GroupNorm kernel on its own (csrc/group_norm_roi.hip) against float64 evaluations and
exact integer data.

Tolerances are the project's own (test_group_norm.py): trunk and head taps 2e-5 of the tensor maximum, boxes 1e-3 px, scores
1e-4, appearance features 10x the trunk tolerance, mismatch budget 0.  The head taps are held to their 2e-5 against the literal
head evaluated on the engine's own RoI features; against the taps of the end-to-end oracle run they measure 1.4e-5 .. 6.3e-5
under use_gn (seeds 0 - 5, simulator and MI355X), which is the two sides' 5e-5 .. 2e-4 px of proposal difference carried through
ROIAlign and four normalised layers, not the head's error (5e-6): conv_head_reference.check_head_taps prints that figure and
says why it is not asserted.  Seed 0 weights and the standard synthetic frames: the
oracle and the CPU simulator agree on them with nothing unmatched in every configuration below, so no seed had to be moved off
an NMS near-tie.  96 x 128 frames, blocks [1, 1, 1, 1], 32 proposals; conv_frcnn_head_dim = 64 for cost, the real 256 once more
on the GPU."""
import numpy as np
import pytest

import conv_head_reference as R
from block_reference import check_batch_swap
from common import small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import conv_head_variables, synthetic_frames, synthetic_weights
from test_group_norm import U, _affine, _check64, _exact_case

F = np.float32
K = 32


def _cfg(**kw):
  base = dict(use_conv_frcnn_head=True, conv_frcnn_head_dim=64, resnet_num_block=[1, 1, 1, 1], rpn_test_post_nms_topk=K)
  base.update(kw)
  return small_config(**base)


# ------------------------------------------------------------------------------------------------- end to end

def test_conv_head_forward_single(backend):
  """The head without GroupNorm on the single-image graph: detections, the head_conv3 and head_fc taps, and what describe()
  says.  Fails on a tree without the feature: get_model raises NotImplementedError."""
  name, lib = backend
  cfg = _cfg()

  def check(m, e, d0, d, out, fr, ref):
    assert d["box_head"] == "4conv1fc" and d["roi_group_norms"] == 0 and d["group_norms"] == 0, d
    assert e.tap("head_conv3").shape == (K, 7, 7, 64) and e.tap("head_fc").shape == (1, 1, K, 1024)
    with pytest.raises(Exception, match="fc6"):
      e.tap("fc6")

  R.run_single(lib, cfg, 96, 128, check=check)


def test_conv_head_gn_forward_single(backend):
  """The head under use_gn: four ROI GroupNorms on top of the 25 frame-level layers, which describe() keeps counting apart."""
  name, lib = backend
  cfg = _cfg(use_gn=True)

  def check(m, e, d0, d, out, fr, ref):
    for x in (d0, d):
      assert x["box_head"] == "4conv1fc" and x["roi_group_norms"] == 4 and x["group_norms"] == 25, x
      assert x["roi_group_norm_floor_bytes"] == 4 * 8 * K * 49 * 64, x
    mean = e.tap("head_conv0/gn_mean").reshape(K, 32); var = e.tap("head_conv0/gn_var").reshape(K, 32)
    # (behind a ReLU: a group whose two channels are dead over the whole ROI has mean = var = 0 exactly)
    assert np.isfinite(mean).all() and (mean >= 0).all() and (var >= 0).all() and var.max() > 0

  R.run_single(lib, cfg, 96, 128, check=check)


def test_conv_head_gn_forward_multi(backend):
  """b = 2 under use_gn; each image -- its trunk taps, its rows of the head taps, its detections -- is bit-identical at either
  position of the batch."""
  name, lib = backend
  cfg = _cfg(use_gn=True, im_batch_size=2)
  swap = check_batch_swap(["c2", "c5", "p2", "p5"])

  def check(m, e, d0, d, out, fr):
    a = {t: e.tap(t).copy() for t in ("head_conv0", "head_conv3", "head_fc")}
    swap(m, e, d0, d, out, fr)                       # (leaves the engine on the swapped batch)
    for t, x in a.items():
      x = x.reshape((2, K) + x.shape[-3:] if t != "head_fc" else (2, K, -1))
      y = e.tap(t).reshape(x.shape)
      assert not np.array_equal(x[0], x[1]), t
      assert np.array_equal(x[0], y[1]) and np.array_equal(x[1], y[0]), t

  R.run_multi(lib, cfg, 2, 96, 128, check=check)


def test_conv_head_version5(backend):
  """version = 5: dilations and class-agnostic output layers behind the head."""
  name, lib = backend
  cfg = _cfg(version=5)
  assert cfg.use_frcnn_class_agnostic and cfg.use_dilations
  R.run_single(lib, cfg, 96, 128)


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_conv_head_gn_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test.  "auto" ends on
  fp16x2 with a healthy guard -- which head conv k + 1 and fc can only where the ROI GroupNorm recorded its output's range."""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]
  cfg = _cfg(use_gn=True, **kw)

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
      assert d["fp16x2_split_launches"] > 0, d

  R.run_single(lib, cfg, 96, 128, check=check)


@pytest.mark.gpu
def test_conv_head_gn_real_width_gpu(hip_lib):
  """conv_frcnn_head_dim = 256, the reference's default (the simulator runs 64 for cost): one workgroup per ROI, 13 quads per
  thread."""
  R.run_single(hip_lib, _cfg(use_gn=True, conv_frcnn_head_dim=256), 96, 128)


def test_conv_head_two_forwards_bit_identical(backend):
  name, lib = backend
  cfg = _cfg(use_gn=True)
  fr = synthetic_frames(1, 96, 128)
  m = models.get_model(cfg, 0, weights=R.weights(cfg), lib=lib)
  try:
    a = m.predict(fr[0]); b = m.predict(fr[0])
    assert len(a[0]) > 0
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  finally:
    m.close()


def test_conv_head_errors(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  cfg, cfg_gn = _cfg(), _cfg(use_gn=True)
  plain = synthetic_weights(_cfg(use_conv_frcnn_head=False), 0)
  with pytest.raises(NotImplementedError, match=r"use_conv_frcnn_head\) cannot be built from weights without its variables: missing fastrcnn/conv0/W"):
    models.get_model(cfg, 0, weights=plain, lib=emu_lib)
  w = synthetic_weights(cfg, 0)
  wg = synthetic_weights(cfg_gn, 0)
  no_gn_head = {k: v for k, v in wg.items() if not k.startswith("fastrcnn/gn")}
  with pytest.raises(NotImplementedError, match="without its variables: missing fastrcnn/gn0/gamma, fastrcnn/gn0/beta"):
    models.get_model(cfg_gn, 0, weights=no_gn_head, lib=emu_lib)
  # the library's own messages: a variable that is there in another shape, and one that went missing behind get_model's check
  bad = dict(w); bad["fastrcnn/conv1/W"] = bad["fastrcnn/conv1/W"][:, :, :32]
  m = models.get_model(cfg, 0, weights=bad, lib=emu_lib)
  try:
    with pytest.raises(OdtError, match=r"bad shapes for fastrcnn/conv1 \(W \[3,3,64,64\]"):
      m.engine(1, 96, 128)
    m.weights = {k: v for k, v in w.items() if k != "fastrcnn/conv2/b"}
    with pytest.raises(OdtError, match=r"missing 4-conv box head variables fastrcnn/conv2/\{W,b\} \(odt_config.use_conv_frcnn_head\)"):
      m.engine(1, 96, 128)
    m.weights = {k: v for k, v in w.items() if k != "fastrcnn/fc/b"}
    with pytest.raises(OdtError, match="missing/bad fastrcnn/fc/b"):
      m.engine(1, 96, 128)
  finally:
    m.close()
  m = models.get_model(cfg_gn, 0, weights=wg, lib=emu_lib)
  try:
    m.weights = {k: v for k, v in wg.items() if k != "fastrcnn/gn3/beta"}
    with pytest.raises(OdtError, match=r"missing GroupNorm variables fastrcnn/gn3/\{gamma,beta\}"):
      m.engine(1, 96, 128)
  finally:
    m.close()
  # refused combinations
  with pytest.raises(NotImplementedError, match="conv_frcnn_head_dim = 48"):
    models.get_model(_cfg(use_gn=True, conv_frcnn_head_dim=48), 0, weights=wg, lib=emu_lib)
  for flag in ("add_relation_nn", "use_att_frcnn_head"):
    with pytest.raises(NotImplementedError, match=flag):
      models.get_model(_cfg(**{flag: True}), 0, weights=w, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="add_relation_nn"):
    models.get_model(_cfg(use_conv_frcnn_head=False, add_relation_nn=True), 0, weights=plain, lib=emu_lib)


# ------------------------------------------------------------------------------------------------- weights

def test_conv_head_synthetic_weights_leave_the_rest_alone():
  """Every other variable of a seed is bit for bit what a config without the flag draws; fc6 / fc7 are absent; the gn{k}
  variables come with use_gn alone."""
  for gn in (False, True):
    cfg = _cfg(use_gn=gn, conv_frcnn_head_dim=96)
    w = synthetic_weights(cfg, 3)
    base = synthetic_weights(_cfg(use_gn=gn, use_conv_frcnn_head=False), 3)
    head = conv_head_variables(cfg)
    assert len(head) == (18 if gn else 10) and len(set(head)) == len(head) and set(head) <= set(w)
    assert head[:2] == ["fastrcnn/conv0/W", "fastrcnn/conv0/b"] and head[-2:] == ["fastrcnn/fc/W", "fastrcnn/fc/b"]
    assert ("fastrcnn/gn0/gamma" in head) == gn and (head.index("fastrcnn/gn0/gamma") == 2 if gn else True)
    assert set(w) - set(base) == set(head)
    assert set(base) - set(w) == {"fastrcnn/fc6/W", "fastrcnn/fc6/b", "fastrcnn/fc7/W", "fastrcnn/fc7/b"}
    for k, v in w.items():
      if k not in head:
        assert np.array_equal(v, base[k]), k
    assert w["fastrcnn/conv0/W"].shape == (3, 3, 256, 96) and w["fastrcnn/conv3/W"].shape == (3, 3, 96, 96)
    assert w["fastrcnn/conv2/b"].shape == (96,) and w["fastrcnn/fc/W"].shape == (96 * 49, 1024) and w["fastrcnn/fc/b"].shape == (1024,)
    if gn:
      assert w["fastrcnn/gn1/gamma"].shape == (96,) and 0.9 <= w["fastrcnn/gn1/gamma"].min() and w["fastrcnn/gn1/gamma"].max() <= 1.1
  assert conv_head_variables(_cfg(use_conv_frcnn_head=False)) == []
  assert synthetic_weights(_cfg(), 0)["fastrcnn/conv0/W"].shape[-1] == 64
  # (the default width is the reference's 256)
  assert small_config(use_conv_frcnn_head=True).conv_frcnn_head_dim == 256


def test_conv_head_weights_survive_the_writers(tmp_path):
  """The head's variables come back from every writer / reader pair of the repository (.npz, TF checkpoint, frozen .pb), and
  config_from_weights reads the flag and the width off fastrcnn/conv0/W."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz
  cfg = _cfg(use_gn=True)
  w = synthetic_weights(cfg, 0)
  np.savez(str(tmp_path / "h.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-3"), w)
  write_frozen_pb(str(tmp_path / "h.pb"), w)
  for got in (load_npz(str(tmp_path / "h.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "h.pb"))):
    assert set(got) >= set(w)
    for k in conv_head_variables(cfg):
      assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "h.pb")))
  assert c.use_conv_frcnn_head and c.conv_frcnn_head_dim == 64 and c.use_gn and c.fpn_frcnn_fc_head_dim == 1024
  assert list(c.resnet_num_block) == [1, 1, 1, 1]
  c = models.config_from_weights(synthetic_weights(_cfg(conv_frcnn_head_dim=128), 0))
  assert c.use_conv_frcnn_head and c.conv_frcnn_head_dim == 128 and not c.use_gn
  c = models.config_from_weights(synthetic_weights(_cfg(use_conv_frcnn_head=False), 0))
  assert not c.use_conv_frcnn_head and c.fpn_frcnn_fc_head_dim == 1024


# ------------------------------------------------------------------------------------------------- op level

def _rois(R_, h, w, C, rng):
  return (rng.standard_normal((R_, h, w, C)) * rng.uniform(0.5, 2.0, (R_, 1, 1, C)) + rng.standard_normal((R_, 1, 1, C))).astype(F)


# R = 5.  7 x 7: the plans' ROIs (49 pixels over 4 .. 32 pixel threads: ragged last pass); 1 x 1: C / 32 values per group; 8 x 8:
# the largest ROI, every register of a thread in use at C = 256 / 512.  C = 32: one channel per group, four groups in a quad;
# 64: two; 256: one workgroup per ROI, 64 quads; 512: two workgroups per ROI, 16 groups each; 96 / 288: quads that straddle a
# group boundary, thread tiles that leave threads idle (288: 36 quads x 7 pixel threads)
OP_SHAPES = [(C, h, w) for C in (32, 64, 256, 512) for (h, w) in ((7, 7), (1, 1), (8, 8))] + [(96, 7, 7), (288, 7, 7)]


@pytest.mark.parametrize("C,h,w", OP_SHAPES)
def test_group_norm_roi_against_float64(backend, C, h, w):
  """Against a float64 evaluation with the bounds of test_group_norm._check64; the recorded |max| is max |out| bit for bit (in
  _check64); a second run is bit-identical."""
  name, lib = backend
  rng = np.random.default_rng(C + 10 * h + w)
  x = _rois(5, h, w, C, rng)
  gamma, beta = _affine(C, rng)
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  _check64(out, amax, mean, var, x, gamma, beta, what="roi")
  assert out.min() < 0
  out2, amax2, mean2, var2 = ops.group_norm_roi(x, gamma, beta, lib=lib)
  assert np.array_equal(out, out2) and amax == amax2 and np.array_equal(mean, mean2) and np.array_equal(var, var2)


@pytest.mark.parametrize("C,ldc", [(256, 260), (64, 128), (512, 516)])
def test_group_norm_roi_reads_a_pitched_tensor(backend, C, ldc):
  """[5,7,7,C] inside a [5,7,7,ldc] allocation whose pad channels are NaN: the dense tensor's output, statistics and recorded
  |max| bit for bit, and nothing written past channel C."""
  name, lib = backend
  rng = np.random.default_rng(3 * C + ldc)
  x = _rois(5, 7, 7, C, rng)
  gamma, beta = _affine(C, rng)
  big = np.full((5, 7, 7, ldc), np.nan, F)
  big[..., :C] = x
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  _check64(out, amax, mean, var, x, gamma, beta, what="roi dense")
  outv, amaxv, meanv, varv = ops.group_norm_roi(big, gamma, beta, view=C, lib=lib)
  assert np.array_equal(outv[..., :C], out) and amax == amaxv and np.array_equal(mean, meanv) and np.array_equal(var, varv)
  assert not outv[..., C:].any()


@pytest.mark.parametrize("C", [32, 256, 512])
def test_group_norm_roi_permutation(backend, C):
  """A ROI moved to another row -- and into a tensor of another R -- gives the same bits."""
  name, lib = backend
  rng = np.random.default_rng(11 + C)
  x = _rois(5, 7, 7, C, rng)
  gamma, beta = _affine(C, rng)
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  perm = np.array([3, 0, 4, 2, 1])
  outp, amaxp, meanp, varp = ops.group_norm_roi(x[perm], gamma, beta, lib=lib)
  assert np.array_equal(outp, out[perm]) and amaxp == amax and np.array_equal(meanp, mean[perm]) and np.array_equal(varp, var[perm])
  out1, _, mean1, var1 = ops.group_norm_roi(x[3:4], gamma, beta, lib=lib)
  assert np.array_equal(out1[0], out[3]) and np.array_equal(mean1[0], mean[3]) and np.array_equal(var1[0], var[3])


def test_group_norm_roi_large_mean(backend):
  """x = 1000 + N(0, 1), C = 64, 7 x 7: |mean| / std ~ 1000.  The bounds of _check64 hold.  A condition on the input, checked
  here: numpy's f32 E[x^2] - mean^2 on the same data violates the var bound, so the input tells an f32 version of the kernel's
  formula from the f64 one."""
  import gn_reference
  name, lib = backend
  rng = np.random.default_rng(5)
  x = (1000.0 + rng.standard_normal((5, 7, 7, 64))).astype(F)
  gamma, beta = _affine(64, rng)
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  _check64(out, amax, mean, var, x, gamma, beta, what="roi large mean")
  _, mean64, var64, _, ex2, _ = gn_reference.group_norm64(x, gamma, beta)
  xg = x.reshape(5, 49, 32, 2)
  m32 = xg.mean(axis=(1, 3), dtype=F)
  v32 = (xg * xg).mean(axis=(1, 3), dtype=F) - m32 * m32
  assert v32.dtype == F
  assert (np.abs(v32.astype(np.float64) - var64) > 8 * U * var64 + 2.0 ** -40 * ex2).all()


@pytest.mark.parametrize("C", [64, 256, 512])
def test_group_norm_roi_exact_on_integer_data(backend, C):
  """array_equal on the _exact_case construction (C / 32 even, so that 49 C / 32 is even): a group / channel mix-up, a swapped
  ROI or a pixel read twice cannot hide in a tolerance."""
  name, lib = backend
  x, gamma, beta, m, y, rng = _exact_case(C, 7, 7, 7 * C + 7)
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  assert np.array_equal(mean, m) and np.array_equal(var, np.ones((2, 32), F))
  assert np.array_equal(out, y) and np.float32(amax) == np.abs(y).max()


def test_group_norm_roi_constant_rois(backend):
  """What rows past the proposal count look like: an all-zero ROI in front of conv0 gives beta exactly; behind a conv it is
  constant per channel (relu(b[c])), and the output is finite and within the float64 bounds."""
  name, lib = backend
  rng = np.random.default_rng(8)
  C = 256
  gamma, beta = _affine(C, rng)
  x = _rois(5, 7, 7, C, rng)
  x[1] = 0
  x[3] = np.maximum(rng.standard_normal(C), 0).astype(F)[None, None, :]
  out, amax, mean, var = ops.group_norm_roi(x, gamma, beta, lib=lib)
  assert np.isfinite(out).all() and np.isfinite(mean).all() and np.isfinite(var).all()
  assert not mean[1].any() and not var[1].any() and np.array_equal(out[1], np.broadcast_to(beta, (7, 7, C)))
  assert (var[3] > 0).all() and np.array_equal(out[3], np.broadcast_to(out[3, 0, 0], (7, 7, C)))
  keep = [0, 2, 3, 4]
  _check64(out[keep], np.abs(out[keep]).max(), mean[keep], var[keep], x[keep], gamma, beta, what="roi constant")
  assert np.float32(amax) == np.abs(out).max()


def test_group_norm_roi_rejects_bad_arguments(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  z = lambda *s: np.zeros(s, F)
  with pytest.raises(OdtError, match=r"group_norm_roi: C must be a multiple of 32 \(32 groups\) in \[32, 512\]"):
    ops.group_norm_roi(z(2, 7, 7, 48), z(48), z(48), lib=emu_lib)
  with pytest.raises(OdtError, match=r"group_norm_roi: C must be a multiple of 32 \(32 groups\) in \[32, 512\]"):
    ops.group_norm_roi(z(2, 7, 7, 544), z(544), z(544), lib=emu_lib)
  with pytest.raises(OdtError, match="group_norm_roi: a ROI holds at most 64 pixels"):
    ops.group_norm_roi(z(2, 9, 9, 64), z(64), z(64), lib=emu_lib)
  with pytest.raises(OdtError, match=r"group_norm_roi: a pixel stride \(ldc\) must be a multiple of 4"):
    ops.group_norm_roi(z(2, 7, 7, 66), z(64), z(64), view=64, lib=emu_lib)
