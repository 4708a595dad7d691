"""Deformable-conv detectors (--use_deformable; reference nn.py:469-485, 574-585, 1642-1712, deformable_helper.py): end to end
against the oracle running the literal block (deformable_reference.deform_block: torch gathers, per-image offsets), and the new
kernels on their own (csrc/conv_deform.hip) against float64 evaluations and exact integer data.

Tolerances are the project's own (test_e2e.py / test_se.py): trunk 2e-5 of the tensor maximum, boxes 1e-3 px, scores 1e-4,
appearance features 10x the trunk tolerance, mismatch budget 0.  Seed 0 weights and the standard synthetic frames: the oracle
and the CPU simulator agree on them with nothing unmatched, so no seed had to be moved off an NMS near-tie."""
import numpy as np
import pytest

import deformable_reference as R
from block_reference import check_batch_swap
from common import small_config, torch_conv_nhwc
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights

F = np.float32
U = 2.0 ** -24           # unit roundoff of f32


def _cfg(**kw):
  base = dict(use_deformable=True, use_dilations=False, resnet_num_block=[1, 1, 1, 1])
  base.update(kw)
  return small_config(**base)


# ------------------------------------------------------------------------------------------------- end to end

def test_deformable_forward_single_small(backend):
  """A 96 x 128 frame: deformable stage entries at C = 128 / 256 / 512 on 24 x 32, 12 x 16 and 6 x 8 maps, three launches.
  Fails on a tree without the feature: get_model raises NotImplementedError.  The trunk tolerance of 2e-5 holds as it is."""
  name, lib = backend
  cfg = _cfg()
  assert cfg.use_deformable and not cfg.use_dilations

  def check(m, e, d0, d, out, fr, ref):
    assert d0["deform_conv_launches"] == 3 and d["deform_conv_launches"] == 3, d
    # with keep_taps the offsets and the deformable output are tappable: offsets against the oracle's at the even positions
    for g, (h, w, C) in zip((1, 2, 3), ((24, 32, 128), (12, 16, 256), (6, 8, 512))):
      off = e.tap("group%d/block0/conv2_offset" % g)
      ref_off, H, W = R.captured["group%d/block0" % g]
      assert (H, W) == (h, w) and off.shape == (1, h // 2, w // 2, 18)
      assert np.abs(off - ref_off[:, ::2, ::2]).max() < 1e-4 * np.abs(ref_off).max()
      t2 = e.tap("group%d/block0/conv2" % g)
      assert t2.shape == (1, h // 2, w // 2, C) and t2.min() < 0      # no ReLU: signed

  R.run_single(lib, cfg, 96, 128, check=check)


def test_deformable_only_where_the_reference_has_it(backend):
  """[1, 4, 2, 3]: group1/block0 is not among its group's last three blocks -- plain, with conv2/bn -- groups 2 and 3 open with
  a deformable block."""
  name, lib = backend
  cfg = _cfg(resnet_num_block=[1, 4, 2, 3])
  w = R.weights(cfg)
  assert "group1/block0/conv2/bn/gamma" in w and "group1/block0/conv2_offset/W" not in w
  for g in (2, 3):
    assert "group%d/block0/conv2/bn/gamma" % g not in w and w["group%d/block0/conv2_offset/W" % g].shape[3] == 18

  def check(m, e, d0, d, out, fr, ref):
    assert d0["deform_conv_launches"] == 2 and d["deform_conv_launches"] == 2, d
    assert sorted(R.captured) == ["group2/block0", "group3/block0"]

  R.run_single(lib, cfg, 96, 128, w=w, check=check)


def test_deformable_forward_multi_small(backend):
  """b = 2 against the restatement with per-image offsets; each image is bit-identical at either position of the batch (the
  reference's helper would sample image i, channel c at the offsets of image (i C + c) mod B)."""
  name, lib = backend
  cfg = _cfg(im_batch_size=2, rpn_test_post_nms_topk=48)
  R.run_multi(lib, cfg, 2, 96, 128, check=check_batch_swap(["c2", "c3", "c4", "c5"]))


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_deformable_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test.  "auto" ends on
  fp16x2 with a healthy guard -- which conv3 + shortcut can only where the deformable conv recorded its output's range."""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]
  cfg = _cfg(**kw)

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

  R.run_single(lib, cfg, 96, 128, check=check)


def test_deformable_two_forwards_bit_identical(backend):
  name, lib = backend
  cfg = _cfg()
  fr = synthetic_frames(1, 96, 128)
  m = models.get_model(cfg, 0, weights=R.weights(cfg), lib=lib)
  try:
    a = m.predict(fr[0]); b = m.predict(fr[0])
    assert len(a[0]) > 0
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  finally:
    m.close()


def test_deformable_test_inputs_exercise_the_sampler():
  """A condition on the inputs of the end-to-end test, not a measurement: at every deformable block the reference offsets move
  the taps by pixels (max |offset| > 2), more than 90 % of the sample coordinates (the f32 sums the clamp receives) are
  fractional, and between 5 % and 60 % of them are clamped."""
  import oracle.graph as G
  cfg = _cfg()
  with R.deform_oracle(cfg):
    G.OracleModel(cfg, R.weights(cfg)).forward(synthetic_frames(1, 96, 128)[0])
    cap = dict(R.captured)
  assert sorted(cap) == ["group1/block0", "group2/block0", "group3/block0"]
  for pre, (off, H, W) in sorted(cap.items()):
    used = off[:, ::2, ::2]
    r, c, r_raw, c_raw = R.sample_coords(used, H, W)
    raw = np.stack([r_raw, c_raw]); cl = np.stack([r, c])
    fractional = float((raw != np.floor(raw)).mean())
    clamped = float((raw != cl).mean())
    print("%s %dx%d: |offset| max %.2f std %.2f, fractional %.3f, clamped %.3f" % (pre, H, W, np.abs(used).max(), used.std(), fractional, clamped))
    assert fractional > 0.9 and 0.05 <= clamped <= 0.6 and np.abs(used).max() > 2, (pre, fractional, clamped)


def test_deformable_unsupported_combinations(emu_lib):
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  with pytest.raises(ValueError, match="use_dilations"):
    models.get_model(_cfg(use_dilations=True), 0, weights=w, lib=emu_lib)
  for kw, what in ((dict(use_resnext=True), "use_resnext"), (dict(use_basic_block=True), "use_basic_block"), (dict(use_se=True), "use_se")):
    with pytest.raises(NotImplementedError, match=what):
      models.get_model(_cfg(**kw), 0, weights=w, lib=emu_lib)
  plain = {k: v for k, v in w.items() if "conv2_offset" not in k}
  with pytest.raises(NotImplementedError, match="group1/block0/conv2_offset/W"):
    models.get_model(cfg, 0, weights=plain, lib=emu_lib)
  # every other variable of the same seed is what a config without the flag draws, bit for bit
  base = synthetic_weights(_cfg(use_deformable=False), 0)
  for k, v in plain.items():
    assert np.array_equal(v, base[k]), k
  assert set(base) - set(plain) == {"group%d/block0/conv2/bn/%s" % (g, s) for g in (1, 2, 3)
                                    for s in ("gamma", "beta", "mean/EMA", "variance/EMA")}


def test_deformable_weights_survive_the_writers(tmp_path):
  """conv2_offset/{W,b} (a bias beside a BN-less conv2) come back from every writer / reader pair of the repository (.npz, TF
  checkpoint, frozen .pb), and config_from_weights reads use_deformable (and, with it, no dilations) off the tensors."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  np.savez(str(tmp_path / "d.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-3"), w)
  write_frozen_pb(str(tmp_path / "d.pb"), w)
  for got in (load_npz(str(tmp_path / "d.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "d.pb"))):
    assert set(got) >= set(w)
    for g in (1, 2, 3):
      for s in ("conv2_offset/W", "conv2_offset/b", "conv2/W"):
        k = "group%d/block0/%s" % (g, s)
        assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "d.pb")))
  assert c.use_deformable and not c.use_dilations and list(c.resnet_num_block) == [1, 1, 1, 1]
  assert not models.config_from_weights(synthetic_weights(_cfg(use_deformable=False), 0)).use_deformable


# ------------------------------------------------------------------------------------------------- op level

def _op_inputs(C, H, W, seed):
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((2, H, W, C)).astype(F)
  w = (rng.standard_normal((3, 3, C, C)) * np.sqrt(2.0 / (9 * C))).astype(F)
  w_off = (rng.standard_normal((3, 3, C, 18)) * 1.5 * np.sqrt(1.0 / (9 * C))).astype(F)
  b_off = (rng.standard_normal(18) * 0.5).astype(F)
  return x, w_off, b_off, w


# B = 2; 9 x 13 and 8 x 12: odd and even maps; 1 x 5: a single row, every vertical neighbour clamps; 2 x 2: a single output
# pixel; 5 x 67: Wo = 34, past one 32-pixel tile (and the 2 x 3 x 34 = 204 pixels are no multiple of it)
@pytest.mark.parametrize("C", [128, 256, 512])
def test_deform_conv_against_float64(backend, C):
  """Offsets: |got - ref64| <= (9 C + 2) 2^-24 (sum |x w| + |b|).  Output, against a float64 evaluation at the RETURNED f32
  offsets with the coordinate formed by one f32 addition: <= (9 C + 16) 2^-24 sum_n |W_n|^T (|lt| + |rt| + |lb| + |rb|) --
  term-count bounds, not tuned ones.  The recorded |max| is max |out| bit for bit, and a second run is bit-identical."""
  name, lib = backend
  for H, W in ((9, 13), (8, 12), (1, 5), (2, 2), (5, 67)):
    x, w_off, b_off, w = _op_inputs(C, H, W, C + 10 * H + W)
    out, amax, off = ops.deform_conv(x, w_off, b_off, w, lib=lib)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert out.shape == (2, Ho, Wo, C) and off.shape == (2, Ho, Wo, 18) and out.dtype == F and off.dtype == F
    ref_off, mag_off = R.offsets64(x, w_off, b_off)
    e_off = np.abs(off.astype(np.float64) - ref_off) / ((9 * C + 2) * U * mag_off)
    ref, mag = R.deform64(x, off, w)
    e_out = np.abs(out.astype(np.float64) - ref) / ((9 * C + 16) * U * mag)
    print("deform_conv C=%d %dx%d: offsets err / bound = %.4f, out err / bound = %.4f" % (C, H, W, e_off.max(), e_out.max()))
    assert e_off.max() <= 1.0, (H, W, float(e_off.max()))
    assert e_out.max() <= 1.0, (H, W, float(e_out.max()))
    assert np.float32(amax) == np.abs(out).max() and amax > 0 and out.min() < 0, (H, W, amax)
    out2, amax2, off2 = ops.deform_conv(x, w_off, b_off, w, lib=lib)
    assert np.array_equal(out, out2) and np.array_equal(off, off2) and amax == amax2


def _gather_exact(x, offs, w):
  """numpy gather of the deformable conv for offsets [18] shared by all pixels, in float64 (exact on small integer data with
  fractions of 0 or 1/2)."""
  B, H, W, C = x.shape
  Ho, Wo = (H + 1) // 2, (W + 1) // 2
  off = np.broadcast_to(np.asarray(offs, F), (B, Ho, Wo, 18))
  return R.deform64(x, off, w)[0]


def test_deform_conv_exact_on_integer_data(backend):
  """w_off = 0, so the offsets are b_off exactly; integer x and w; per-tap offsets from {0, +-1, +-0.5, +2, +-100}, different
  for rows and columns: array_equal against a numpy gather.  A row / column swap, a wrong tap order, a zero border instead of
  the clamp, ceil at an integer coordinate or the wrong sampling grid cannot hide in a tolerance.  With all offsets zero the
  interior equals the plain stride-2 conv (one pad row / column in front) exactly, the border the replicate-clamped gather."""
  name, lib = backend
  rng = np.random.default_rng(11)
  rows = [0, 1, -1, 0.5, -0.5, 2, 100, -100, 0.5]
  cols = [-0.5, 2, 0, -100, 1, 0.5, -1, 0, 100]
  b_off = np.stack([rows, cols], axis=1).reshape(18).astype(F)
  for C, (H, W) in ((128, (9, 13)), (256, (8, 12)), (512, (5, 7))):
    x = rng.integers(-4, 5, (2, H, W, C)).astype(F)
    w = rng.integers(-3, 4, (3, 3, C, C)).astype(F)
    w[:, :, :, 0] = np.arange(9 * C).reshape(3, 3, C) % 7 - 3          # an output channel that tells taps and channels apart
    w_off = np.zeros((3, 3, C, 18), F)
    out, amax, off = ops.deform_conv(x, w_off, b_off, w, lib=lib)
    assert np.array_equal(off, np.broadcast_to(b_off, off.shape)), C
    ref = _gather_exact(x, b_off, w)
    assert np.array_equal(out.astype(np.float64), ref), C
    assert np.float32(amax) == np.abs(out).max()
    # all offsets zero
    zero = np.zeros(18, F)
    out0, _, off0 = ops.deform_conv(x, w_off, zero, w, lib=lib)
    assert not off0.any()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    conv = torch_conv_nhwc(x, w, None, 2, 1, 1, 1, Ho, Wo, dtype=np.float64)
    yi = slice(1, Ho - 1 if H % 2 else Ho); xi = slice(1, Wo - 1 if W % 2 else Wo)      # taps inside the map: no clamp, no pad
    assert yi.stop - yi.start >= 1 and xi.stop - xi.start >= 1
    assert np.array_equal(out0[:, yi, xi].astype(np.float64), conv[:, yi, xi]), C
    assert np.array_equal(out0.astype(np.float64), _gather_exact(x, zero, w)), C
    assert not np.array_equal(out0[:, 0].astype(np.float64), conv[:, 0])              # the border is a clamp, not zero padding


def test_deform_conv_rejects_bad_sizes(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  with pytest.raises(OdtError, match="128, 256 or 512"):
    ops.deform_conv(np.zeros((1, 4, 4, 64), F), np.zeros((3, 3, 64, 18), F), np.zeros(18, F), np.zeros((3, 3, 64, 64), F), lib=emu_lib)


@pytest.mark.parametrize("C,Ha,Wa,ldc", [(128, 9, 13, 128), (128, 7, 16, 192), (256, 10, 14, 260), (512, 7, 13, 516)])
def test_deform_conv_reads_a_pitched_view(backend, C, Ha, Wa, ldc):
  """The plan hands the kernels t1 as a view (Tensor::H / W / C against h / w).  A [2,7,13,C] view inside a [2,Ha,Wa,ldc]
  allocation -- taller only, wider and more channels, every pitch at once with ldc no multiple of 8 -- whose every element
  outside the view is NaN gives the dense tensor's offsets, output and recorded |max| bit for bit: the same arithmetic in the
  same order, and no read past a row, a column or a channel of the view (a clamped neighbour or a padded tap included)."""
  name, lib = backend
  H, W = 7, 13
  x, w_off, b_off, w = _op_inputs(C, H, W, 3 * C + ldc)
  big = np.full((2, Ha, Wa, ldc), np.nan, F)
  big[:, :H, :W, :C] = x
  out, amax, off = ops.deform_conv(x, w_off, b_off, w, lib=lib)
  outv, amaxv, offv = ops.deform_conv(big, w_off, b_off, w, lib=lib, view=(H, W, C))
  assert np.isfinite(outv).all() and np.isfinite(offv).all()
  assert np.array_equal(off, offv) and np.array_equal(out, outv) and amax == amaxv


def test_deform_conv_view_rejects_bad_pitches(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  z = lambda *s: np.zeros(s, F)
  with pytest.raises(OdtError, match="bad sizes"):      # a view taller than its allocation
    ops.deform_conv(z(1, 4, 4, 128), z(3, 3, 128, 18), z(18), z(3, 3, 128, 128), lib=emu_lib, view=(5, 4, 128))
  with pytest.raises(OdtError, match="bad sizes"):      # a channel pitch that breaks the 16-byte loads
    ops.deform_conv(z(1, 4, 4, 130), z(3, 3, 128, 18), z(18), z(3, 3, 128, 128), lib=emu_lib, view=(4, 4, 128))
