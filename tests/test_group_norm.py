"""GroupNorm detectors (--use_gn; reference nn.py:81-108, 487-521, 859-862, 947-1014): end to end against the oracle running the
literal group_norm (gn_reference.gn_oracle: torch, statistics per image), and the new kernels on their own
(csrc/group_norm.hip) against float64 evaluations and exact integer data.

Tolerances are the project's own (test_e2e.py / test_se.py / test_deformable.py): trunk 2e-5 of the tensor maximum, boxes 1e-3
px, scores 1e-4, appearance features 10x the trunk tolerance, mismatch budget 0.  Seed 0 weights and the standard synthetic
frames: the oracle and the CPU simulator agree on them with nothing unmatched, so no seed had to be moved off an NMS near-tie."""
import numpy as np
import pytest

import gn_reference as R
from block_reference import check_batch_swap
from common import small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import group_norm_variables, synthetic_frames, synthetic_weights

F = np.float32
U = 2.0 ** -24           # unit roundoff of f32


def _cfg(**kw):
  base = dict(use_gn=True, resnet_num_block=[1, 1, 1, 1])
  base.update(kw)
  return small_config(**base)


# ------------------------------------------------------------------------------------------------- end to end

def _conv0_stats(cfg, w, frame):
  """mean / var [32] of the raw conv0 map of the oracle's graph, in float64."""
  import oracle.graph as G
  import torch
  import torch.nn.functional as TF
  with torch.no_grad():
    img = G.preprocess(np.asarray(frame)[None])
    H, W = img.shape[2:]
    mult = cfg.fpn_resolution_requirement
    ph = int(np.ceil(H / mult) * mult) - H; pw = int(np.ceil(W / mult) * mult) - W
    y = G.conv2d(TF.pad(img, (3, 2 + pw, 3, 2 + ph)), w, "conv0", stride=2, padding="VALID").double()
  yr = y.reshape(1, 32, 2, -1)
  return yr.mean(dim=(2, 3)).numpy(), yr.var(dim=(2, 3), unbiased=False).numpy()


def test_gn_forward_single_small(backend):
  """A 96 x 128 frame, blocks [1, 1, 1, 1], dilations on: 25 GroupNorm layers, channels per group from 2 (conv0, res2) to 64
  (C = 2048); the dilated group3/block0 normalises the 2 x 3 VALID result inside a 3 x 4 tensor whose first row and column stay
  zero.  Fails on a tree without the feature: get_model raises NotImplementedError.  The trunk tolerance of 2e-5 holds as it is."""
  name, lib = backend
  cfg = _cfg()
  assert cfg.use_gn and cfg.use_dilations

  def check(m, e, d0, d, out, fr, ref):
    assert d0["group_norms"] == 25 and d["group_norms"] == 25, d
    assert e.tap("c5").shape == (1, 3, 4, 2048)
    mean64, var64 = _conv0_stats(cfg, m.weights, fr[0])
    for scope in ("conv0", "fpn/gn_p2"):
      mean = e.tap(scope + "/gn_mean").reshape(1, 32); var = e.tap(scope + "/gn_var").reshape(1, 32)
      assert np.isfinite(mean).all() and (var > 0).all(), scope
    mean = e.tap("conv0/gn_mean").reshape(1, 32); var = e.tap("conv0/gn_var").reshape(1, 32)
    assert np.abs(mean - mean64).max() <= 2e-5 * np.abs(mean64).max() and np.abs(var - var64).max() <= 2e-5 * var64.max()

  R.run_single(lib, cfg, 96, 128, check=check)


def test_gn_forward_multi_small(backend):
  """b = 2 with statistics per image; each image is bit-identical at either position of the batch."""
  name, lib = backend
  cfg = _cfg(im_batch_size=2, rpn_test_post_nms_topk=48)
  R.run_multi(lib, cfg, 2, 96, 128, check=check_batch_swap(["c2", "c3", "c4", "c5", "p2", "p5"]))


def test_gn_forward_without_dilations(backend):
  name, lib = backend
  R.run_single(lib, _cfg(use_dilations=False), 96, 128)


def test_gn_forward_identity_and_dilated_blocks(backend):
  """[1, 1, 2, 3]: identity blocks (the block's input is the apply kernel's plain residual) and three dilated blocks in group 3."""
  name, lib = backend
  cfg = _cfg(resnet_num_block=[1, 1, 2, 3])

  def check(m, e, d0, d, out, fr, ref):
    assert d["group_norms"] == 3 * 7 + 4 + 1 + 8, d

  R.run_single(lib, cfg, 96, 128, check=check)


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_gn_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test.  "auto" ends on
  fp16x2 with a healthy guard -- which the convs behind a GroupNorm can only where the apply kernel recorded its output's range."""
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
      assert d["fp16x2_split_launches"] > 0, d

  R.run_single(lib, cfg, 96, 128, check=check)


def test_gn_two_forwards_bit_identical(backend):
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


def test_gn_unsupported_combinations(emu_lib):
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  for kw, what in ((dict(use_se=True), "use_se"), (dict(use_resnext=True), "use_resnext"), (dict(use_basic_block=True), "use_basic_block"),
                   (dict(use_deformable=True, use_dilations=False), "use_deformable")):
    with pytest.raises(NotImplementedError, match="use_gn together with " + what):
      models.get_model(_cfg(**kw), 0, weights=w, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="use_conv_frcnn_head"):      # the GroupNorm 4-conv head is the follow-up
    models.get_model(_cfg(use_conv_frcnn_head=True), 0, weights=w, lib=emu_lib)
  less = {k: v for k, v in w.items() if k != "group1/block0/conv2/gn/gamma"}
  with pytest.raises(NotImplementedError, match="group1/block0/conv2/gn/gamma"):
    models.get_model(cfg, 0, weights=less, lib=emu_lib)


def test_gn_synthetic_weights_leave_the_rest_alone():
  """Every other variable of a seed is bit for bit what a config without the flag draws; the bn variables of the normalised
  layers are absent; conv3/gn/gamma carries the 0.25."""
  cfg = _cfg(resnet_num_block=[1, 1, 2, 3])
  w = synthetic_weights(cfg, 0)
  base = synthetic_weights(_cfg(resnet_num_block=[1, 1, 2, 3], use_gn=False), 0)
  gn = set(group_norm_variables(cfg))
  assert len(gn) == 2 * (3 * 7 + 4 + 1 + 8) and gn <= set(w)
  assert not [k for k in w if "/bn/" in k]
  for k, v in w.items():
    if k not in gn:
      assert np.array_equal(v, base[k]), k
  assert set(base) - set(w) == {k for k in base if "/bn/" in k} and set(w) - set(base) == gn
  assert w["conv0/gn/gamma"].shape == (64,) and w["fpn/gn_p5/beta"].shape == (256,) and w["group3/block2/conv3/gn/gamma"].shape == (2048,)
  assert 0.9 * 0.25 <= w["group0/block0/conv3/gn/gamma"].min() and w["group0/block0/conv3/gn/gamma"].max() <= 1.1 * 0.25
  assert 0.9 <= w["group0/block0/conv2/gn/gamma"].min() and w["group0/block0/conv2/gn/gamma"].max() <= 1.1


def test_gn_weights_survive_the_writers(tmp_path):
  """gn/{gamma,beta} and fpn/gn_* come back from every writer / reader pair of the repository (.npz, TF checkpoint, frozen .pb),
  and config_from_weights reads use_gn off the tensors."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  np.savez(str(tmp_path / "g.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-3"), w)
  write_frozen_pb(str(tmp_path / "g.pb"), w)
  for got in (load_npz(str(tmp_path / "g.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "g.pb"))):
    assert set(got) >= set(w)
    for k in group_norm_variables(cfg):
      assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "g.pb")))
  assert c.use_gn and list(c.resnet_num_block) == [1, 1, 1, 1]
  assert not models.config_from_weights(synthetic_weights(_cfg(use_gn=False), 0)).use_gn


# ------------------------------------------------------------------------------------------------- op level

def _affine(C, rng):
  return rng.uniform(0.5, 1.5, C).astype(F), (rng.standard_normal(C) * 0.5).astype(F)


def _check64(out, amax, mean, var, x, gamma, beta, res=None, upsample=False, relu=False, what=""):
  """|out - ref64| <= 16 u (|x| |a| + |mean| |a| + |beta|) with a, mean from float64: three terms, at most 8 roundings each
  (var, + eps, sqrt, the division, times gamma in a; the product; the subtraction; the final add), doubled.  A residual adds one
  more rounding of a sum that holds |res| as well: + 2 u |res|.  mean within 2 u mean|x|; var within 8 u var64 + 2^-40 E[x^2];
  the recorded |max| is max |out| bit for bit."""
  ref, mean64, var64, a64, ex2, mabs = R.group_norm64(x, gamma, beta, res, upsample, relu)
  B, h, w, C = x.shape
  gs = C // 32
  mean_c = np.repeat(mean64, gs, axis=1)
  bound = 16 * U * (np.abs(x.astype(np.float64)) * np.abs(a64)[:, None, None, :] + (np.abs(mean_c) * np.abs(a64))[:, None, None, :] +
                    np.abs(beta.astype(np.float64)))
  if res is not None:
    r = np.abs(res.astype(np.float64))
    bound = bound + 2 * U * (r.repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w] if upsample else r)
  e_out = float((np.abs(out.astype(np.float64) - ref) / bound).max())
  e_mean = float((np.abs(mean.astype(np.float64) - mean64) / (2 * U * mabs)).max())
  e_var = float((np.abs(var.astype(np.float64) - var64) / (8 * U * var64 + 2.0 ** -40 * ex2)).max())
  print("group_norm %s C=%d %dx%d: out err / bound = %.4f, mean %.4f, var %.4f" % (what, C, h, w, e_out, e_mean, e_var))
  assert out.dtype == F and out.shape == x.shape and mean.shape == (B, 32) and var.shape == (B, 32)
  assert e_out <= 1.0 and e_mean <= 1.0 and e_var <= 1.0, (what, C, h, w, e_out, e_mean, e_var)
  assert np.float32(amax) == np.abs(out).max() and amax > 0, (what, amax)
  return e_var


# B = 2.  1 x 1: two values per group; 5 x 7 / 9 x 13: odd maps, rows shorter than the pixel threads of a workgroup; 61 x 67:
# sixteen row ranges (the launcher's choice) and rows longer than one pass of the unrolled loops; 2048 channels: two workgroups
# side by side over the channels of a pixel, 64 channels per group
SHAPES = [(64, 1, 1), (64, 5, 7), (64, 61, 67), (128, 9, 13), (256, 8, 12), (2048, 3, 5)]


@pytest.mark.parametrize("C,h,w", SHAPES)
def test_group_norm_against_float64(backend, C, h, w):
  """Every variant of the op against a float64 evaluation (bounds: _check64): ReLU on and off, a plain residual, a 2x-upsampled
  residual (8 x 12 from 4 x 6), chunks 1 / 2 / 5 on 9 x 13; a second run is bit-identical."""
  name, lib = backend
  rng = np.random.default_rng(C + 10 * h + w)
  x = (rng.standard_normal((2, h, w, C)) * rng.uniform(0.5, 2.0, (2, 1, 1, C)) + rng.standard_normal((2, 1, 1, C))).astype(F)
  gamma, beta = _affine(C, rng)
  res = rng.standard_normal((2, h, w, C)).astype(F)
  for relu in (False, True):
    out, amax, mean, var = ops.group_norm(x, gamma, beta, relu=relu, lib=lib)
    _check64(out, amax, mean, var, x, gamma, beta, relu=relu, what="relu=%d" % relu)
    assert relu or out.min() < 0
    out2, amax2, mean2, var2 = ops.group_norm(x, gamma, beta, relu=relu, lib=lib)
    assert np.array_equal(out, out2) and amax == amax2 and np.array_equal(mean, mean2) and np.array_equal(var, var2)
    outr, amaxr, meanr, varr = ops.group_norm(x, gamma, beta, relu=relu, res=res, lib=lib)
    _check64(outr, amaxr, meanr, varr, x, gamma, beta, res=res, relu=relu, what="res relu=%d" % relu)
    assert np.array_equal(mean, meanr) and np.array_equal(var, varr)
  if (h, w) == (8, 12):
    up = rng.standard_normal((2, 4, 6, C)).astype(F)
    for relu in (False, True):
      out, amax, mean, var = ops.group_norm(x, gamma, beta, relu=relu, res=up, upsample=True, lib=lib)
      _check64(out, amax, mean, var, x, gamma, beta, res=up, upsample=True, relu=relu, what="upsampled res relu=%d" % relu)
  if (h, w) == (9, 13):
    for chunks in (1, 2, 5):
      out, amax, mean, var = ops.group_norm(x, gamma, beta, chunks=chunks, lib=lib)
      _check64(out, amax, mean, var, x, gamma, beta, what="chunks=%d" % chunks)


def test_group_norm_large_mean(backend):
  """x = 1000 + N(0, 1), C = 64, 61 x 67: |mean| / std ~ 1000.  The bounds of _check64 hold.  A condition on the input, checked
  here: numpy's f32 E[x^2] - mean^2 on the same data violates the var bound, so the input tells an f32 version of the kernel's
  formula from the f64 one."""
  name, lib = backend
  rng = np.random.default_rng(5)
  x = (1000.0 + rng.standard_normal((2, 61, 67, 64))).astype(F)
  gamma, beta = _affine(64, rng)
  out, amax, mean, var = ops.group_norm(x, gamma, beta, lib=lib)
  _check64(out, amax, mean, var, x, gamma, beta, what="large mean")
  _, mean64, var64, _, ex2, _ = R.group_norm64(x, gamma, beta)
  xg = x.reshape(2, 61 * 67, 32, 2)
  m32 = xg.mean(axis=(1, 3), dtype=F)
  v32 = (xg * xg).mean(axis=(1, 3), dtype=F) - m32 * m32
  assert v32.dtype == F
  assert (np.abs(v32.astype(np.float64) - var64) > 8 * U * var64 + 2.0 ** -40 * ex2).all()


def test_group_norm_constant_groups(backend):
  """1 x 1 with two channels per group and the same value in both: var = 0 exactly, mean = the value, and the output is exactly
  beta.  (x a and mean a are the same f32 product p; beta - p and p + (beta - p) are exact for the values chosen here -- gamma
  1 or 2, beta a multiple of 1/4, p away from a power of two -- which the test checks in numpy as a condition on its input.)"""
  name, lib = backend
  rng = np.random.default_rng(6)
  k = rng.integers(1, 5, (2, 32)).astype(F)
  x = np.repeat(k, 2, axis=1).reshape(2, 1, 1, 64)
  gamma = rng.integers(1, 3, 64).astype(F)
  beta = (rng.integers(-3, 4, 64) / 4.0).astype(F)
  a = (F(1) / np.sqrt(F(0) + F(1e-5))) * gamma
  p = x.reshape(2, 64) * a
  assert a.dtype == F and p.dtype == F and np.array_equal(p + (beta - p), np.broadcast_to(beta, (2, 64)))
  out, amax, mean, var = ops.group_norm(x, gamma, beta, lib=lib)
  assert np.array_equal(var, np.zeros((2, 32), F)) and np.array_equal(mean, k)
  assert np.array_equal(out.reshape(2, 64), np.broadcast_to(beta, (2, 64)))
  assert np.float32(amax) == np.abs(beta).max()


def _exact_case(C, h, w, seed):
  """Integer data with x in {m - 1, m + 1} in equal numbers per (image, group), a different m for each; a different gamma and
  beta for each channel: mean = m and var = 1 exactly, so out is the f32 expression evaluated in numpy."""
  rng = np.random.default_rng(seed)
  gs = C // 32
  n = h * w * gs
  assert n % 2 == 0
  m = (rng.permutation(64).reshape(2, 32) - 32).astype(F)
  sign = np.stack([rng.permutation(np.repeat([-1.0, 1.0], n // 2)) for _ in range(64)]).reshape(2, 32, h, w, gs)
  x = (m[:, :, None, None, None] + sign).transpose(0, 2, 3, 1, 4).reshape(2, h, w, C).astype(F)
  gamma = (0.5 + np.arange(C) / C).astype(F)
  beta = (np.arange(C)[::-1] / 8.0 - C / 16.0).astype(F)
  a = (F(1) / np.sqrt(F(1) + F(1e-5))) * gamma                       # [C], f32
  mc = np.repeat(m, gs, axis=1)                                      # [2, C]
  s = beta[None] - mc * a[None]
  y = x * a + s[:, None, None, :]
  assert y.dtype == F
  return x, gamma, beta, m, y, rng


@pytest.mark.parametrize("C,h,w", [(64, 5, 7), (128, 9, 13), (256, 8, 12), (2048, 3, 4)])
def test_group_norm_exact_on_integer_data(backend, C, h, w):
  """array_equal: a group / channel mix-up, a swapped image, a wrong upsample index or a residual read at the wrong pitch cannot
  hide in a tolerance."""
  name, lib = backend
  x, gamma, beta, m, y, rng = _exact_case(C, h, w, 7 * C + h)
  out, amax, mean, var = ops.group_norm(x, gamma, beta, lib=lib)
  assert np.array_equal(mean, m) and np.array_equal(var, np.ones((2, 32), F))
  assert np.array_equal(out, y) and np.float32(amax) == np.abs(y).max()
  res = rng.integers(-64, 65, (2, h, w, C)).astype(F)
  out, amax, _, _ = ops.group_norm(x, gamma, beta, relu=True, res=res, lib=lib)
  want = np.maximum(y + res, F(0))
  assert np.array_equal(out, want) and np.float32(amax) == want.max()
  if h % 2 == 0 and w % 2 == 0:
    up = rng.integers(-64, 65, (2, h // 2, w // 2, C)).astype(F)
    out, amax, _, _ = ops.group_norm(x, gamma, beta, res=up, upsample=True, lib=lib)
    want = y + up.repeat(2, axis=1).repeat(2, axis=2)
    assert np.array_equal(out, want) and np.float32(amax) == np.abs(want).max()


@pytest.mark.parametrize("C,Ha,Wa,ldc", [(128, 9, 13, 128), (128, 7, 16, 192), (256, 10, 14, 260), (512, 7, 13, 516)])
def test_group_norm_reads_a_pitched_view(backend, C, Ha, Wa, ldc):
  """A [2,7,13,C] view inside a [2,Ha,Wa,ldc] allocation (the tuples of test_deform_conv_reads_a_pitched_view) whose every
  element outside the view is NaN gives the dense tensor's output, statistics and recorded |max| bit for bit, and writes
  nothing outside the view."""
  name, lib = backend
  H, W = 7, 13
  rng = np.random.default_rng(3 * C + ldc)
  x = rng.standard_normal((2, H, W, C)).astype(F)
  gamma, beta = _affine(C, rng)
  res = rng.standard_normal((2, H, W, C)).astype(F)
  big = np.full((2, Ha, Wa, ldc), np.nan, F)
  big[:, :H, :W, :C] = x
  out, amax, mean, var = ops.group_norm(x, gamma, beta, relu=True, res=res, lib=lib)
  outv, amaxv, meanv, varv = ops.group_norm(big, gamma, beta, relu=True, res=res, view=(H, W, C), lib=lib)
  assert np.isfinite(outv).all()
  assert np.array_equal(outv[:, :H, :W, :C], out) and amax == amaxv and np.array_equal(mean, meanv) and np.array_equal(var, varv)
  outside = outv.copy(); outside[:, :H, :W, :C] = 0
  assert not outside.any()


def test_group_norm_interior_of_a_zero_bordered_tensor(backend):
  """The dilated stage entry: the interior at offset (1, 1) of a tensor whose first row and column are zero.  The border stays
  exactly zero (a ReLU-less beta would show there), the interior is the dense run bit for bit, the statistics ignore the border."""
  name, lib = backend
  rng = np.random.default_rng(9)
  for C, h, w in ((512, 2, 3), (64, 5, 7)):
    x = (rng.standard_normal((2, h, w, C)) + 0.5).astype(F)
    gamma, beta = _affine(C, rng)
    big = np.zeros((2, h + 1, w + 1, C), F)
    big[:, 1:, 1:] = x
    out, amax, mean, var = ops.group_norm(x, gamma, beta, lib=lib)
    outb, amaxb, meanb, varb = ops.group_norm(big, gamma, beta, view=(h, w, C), offset=(1, 1), lib=lib)
    assert not outb[:, 0].any() and not outb[:, :, 0].any()
    assert np.array_equal(outb[:, 1:, 1:], out) and amax == amaxb and np.array_equal(mean, meanb) and np.array_equal(var, varb)


def test_group_norm_rejects_bad_arguments(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  z = lambda *s: np.zeros(s, F)
  with pytest.raises(OdtError, match="multiple of 32"):
    ops.group_norm(z(1, 4, 4, 48), z(48), z(48), lib=emu_lib)
  with pytest.raises(OdtError, match="outside its allocation"):      # a view taller than its allocation
    ops.group_norm(z(1, 4, 4, 64), z(64), z(64), view=(5, 4, 64), lib=emu_lib)
  with pytest.raises(OdtError, match="outside its allocation"):      # ... or pushed past it by the offset
    ops.group_norm(z(1, 4, 4, 64), z(64), z(64), view=(4, 4, 64), offset=(1, 0), lib=emu_lib)
  with pytest.raises(OdtError, match="multiple of 4"):               # a channel pitch that breaks the 16-byte loads
    ops.group_norm(z(1, 4, 4, 66), z(64), z(64), view=(4, 4, 64), lib=emu_lib)
  with pytest.raises(OdtError, match="chunks"):
    ops.group_norm(z(1, 4, 4, 64), z(64), z(64), chunks=5, lib=emu_lib)
  with pytest.raises(OdtError, match="residual is smaller"):
    ops.group_norm(z(1, 4, 4, 64), z(64), z(64), res=z(1, 1, 2, 64), upsample=True, lib=emu_lib)
