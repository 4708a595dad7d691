"""Model version 6: the Squeeze-Excitation ResNet backbone (reference nn.py:506-517, obj_detect_tracking.py --version 6).

End to end against the oracle running the LITERAL SE bottleneck (se_reference.se_bottleneck: the mean of conv3's output),
while the product pools conv2's output and folds conv3 + BN into fc1; the surface (config, loaders, eager weight check);
and the new kernels one by one (csrc/resnet_se.hip) in the style of test_effdet_ops.py.

Tolerances are the project's own (test_e2e.py): trunk 2e-5 of the tensor maximum, boxes 1e-3 px, scores 1e-4, appearance
features 10x the trunk tolerance, mismatch budget 0."""
import copy

import numpy as np
import pytest
import torch

from common import assert_same_detections, make_config, match_detections, small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights
from oracle.graph import OracleModel
from se_reference import se_oracle
from test_e2e import _check_trunk, _rel, _with_taps

F = np.float32
U = 2.0 ** -24           # unit roundoff of f32
_W = {}


def _weights(cfg, seed=0):
  """common.weights_for does not key on use_se: the SE tests draw their own."""
  key = (tuple(cfg.resnet_num_block), cfg.num_class, seed, bool(cfg.use_frcnn_class_agnostic), bool(cfg.use_se))
  if key not in _W:
    _W[key] = synthetic_weights(cfg, seed)
  return _W[key]


def _oracle(cfg, w):
  return OracleModel(cfg, w)


def _run_single(lib, cfg, H, W, tol=2e-5, w=None, check=None):
  """test_e2e._run_single for an SE graph: the production handle against the keep_taps handle bit for bit, trunk taps,
  proposals and detections pair by pair against the literal-SE oracle; mismatch budget 0."""
  w = _weights(cfg) if w is None else w
  fr = synthetic_frames(1, H, W)
  with se_oracle():
    ref = _oracle(cfg, w).forward(fr[0])
  m0 = models.get_model(cfg, 0, weights=w, lib=lib)
  try:
    prod = m0.predict(fr[0])
    d0 = m0.engine(1, H, W).describe()
    assert d0["memory"]["keep_taps"] == 0
    with pytest.raises(Exception, match="keep_taps"):
      m0.engine(1, H, W).tap("c3")
  finally:
    m0.close()
  m = models.get_model(_with_taps(cfg), 0, weights=w, lib=lib)
  try:
    boxes, labels, probs, feats = m.predict(fr[0])
    for a, b in zip(prod, (boxes, labels, probs, feats)):
      assert np.array_equal(a, b), "arena and keep_taps handles disagree"
    e = m.engine(1, H, W)
    _check_trunk(e, ref, tol)
    for g in [g for g in range(4) if cfg.resnet_num_block[g] > 1]:      # (a group's last block is tapped as c2 ... c5)
      name = "group%d/block0" % g
      assert _rel(e.tap(name).transpose(0, 3, 1, 2), ref[name]) < tol, name
    assert feats.shape == (boxes.shape[0], 256, 7, 7)
    n = int(e.tap("nproposals")[0])
    assert n == ref["proposals"].shape[0] and n > 0
    pm, rm = match_detections(e.tap("proposals")[0, 0, :n], np.zeros(n), np.zeros(n), ref["proposals"], np.zeros(n),
                              np.zeros(n), 1e-3, 1)
    assert pm + rm == 0, "proposal sets differ: %d/%d of %d" % (pm, rm, n)
    miss, extra = match_detections(boxes, labels, probs, ref["final_boxes"], ref["final_labels"], ref["final_probs"],
                                   1e-3, 1e-4)
    assert miss + extra == 0 and len(boxes) > 0, (miss, extra, len(boxes))
    assert_same_detections(boxes, labels, probs, feats, ref["final_boxes"], ref["final_labels"], ref["final_probs"],
                           ref["fpn_box_feat"], 1e-3, 1e-4, 10 * tol)
    d = e.describe()
    assert d["use_se"] == 1 and d["se_blocks"] == sum(cfg.resnet_num_block) and d0["use_se"] == 1, d
    assert d["bottleneck_tails_fused"] == 0, d
    if check is not None:
      check(m, e, d0, d, (boxes, labels, probs, feats), fr)
  finally:
    m.close()


def _run_multi(lib, cfg, B, H, W, tol=2e-5, check=None):
  """test_e2e._run_multi for an SE graph."""
  w = _weights(cfg)
  fr = synthetic_frames(B, H, W)
  with se_oracle():
    ref = _oracle(cfg, w).forward_multi(fr)
  m0 = models.get_model(cfg, 0, weights=w, lib=lib, is_multi=True)
  try:
    prod = m0.predict_batch(fr)
    d0 = m0.engine(B, H, W).describe()
  finally:
    m0.close()
  m = models.get_model(_with_taps(cfg), 0, weights=w, lib=lib, is_multi=True)
  try:
    boxes, labels, probs, valid, feats = m.predict_batch(fr)
    for a, b in zip(prod, (boxes, labels, probs, valid, feats)):
      assert np.array_equal(a, b), "arena and keep_taps handles disagree"
    e = m.engine(B, H, W)
    _check_trunk(e, ref, tol)
    assert labels.dtype == np.float32 and valid.dtype == np.int32
    assert boxes.shape == (B, cfg.result_per_im, 4)
    assert np.array_equal(valid, ref["final_valid_indices"]) and valid.min() > 0
    assert feats.shape[0] == valid.sum()
    off = 0
    for b in range(B):
      v = int(valid[b])
      miss, extra = match_detections(boxes[b, :v], labels[b, :v], probs[b, :v], ref["final_boxes"][b, :v],
                                     ref["final_labels"][b, :v], ref["final_probs"][b, :v], 1e-3, 1e-4)
      assert miss + extra == 0, (b, miss, extra)
      assert_same_detections(boxes[b, :v], labels[b, :v], probs[b, :v], feats[off:off + v], ref["final_boxes"][b, :v],
                             ref["final_labels"][b, :v], ref["final_probs"][b, :v], ref["fpn_box_feat"][off:off + v],
                             1e-3, 1e-4, 10 * tol)
      off += v
    d = e.describe()
    assert d["use_se"] == 1 and d["se_blocks"] == sum(cfg.resnet_num_block), d
    if check is not None:
      check(m, e, d0, d, (boxes, labels, probs, valid, feats), fr)
  finally:
    m.close()


# ------------------------------------------------------------------------------------------------- end to end

def test_se_forward_single_small(backend):
  """Fails on a tree without the feature: get_model raises NotImplementedError for use_se."""
  name, lib = backend
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1])
  assert cfg.use_se and cfg.use_frcnn_class_agnostic and not cfg.use_dilations
  _run_single(lib, cfg, 96, 128)


def test_se_forward_multi_small_and_batch_independence(backend):
  """The multi graph, and the gate's batch independence: each image's trunk taps, gates and detections are bit-identical
  to the same frame at the other position of a batch of the same two frames."""
  name, lib = backend
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1], im_batch_size=2, rpn_test_post_nms_topk=48)
  taps = ["c2", "c3", "c4", "c5", "group0/block0/se_gate", "group3/block0/se_gate"]

  def check(m, e, d0, d, out, fr):
    a = {t: e.tap(t) for t in taps}
    boxes, labels, probs, valid, feats = out
    sb, sl, sp, sv, sf = m.predict_batch(fr[::-1].copy())
    for t in taps:
      x, y = a[t], e.tap(t)
      if t.endswith("se_gate"):      # [1, 1, B, C]
        assert x[0, 0, 0].min() > 0 and not np.array_equal(x[0, 0, 0], x[0, 0, 1]), t
        assert np.array_equal(x[0, 0, 0], y[0, 0, 1]) and np.array_equal(x[0, 0, 1], y[0, 0, 0]), t
      else:
        assert np.array_equal(x[0], y[1]) and np.array_equal(x[1], y[0]), t
    assert np.array_equal(valid, sv[::-1])
    for b in range(2):
      assert np.array_equal(boxes[b], sb[1 - b]) and np.array_equal(probs[b], sp[1 - b]) and np.array_equal(labels[b], sl[1 - b])
    v0 = int(valid[0])
    assert np.array_equal(feats[:v0], sf[int(valid[1]):]) and np.array_equal(feats[v0:], sf[:int(valid[1])])

  _run_multi(lib, cfg, 2, 96, 128, check=check)


def test_se_two_forwards_bit_identical(backend):
  name, lib = backend
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1])
  fr = synthetic_frames(1, 96, 128)
  m = models.get_model(cfg, 0, weights=_weights(cfg), lib=lib)
  try:
    a = m.predict(fr[0]); b = m.predict(fr[0])
    assert len(a[0]) > 0
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  finally:
    m.close()


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_se_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test; "auto" builds
  the guard's bf16x3 twin (an SE plan as well) and reports a healthy guard."""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1], **kw)

  def check(m, e, d0, d, out, fr):
    if mode == "f32":
      assert d["conv_arith"] == "exact f32 MFMA" and d["fp16x2_split_launches"] == 0, d
    elif mode == "split3":
      assert d["fp16x2_split_launches"] == 0 and d["policy"]["family"] == 3, d
    else:
      auto = d["conv_split_family_auto"]
      assert "auto" in d["range_guard"] and auto["chosen"].startswith("fp16x2"), d
      assert len(auto["checks"]) == 1 and auto["calibration_forwards_left"] == 0 and not auto["incomplete"], auto
      assert auto["checks"][0]["max_rel_diff"] <= auto["tolerance"], auto

  _run_single(lib, cfg, 96, 128, check=check)


def test_se_unit_gate_matches_the_ungated_graph(backend):
  """fc2/W = 0, fc2/b = 30: sigmoid(30) rounds to exactly 1.0f, so the SE plan computes the plain ResNet -- through its own
  ops (separate convshortcut, conv3 without epilogue, apply).  Its trunk taps equal those of the same weights run with
  use_se=False, undilated, within the trunk tolerance (not bit for bit: the stage entries sum in another order)."""
  name, lib = backend
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1], keep_taps=True)
  w = dict(_weights(cfg))
  for k in list(w):
    if k.endswith("/fc2/W"):
      w[k] = np.zeros_like(w[k])
    if k.endswith("/fc2/b"):
      w[k] = np.full_like(w[k], 30.0)
  cfg0 = small_config(version=2, use_dilations=False, use_frcnn_class_agnostic=True, resnet_num_block=[1, 1, 1, 1], keep_taps=True)
  assert not cfg0.use_se and cfg0.use_frcnn_class_agnostic and not cfg0.use_dilations
  fr = synthetic_frames(1, 96, 128)
  names = ["c2", "c3", "c4", "c5", "p2", "p3", "p4", "p5", "p6", "rpn2", "rpn6"]
  got = []
  for c in (cfg, cfg0):
    m = models.get_model(c, 0, weights=w, lib=lib)
    try:
      m.predict(fr[0])
      e = m.engine(1, 96, 128)
      got.append({n: e.tap(n) for n in names})
      if c is cfg:
        for g in range(4):
          gate = e.tap("group%d/block0/se_gate" % g)
          assert np.array_equal(gate, np.ones_like(gate)), "sigmoid(30) must be exactly 1.0f"
    finally:
      m.close()
  for n in names:
    assert _rel(got[0][n], got[1][n]) < 2e-5, n
  # and with the drawn weights the gate matters: c5 moves by far more than any tolerance here
  m = models.get_model(cfg, 0, weights=_weights(cfg), lib=lib)
  try:
    m.predict(fr[0])
    c5 = m.engine(1, 96, 128).tap("c5")
  finally:
    m.close()
  assert _rel(c5, got[1]["c5"]) > 1e-2


# ------------------------------------------------------------------------------------------------- surface

def test_se_config_versions():
  from object_detection_tracking_amd.config import make_config as mk
  c6 = mk(version=6)
  assert c6.use_dilations is False and c6.use_se is True and c6.use_frcnn_class_agnostic is True
  assert mk(version=6, use_dilations=True).use_dilations is True
  # versions 2-5: what they produced before version 6 existed here
  want = {2: (True, False, False), 3: (True, False, False), 4: (True, True, False), 5: (True, True, False)}
  for v, (dil, agn, se) in want.items():
    c = mk(version=v)
    assert (c.use_dilations, c.use_frcnn_class_agnostic, c.use_se) == (dil, agn, se), v
  assert mk().version == 3 and mk().use_dilations is True
  assert mk(version=2, use_dilations=False).use_dilations is False


def test_se_synthetic_weights_leave_the_rest_untouched():
  cfg = small_config(version=6, resnet_num_block=[1, 2, 1, 1])
  w = synthetic_weights(cfg, 3)
  cfg0 = copy.copy(cfg); cfg0.use_se = False
  w0 = synthetic_weights(cfg0, 3)
  assert all(np.array_equal(w[k], w0[k]) for k in w0) and not any("/fc" in k and k.startswith("group") for k in w0)
  se = sorted(set(w) - set(w0))
  assert len(se) == 4 * 5 and w["group1/block1/fc1/W"].shape == (512, 32) and w["group1/block1/fc2/W"].shape == (32, 512)
  assert w["group3/block0/fc1/b"].shape == (128,) and w["group3/block0/fc2/b"].shape == (2048,)
  assert all(w[k].dtype == np.float32 for k in se)
  # the recipe: a generator of its own, groups and blocks in order, fc1/W, fc1/b, fc2/W, fc2/b per block
  rng = np.random.default_rng([3, 6])
  first = rng.standard_normal((256, 16), dtype=np.float32) * np.float32(np.sqrt(2.0 / 256))
  assert np.array_equal(w["group0/block0/fc1/W"], first)


def test_se_loaders_round_trip_and_detection(tmp_path, backend):
  """An SE weight set through every writer / reader pair of the repository (.npz, TF checkpoint, frozen .pb);
  config_from_weights reads use_se (and, with it, no dilations) off the tensors; weights without the SE variables cannot
  construct an SE model."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz
  name, lib = backend
  cfg = small_config(version=6, resnet_num_block=[1, 1, 1, 1])
  w = _weights(cfg)
  np.savez(str(tmp_path / "se.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-6"), w)
  write_frozen_pb(str(tmp_path / "se.pb"), w)
  for got in (load_npz(str(tmp_path / "se.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "se.pb"))):
    assert set(got) >= set(w)
    for k in w:
      assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "se.pb")))
  assert c.use_se and not c.use_dilations and c.use_frcnn_class_agnostic and list(c.resnet_num_block) == [1, 1, 1, 1]
  assert models.config_from_weights(w, use_dilations=True).use_dilations
  w5 = synthetic_weights(small_config(version=5, resnet_num_block=[1, 1, 1, 1]), 0)
  c5 = models.config_from_weights(w5)
  assert not c5.use_se and c5.use_dilations
  with pytest.raises(NotImplementedError, match="squeeze-excitation variables: missing group0/block0/fc1/W"):
    models.get_model(cfg, 0, weights=w5, lib=lib)
  bad = dict(w); bad["group2/block0/fc2/W"] = np.zeros((64, 1000), np.float32)
  with pytest.raises(NotImplementedError, match="group2/block0/fc2/W"):
    models.get_model(cfg, 0, weights=bad, lib=lib)
  # the frozen route end to end: the file alone says it is an SE model
  m = models.Mask_RCNN_FPN_frozen(str(tmp_path / "se.pb"), 0, lib=lib)
  try:
    assert m.config.use_se and not m.config.use_dilations
  finally:
    m.close()


# ------------------------------------------------------------------------------------------------- op level

def _ints(rng, shape, lo=-8, hi=9):
  return rng.integers(lo, hi, shape).astype(F)


@pytest.mark.parametrize("B,HW,C,ldc", [
    (2, 37, 64, 64),        # whole quads, less than one workgroup per image
    (1, 301, 256, 256),     # stride a multiple of the quads per pixel: the register-gate walk, with an odd tail pass
    (3, 50, 10, 12),        # partial 16-byte group, pad channels
    (2, 129, 7, 8),         # one partial quad in two, partial workgroup
    (1, 1031, 28, 28),      # 7 quads per pixel: a grid rounded to whole pixels per stride
    (2, 700, 2048, 2048),   # 512 quads per pixel (res5)
])
@pytest.mark.parametrize("in_place", [False, True])
def test_rse_apply_bit_exact(backend, B, HW, C, ldc, in_place):
  """out = max(y * g + s, 0): bit-equal to the same three f32 numpy operations; the recorded |max| is out.max() exactly;
  pad channels [C, ldc) -- NaN in y, the shortcut and the gate -- are neither written nor counted."""
  name, lib = backend
  if name == "emu" and HW * ldc > 400000:
    HW = 150
  rng = np.random.default_rng(HW * 7 + C)
  y = rng.standard_normal((B, HW, ldc)).astype(F) * F(3)
  s = rng.standard_normal((B, HW, ldc)).astype(F)
  g = rng.uniform(0.05, 0.95, (B, ldc)).astype(F)
  y[..., C:] = np.nan; s[..., C:] = np.nan; g[..., C:] = np.nan
  init = np.full((B, HW, ldc), 77.0, F)
  out, amax = ops.rse_apply(y, g, s, C=C, in_place=in_place, out_init=init, lib=lib)
  ref = np.maximum(y[..., :C] * g[:, None, :C] + s[..., :C], F(0))
  assert ref.dtype == F
  assert np.array_equal(out[..., :C], ref)
  if in_place:
    assert np.isnan(out[..., C:]).all()            # y's own pad channels, untouched
  else:
    assert np.array_equal(out[..., C:], init[..., C:])
  assert amax == float(ref.max()) and amax > 0


def _gate_case(rng, B, HW, ch):
  r, cout = ch // 4, 4 * ch
  t2 = _ints(rng, (B, HW, ch), 0, 9)
  w3 = (rng.standard_normal((ch, cout)) * np.sqrt(2.0 / ch) * 0.12).astype(F)
  b3 = (rng.standard_normal(cout) * 0.05).astype(F)
  f1 = (rng.standard_normal((cout, r)) * np.sqrt(2.0 / cout)).astype(F)
  f1b = (rng.standard_normal(r) * 0.02).astype(F)
  f2 = (rng.standard_normal((r, cout)) * np.sqrt(2.0 / r)).astype(F)
  f2b = (rng.standard_normal(cout) * 0.5).astype(F)
  return t2, w3, b3, f1, f1b, f2, f2b


def _gate_ref(t2, w3, b3, f1, f1b, f2, f2b):
  """float64 of the LITERAL formula -- the mean over the pixels of conv3's output, then fc1 / ReLU / fc2 / sigmoid -- and a
  per-element bound for the device's f32 evaluation of the FOLDED form, from term counts (u = 2^-24):
    pre-ReLU a_j = sum_i m_i w1_ji + b1_j with w1 = w3 @ fc1/W rounded once (u |w1| <= u |w3| @ |fc1|), b1 likewise, the
    device mean rounded once (u), an f32 dot product of ch terms plus the bias ((ch + 1) u): (ch + 4) u (A_j + Bb_j),
    A = |m| @ |w3| @ |fc1|, Bb = |b3| @ |fc1| + |fc1/b|; ReLU is 1-Lipschitz;
    z_c: r terms plus the bias, (r + 1) u (|h| @ |fc2| + |b2|), plus the incoming error through |fc2|;
    sigmoid: Lipschitz 1/4, plus 4 ulp (2^-23 relative) for expf, the add and the division."""
  t2, w3, b3, f1, f1b, f2, f2b = (np.asarray(a, np.float64) for a in (t2, w3, b3, f1, f1b, f2, f2b))
  ch, r = w3.shape[0], f1.shape[1]
  l = t2 @ w3 + b3                           # conv3 (+ folded BN) at every pixel
  m4 = l.mean(axis=1)                        # GlobalAvgPooling of conv3's output
  h = np.maximum(m4 @ f1 + f1b, 0.0)
  z = h @ f2 + f2b
  g = 1.0 / (1.0 + np.exp(-z))
  m = np.abs(t2.mean(axis=1))
  err_a = 1.01 * (ch + 4) * U * (m @ np.abs(w3) @ np.abs(f1) + np.abs(b3) @ np.abs(f1) + np.abs(f1b))
  err_z = 1.01 * (r + 1) * U * (np.abs(h) @ np.abs(f2) + np.abs(f2b)) + err_a @ np.abs(f2)
  return g, 0.25 * err_z + 4 * 2.0 ** -23 * g


@pytest.mark.parametrize("B,HW,ch", [(2, 37, 64), (1, 1200, 128), (3, 500, 256), (2, 64, 512)])
def test_rse_pool_and_gate(backend, B, HW, ch):
  """Pool of t2 (integer values: exact against float64) and the gate against float64 of the literal formula."""
  name, lib = backend
  rng = np.random.default_rng(HW + ch)
  t2, w3, b3, f1, f1b, f2, f2b = _gate_case(rng, B, HW, ch)
  w1, b1 = ops.se_fold(w3, b3, f1, f1b)
  mean, gate = ops.rse_gate(t2, w1, b1, f2, f2b, lib=lib)
  sums = t2.astype(np.float64).sum(1)
  assert np.abs(sums).max() < 2 ** 24
  assert np.array_equal(mean, (sums.astype(F) / F(HW)).astype(F))
  g, tol = _gate_ref(t2, w3, b3, f1, f1b, f2, f2b)
  assert np.all(np.abs(gate - g) <= tol), float((np.abs(gate - g) / tol).max())
  assert gate.min() > 0.01 and gate.max() < 0.99 and gate.std() > 0.05      # a gate that matters
  # fixed summation orders: run to run bit-identical
  mean2, gate2 = ops.rse_gate(t2, w1, b1, f2, f2b, lib=lib)
  assert np.array_equal(mean, mean2) and np.array_equal(gate, gate2)


@pytest.mark.parametrize("kind,B,H,W,ch", [("stride1", 2, 12, 20, 64), ("entry", 1, 7, 9, 128)])
def test_se_tail_against_torch(backend, kind, B, H, W, ch):
  """ops.se_tail (pool, gate, conv3, apply as the plan runs them) against torch in float64: a stride-1 block (the shortcut is
  the block's input) and a stage entry (the shortcut is a stride-2 1x1 convshortcut of a [2H, 2W] input of half the
  width).  Bound per element: the conv at (K + 16) u sum|t2||w3| (an f32 dot product of K terms in any of the three conv
  arithmetics: csrc/conv_split_common.hpp bounds the split products' dropped terms by 12 u) times the gate, the gate's own
  bound times |y|, and three roundings of the apply step."""
  name, lib = backend
  rng = np.random.default_rng(ch + H)
  t2, w3, b3, f1, f1b, f2, f2b = _gate_case(rng, B, H * W, ch)
  t2 = t2.reshape(B, H, W, ch)
  C3 = 4 * ch
  if kind == "stride1":
    sc = rng.standard_normal((B, H, W, C3)).astype(F)
  else:
    x = torch.from_numpy(rng.standard_normal((B, C3 // 2, 2 * H, 2 * W)).astype(F))
    ws = torch.from_numpy((rng.standard_normal((C3, C3 // 2, 1, 1)) * np.sqrt(1.0 / (C3 // 2))).astype(F))
    sc = torch.nn.functional.conv2d(x[:, :, :-1, :-1], ws, stride=2).permute(0, 2, 3, 1).contiguous().numpy()
    assert sc.shape == (B, H, W, C3)
  out, gate, amax = ops.se_tail(t2, w3, b3, (f1, f1b), (f2, f2b), sc, lib=lib)
  td = torch.from_numpy(t2).double().permute(0, 3, 1, 2)
  y = torch.nn.functional.conv2d(td, torch.from_numpy(w3).double().t()[:, :, None, None], torch.from_numpy(b3).double())
  sq = y.mean(dim=(2, 3))
  sq = torch.relu(sq @ torch.from_numpy(f1).double() + torch.from_numpy(f1b).double())
  sq = torch.sigmoid(sq @ torch.from_numpy(f2).double() + torch.from_numpy(f2b).double())
  ref = torch.relu(y * sq[:, :, None, None] + torch.from_numpy(sc).double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
  yn = y.permute(0, 2, 3, 1).numpy()
  g, gtol = _gate_ref(t2.reshape(B, H * W, ch), w3, b3, f1, f1b, f2, f2b)
  assert np.allclose(g, sq.numpy(), rtol=0, atol=1e-12)
  assert np.all(np.abs(gate - g) <= gtol), float((np.abs(gate - g) / gtol).max())
  conv_err = (ch + 16) * U * (np.abs(t2.astype(np.float64)) @ np.abs(w3.astype(np.float64)) + np.abs(b3.astype(np.float64)))
  tol = conv_err * g[:, None, None, :] + np.abs(yn) * gtol[:, None, None, :] + 3 * U * (np.abs(yn) * g[:, None, None, :] + np.abs(sc))
  assert np.all(np.abs(out - ref) <= tol), float((np.abs(out - ref) / tol).max())
  assert amax == float(out.max()) and (out > 0).mean() > 0.2


def test_rse_launchers_reject_bad_sizes(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  with pytest.raises(OdtError, match="bad sizes"):
    ops.rse_apply(np.zeros((1, 4, 6), F), np.zeros((1, 6), F), np.zeros((1, 4, 6), F), lib=emu_lib)      # ldc % 4
  with pytest.raises(OdtError, match="LDS"):
    ops.rse_gate(np.zeros((1, 4, 4096), F), np.zeros((8, 4096), F), np.zeros(8, F), np.zeros((8, 16), F), np.zeros(16, F),
                 lib=emu_lib)


# ------------------------------------------------------------------------------------------------- R101 on the GPU

@pytest.mark.gpu
def test_se_forward_single_r101_256x448(hip_lib):
  cfg = make_config(version=6, rpn_test_post_nms_topk=300, max_size=448, short_edge_size=256)
  _run_single(hip_lib, cfg, 256, 448)


@pytest.mark.gpu
def test_se_forward_single_r101_1080p(hip_lib):
  cfg = make_config(version=6, rpn_test_post_nms_topk=300)
  _run_single(hip_lib, cfg, 1080, 1920)


@pytest.mark.gpu
def test_se_forward_multi_r101_b2_256x448(hip_lib):
  cfg = make_config(version=6, rpn_test_post_nms_topk=300, max_size=448, short_edge_size=256, im_batch_size=2)
  _run_multi(hip_lib, cfg, 2, 256, 448)


@pytest.mark.gpu
def test_se_forward_multi_r101_b8_1080p(hip_lib):
  """The benchmark's shape on the SE graph, with the checks of test_e2e.test_forward_multi_r101_b8_1080p; and every block's
  conv1 runs on the fp16x2 kernels, which it can only where the apply kernel recorded its input's range."""
  cfg = make_config(version=6, rpn_test_post_nms_topk=300, im_batch_size=8)

  def check(m, e, d0, d, out, fr):
    for dd in (d0, d):
      assert dd["se_blocks"] == 33 and dd["se_blocks_conv1_on_fp16x2"] == 33, dd
    names = [n for n, _, _, _ in e.profile_layers() if "/conv1" in n]
    assert len(names) == 33 and all(n.endswith("[fp16x2]") for n in names), names

  _run_multi(hip_lib, cfg, 8, 1080, 1920, tol=1e-5, check=check)
