"""Reference side of the --use_conv_frcnn_head tests: a literal torch restatement of the reference's 4conv1fc box head
(conv_frcnn_head, models.py:1110-1124: four times conv2d(kernel 3, 'SAME', ReLU) -- under use_gn each followed by group_norm,
behind the ReLU and with nothing behind it -- then dense + ReLU over the NCHW-flattened map; reached from fastrcnn_2fc_head /
fastrcnn_2fc_head_class_agnostic, whose output layers follow unchanged), a context manager that runs an OracleModel on that
head without editing oracle/ (oracle/graph.py calls box_head by module-level name; under use_gn it nests gn_reference.gn_oracle),
and the end-to-end comparisons of gn_reference.py restated with this feature's describe() and head-tap checks.  A helper
module, not a conftest: the tests import it by name."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import gn_reference as GR
import oracle.graph as G
from common import assert_same_detections, match_detections
from object_detection_tracking_amd import models
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights
from test_e2e import _check_trunk, _rel, _with_taps

_W = {}


def weights(cfg, seed=0):
  key = (tuple(cfg.resnet_num_block), cfg.num_class, seed, bool(cfg.use_gn), bool(cfg.use_conv_frcnn_head),
         int(cfg.conv_frcnn_head_dim), bool(getattr(cfg, "use_frcnn_class_agnostic", False)))
  if key not in _W:
    _W[key] = synthetic_weights(cfg, seed)
  return _W[key]


def conv_box_head(use_gn, rec=None):
  """The 4conv1fc head with the arguments of oracle.graph.box_head.  rec (a dict) receives the last conv layer's output
  "head_conv3" [R,D_c,7,7] and the hidden vector "head_fc" [R,head_dim] of the last call."""

  def box_head(roi_feat, weights, num_class, partial_ids=None, class_agnostic=False):
    with torch.no_grad():
      l = torch.from_numpy(np.ascontiguousarray(roi_feat))                # [R,C,7,7]
      for k in range(4):
        W = G._w(weights, "fastrcnn/conv%d/W" % k).permute(3, 2, 0, 1).contiguous()
        l = torch.relu(TF.conv2d(l, W, G._w(weights, "fastrcnn/conv%d/b" % k), padding=1))
        if use_gn:
          l = GR.group_norm(l, G._w(weights, "fastrcnn/gn%d/gamma" % k), G._w(weights, "fastrcnn/gn%d/beta" % k))
      h = torch.relu(l.reshape(l.shape[0], -1) @ G._w(weights, "fastrcnn/fc/W") + G._w(weights, "fastrcnn/fc/b"))
      cls = h @ G._w(weights, "fastrcnn/outputs/class/W") + G._w(weights, "fastrcnn/outputs/class/b")
      box = h @ G._w(weights, "fastrcnn/outputs/box/W") + G._w(weights, "fastrcnn/outputs/box/b")
      if class_agnostic:
        box = box.reshape(-1, 1, 4).repeat(1, num_class - 1, 1)
      else:
        box = box.reshape(-1, num_class, 4)[:, 1:, :]
    if rec is not None:
      rec["head_conv3"] = l.numpy(); rec["head_fc"] = h.numpy()
    cls, box = cls.numpy(), np.ascontiguousarray(box.numpy())
    if partial_ids is not None:
      ids = [int(i) for i in partial_ids]
      cls = np.ascontiguousarray(cls[:, [0] + ids])
      box = np.ascontiguousarray(box[:, [i - 1 for i in ids], :])
    return cls, box

  return box_head


@contextlib.contextmanager
def head_oracle(cfg):
  """While active, oracle.graph.box_head is the 4conv1fc head (and, under cfg.use_gn, the trunk is gn_oracle's).  Yields the
  dict the head records its taps in."""
  rec = {}
  saved = G.box_head
  G.box_head = conv_box_head(bool(cfg.use_gn), rec)
  try:
    with (GR.gn_oracle() if cfg.use_gn else contextlib.nullcontext()):
      yield rec
  finally:
    G.box_head = saved


def describe_ok(cfg, d):
  assert d["box_head"] == "4conv1fc", d
  assert d["use_gn"] == int(bool(cfg.use_gn)), d
  assert d["roi_group_norms"] == (4 if cfg.use_gn else 0), d
  # (the frame-level count does not move with the head)
  assert d["group_norms"] == (3 * sum(cfg.resnet_num_block) + 4 + 1 + 8 if cfg.use_gn else 0), d


def check_head_taps(e, cfg, w, tol, rec_e2e=None, rows=None):
  """head_conv3 [R,7,7,D_c] and head_fc [1,1,R,head_dim] of a keep_taps engine against the literal head evaluated on the engine's
  own RoI features (the "roi_feat" tap, every row of it: the zero RoIs past the proposal count too): tol of the tensor maximum.

  Why on the engine's own RoI features and not against the taps of the end-to-end oracle run: the two sides' proposals agree to
  the project's box tolerance (1e-3 px asserted; 5e-5 .. 2e-4 px measured on seeds 0 - 5), and ROIAlign turns a box that moved by
  d px into features that moved by d times the pyramid's gradient -- 7e-6 .. 1.5e-5 of the tensor maximum on those seeds, half
  the tolerance spent in front of the head.  The head, evaluated in float64 on both inputs, carries that to 1.5e-5 .. 6.3e-5 at
  head_conv3 under use_gn (a normalisation divides by a group's standard deviation), while this project's head is within 5e-6
  of float64 on the same input.  The end-to-end figures are printed (rec_e2e over `rows`); the detections are compared end to
  end by the callers."""
  roi = e.tap("roi_feat")
  R_ = roi.shape[2]
  roi = np.ascontiguousarray(roi.reshape(R_, 7, 7, -1).transpose(0, 3, 1, 2))
  rec = {}
  conv_box_head(bool(cfg.use_gn), rec)(roi, w, cfg.num_class, None, bool(getattr(cfg, "use_frcnn_class_agnostic", False)))
  c3 = e.tap("head_conv3").transpose(0, 3, 1, 2)
  fc = e.tap("head_fc").reshape(R_, -1)
  for name, got, ref in (("head_conv3", c3, rec["head_conv3"]), ("head_fc", fc, rec["head_fc"])):
    print("head tap %s: rel err %.3g (tolerance %.3g)" % (name, _rel(got, ref), tol))
    assert got.shape == ref.shape and np.isfinite(got).all() and _rel(got, ref) < tol, name
    if rec_e2e is not None:
      print("  ... against the end-to-end oracle's (not asserted): %.3g" % _rel(got[rows], rec_e2e[name]))


def run_single(lib, cfg, H, W, tol=2e-5, check=None, seed=0):
  """gn_reference.run_single against the 4conv1fc oracle: the production handle against the keep_taps handle bit for bit, trunk
  and head taps (check_head_taps) 2e-5 of the tensor maximum, proposals and detections pair by pair (boxes 1e-3 px, scores 1e-4,
  features 10x the trunk tolerance); mismatch budget 0."""
  w = weights(cfg, seed)
  fr = synthetic_frames(1, H, W)
  with head_oracle(cfg) as rec:
    ref = G.OracleModel(cfg, w).forward(fr[0])
  m0 = models.get_model(cfg, 0, weights=w, lib=lib)
  try:
    prod = m0.predict(fr[0])
    d0 = m0.engine(1, H, W).describe()
    assert d0["memory"]["keep_taps"] == 0
  finally:
    m0.close()
  m = models.get_model(_with_taps(cfg), 0, weights=w, lib=lib)
  try:
    out = m.predict(fr[0])
    boxes, labels, probs, feats = out[:4]
    for a, b in zip(prod, out):
      assert np.array_equal(a, b), "arena and keep_taps handles disagree"
    e = m.engine(1, H, W)
    _check_trunk(e, ref, tol)
    n = int(e.tap("nproposals")[0])
    assert n == ref["proposals"].shape[0] and n > 0
    pm, rm = match_detections(e.tap("proposals")[0, 0, :n], np.zeros(n), np.zeros(n), ref["proposals"], np.zeros(n),
                              np.zeros(n), 1e-3, 1)
    assert pm + rm == 0, "proposal sets differ: %d/%d of %d" % (pm, rm, n)
    # (b = 1: both sides keep the proposals in score order, row i of the engine is RoI i of the oracle)
    assert np.abs(e.tap("proposals")[0, 0, :n] - ref["proposals"]).max() <= 1e-3
    check_head_taps(e, cfg, w, tol, rec, np.arange(n))
    miss, extra = match_detections(boxes, labels, probs, ref["final_boxes"], ref["final_labels"], ref["final_probs"],
                                   1e-3, 1e-4)
    assert miss + extra == 0 and len(boxes) > 0, (miss, extra, len(boxes))
    assert_same_detections(boxes, labels, probs, feats, ref["final_boxes"], ref["final_labels"], ref["final_probs"],
                           ref["fpn_box_feat"], 1e-3, 1e-4, 10 * tol)
    d = e.describe()
    describe_ok(cfg, d0); describe_ok(cfg, d)
    if check is not None:
      check(m, e, d0, d, out, fr, ref)
    return out
  finally:
    m.close()


def run_multi(lib, cfg, B, H, W, tol=2e-5, check=None, seed=0):
  """gn_reference.run_multi against the 4conv1fc oracle (GroupNorm statistics per image in the trunk, per RoI in the head)."""
  w = weights(cfg, seed)
  fr = synthetic_frames(B, H, W)
  with head_oracle(cfg):
    ref = G.OracleModel(cfg, w).forward_multi(fr)
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
    check_head_taps(e, cfg, w, tol)
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
    describe_ok(cfg, d0); describe_ok(cfg, d)
    if check is not None:
      check(m, e, d0, d, (boxes, labels, probs, valid, feats), fr)
  finally:
    m.close()
