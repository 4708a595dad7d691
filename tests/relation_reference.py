"""Reference side of the --add_relation_nn tests: a literal torch restatement, in float64, of the reference's relation module
(relation_network nn.py:115-190 over geometric_encoding nn.py:273-298) and of the 2-FC box head that carries two of them
(models.py:1044-1054: h6' = h6 + RM_r1(h6, boxes), h7' = h7 + RM_r2(h7, boxes)), a context manager that runs an OracleModel on
that head without editing oracle/, and the end-to-end comparison of conv_head_reference.run_single restated with this feature's
taps.  A helper module, not a conftest: the tests import it by name.

oracle.graph calls box_head(roi_feat, ...) by module-level name and does not pass the proposal boxes, which the relation head
needs.  The call in front of it, multilevel_roi_align(p, boxes, ...), does: relation_oracle wraps that function too and hands
the boxes of its last call with as many rows as roi_feat to the head.

Tap tolerance.  The project holds taps to 2e-5 of the tensor maximum.  A softmax multiplies logit error, so the tolerance of the
relation taps (the attention output and h + RM) is max(2e-5, 4 x d), where d is the distance -- relative to the tensor maximum --
between a float32 and the float64 torch evaluation of this literal module on the same inputs; the factor 4 leaves room for
another summation order and the device's tanhf / expf / logf.  Measured on the CPU, weights of seeds 0 - 5 (the oracle's
roi_feat and proposals of the 96 x 128 synthetic frame, D = 1024, n = K = 32): d = 4.0e-7 .. 2.8e-6 at the attention outputs and
3.3e-7 .. 6.1e-7 at h + RM, so 4 x d <= 1.1e-5 < 2e-5 and the asserted tolerance is TAP_TOL = 2e-5, the project's own.  (The
kernels measure 2.0e-6 .. 4.1e-6 against float64 on the simulator and the MI355X; the fp16x2 / bf16x3 Q | K projection meets
the tolerance, so no layer had to move to the exact-f32 kernel.)  tol_measure repeats the measurement on an engine's taps.

Condition on the synthetic weights (weights_informative, asserted on the reference alone, so that a uniform or one-hot softmax
cannot hide a wrong kernel): over real rows and heads the median of max_j P lies in [2 / n, 0.9] and the share of relu(a) > 0 in
[0.1, 0.9]."""
import contextlib
import math

import numpy as np
import torch

import oracle.graph as G
from common import assert_same_detections, match_detections
from object_detection_tracking_amd import models
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights
from test_e2e import _check_trunk, _rel, _with_taps

GROUP = 16
TAP_TOL = 2e-5
_W = {}


def weights(cfg, seed=0):
  key = (tuple(cfg.resnet_num_block), cfg.num_class, seed, bool(cfg.use_gn), bool(cfg.add_relation_nn),
         int(cfg.fpn_frcnn_fc_head_dim), bool(getattr(cfg, "use_frcnn_class_agnostic", False)))
  if key not in _W:
    _W[key] = synthetic_weights(cfg, seed)
  return _W[key]


def _t(a, dtype):
  return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype)


def geometric_bias(boxes, geo_emb, geo_conv, dtype=torch.float64):
  """boxes [n,4] -> (bias [n,16,n] = log(max(relu(a), 1e-6)), a [n,n,16]); nn.py:273-298, 123-143, 170."""
  b = _t(boxes, dtype)
  x1, y1, x2, y2 = b[:, 0:1], b[:, 1:2], b[:, 2:3], b[:, 3:4]
  w = x2 - x1
  h = y2 - y1
  cx = 0.5 * (x1 + x2)
  cy = 0.5 * (y1 + y2)
  lo = torch.tensor(1e-3, dtype=dtype)
  dx = torch.log(torch.maximum(torch.abs((cx - cx.t()) / w), lo))
  dy = torch.log(torch.maximum(torch.abs((cy - cy.t()) / w), lo))      # (over w, as the reference has it)
  dw = torch.log(w / w.t())
  dh = torch.log(h / h.t())
  e = torch.stack([dx, dy, dw, dh], dim=2)                                # [n,n,4]
  g = torch.tanh(e @ _t(geo_emb[0], dtype) + _t(geo_emb[1], dtype))       # [n,n,64]
  a = g @ _t(geo_conv[0], dtype).reshape(64, GROUP) + _t(geo_conv[1], dtype)      # [n,n,16]
  bias = torch.log(torch.maximum(torch.relu(a), torch.tensor(1e-6, dtype=dtype))).permute(0, 2, 1)
  return bias, a


def attention(q, k, v, bias, dtype=torch.float64):
  """q, k, v [n,D], bias [n,16,n] -> (O [n,16,D], P [n,16,n]); nn.py:151-183."""
  q, k, v, bias = _t(q, dtype), _t(k, dtype), _t(v, dtype), _t(bias, dtype)
  n, D = q.shape
  dh = D // GROUP
  qh = q.reshape(n, GROUP, dh).permute(1, 0, 2)
  kh = k.reshape(n, GROUP, dh).permute(1, 0, 2)
  logits = (1.0 / math.sqrt(float(dh))) * torch.matmul(qh, kh.transpose(1, 2))      # [16,n,n]
  s = bias + logits.permute(1, 0, 2)                                                # [n,16,n]
  p = torch.softmax(s, dim=-1)
  o = torch.matmul(p.reshape(n * GROUP, n), v).reshape(n, GROUP, D)
  return o, p


def relation_module(f, boxes, weights, scope, dtype=torch.float64, rec=None):
  """RM(f [n,D], boxes [n,4]) over the variables scope/...; rec receives "attn" (O), "P" and "a"."""
  def wv(name):
    return np.asarray(weights[scope + "/" + name])
  f = _t(f, dtype)
  bias, a = geometric_bias(boxes, (wv("geo_emb/W"), wv("geo_emb/b")), (wv("geo_conv/W"), wv("geo_conv/b")), dtype)
  q = f @ _t(wv("query_linear/W"), dtype)
  k = f @ _t(wv("key_linear/W"), dtype)
  o, p = attention(q, k, f, bias, dtype)
  if rec is not None:
    rec["attn"] = o.numpy(); rec["P"] = p.numpy(); rec["a"] = a.numpy()
  return o.reshape(f.shape[0], -1) @ _t(wv("output_linear/W"), dtype)


def relation_head(roi_flat, boxes, weights, dtype=torch.float64, rec=None):
  """roi_flat [n, C*49] (NCHW-flattened, as fc6 reads it) -> h7' [n,D]; rec receives rm_r1, rm_r2 (h6', h7') and the two
  modules' own records under "r1" / "r2"."""
  def wv(name):
    return _t(weights[name], dtype)
  x = _t(roi_flat, dtype)
  r1, r2 = {}, {}
  h6 = torch.relu(x @ wv("fastrcnn/fc6/W") + wv("fastrcnn/fc6/b"))
  h6 = h6 + relation_module(h6, boxes, weights, "fastrcnn/RM_r1", dtype, r1)
  h7 = torch.relu(h6 @ wv("fastrcnn/fc7/W") + wv("fastrcnn/fc7/b"))
  h7p = h7 + relation_module(h7, boxes, weights, "fastrcnn/RM_r2", dtype, r2)
  if rec is not None:
    rec.update(rm_r1=h6.numpy(), rm_r2=h7p.numpy(), fc7=h7.numpy(), r1=r1, r2=r2)
  return h7p


def relation_box_head(get_boxes, rec=None):
  """The relation head with the arguments of oracle.graph.box_head (float64 inside, float32 out, as the oracle's tensors are)."""

  def box_head(roi_feat, weights, num_class, partial_ids=None, class_agnostic=False):
    with torch.no_grad():
      boxes = get_boxes(roi_feat.shape[0])
      r = {}
      h = relation_head(roi_feat.reshape(roi_feat.shape[0], -1), boxes, weights, torch.float64, r)
      cls = h @ _t(weights["fastrcnn/outputs/class/W"], torch.float64) + _t(weights["fastrcnn/outputs/class/b"], torch.float64)
      box = h @ _t(weights["fastrcnn/outputs/box/W"], torch.float64) + _t(weights["fastrcnn/outputs/box/b"], torch.float64)
      if class_agnostic:
        box = box.reshape(-1, 1, 4).repeat(1, num_class - 1, 1)
      else:
        box = box.reshape(-1, num_class, 4)[:, 1:, :]
    if rec is not None:
      rec.update(r)
    cls, box = cls.numpy().astype(np.float32), np.ascontiguousarray(box.numpy().astype(np.float32))
    if partial_ids is not None:
      ids = [int(i) for i in partial_ids]
      cls = np.ascontiguousarray(cls[:, [0] + ids])
      box = np.ascontiguousarray(box[:, [i - 1 for i in ids], :])
    return cls, box

  return box_head


@contextlib.contextmanager
def relation_oracle(cfg):
  """While active, oracle.graph.box_head is the relation head, fed with the boxes of the multilevel_roi_align call in front of
  it (and, under cfg.use_gn, the trunk is gn_oracle's).  Yields the dict the head records its taps in."""
  rec, last = {}, {}
  saved_head, saved_roi = G.box_head, G.multilevel_roi_align

  def roi_align(features, boxes, *a, **kw):
    last["boxes"] = np.asarray(boxes).copy()
    return saved_roi(features, boxes, *a, **kw)

  def get_boxes(rows):
    assert last["boxes"].shape == (rows, 4), (last["boxes"].shape, rows)
    return last["boxes"]

  G.box_head = relation_box_head(get_boxes, rec)
  G.multilevel_roi_align = roi_align
  try:
    if cfg.use_gn:
      import gn_reference as GR
      with GR.gn_oracle():
        yield rec
    else:
      yield rec
  finally:
    G.box_head, G.multilevel_roi_align = saved_head, saved_roi


def weights_informative(rec, n):
  """The condition on the synthetic weights, on the reference's own records of the two modules."""
  for r in (rec["r1"], rec["r2"]):
    pmax = float(np.median(r["P"].max(axis=-1)))
    share = float((r["a"] > 0).mean())
    print("relation weights: median max_j P %.3f (in [%.3f, 0.9]), share of relu(a) > 0 %.3f" % (pmax, 2.0 / n, share))
    assert 2.0 / n <= pmax <= 0.9, pmax
    assert 0.1 <= share <= 0.9, share


def engine_head_reference(e, cfg, w, dtype=torch.float64):
  """The literal head on the engine's own roi_feat and proposals taps, real rows only: (n, rec)."""
  n = int(e.tap("nproposals")[0])
  roi = e.tap("roi_feat")
  K = roi.shape[2]
  roi = np.ascontiguousarray(roi.reshape(K, 7, 7, -1).transpose(0, 3, 1, 2)).reshape(K, -1)[:n]
  boxes = e.tap("proposals")[0, 0, :n]
  rec = {}
  with torch.no_grad():
    relation_head(roi, boxes, w, dtype, rec)
  return n, rec


def check_relation_taps(e, cfg, w, tol=TAP_TOL):
  """rm_r1, rm_r2 [1,1,K,D] and rm_r1_attn, rm_r2_attn [1,1,K,16 D] of a keep_taps engine against the literal module evaluated
  in float64 on the engine's own roi_feat and proposals taps (conv_head_reference.check_head_taps says why not against the
  end-to-end oracle's): tol of the tensor maximum over the n real rows; the padded rows of the attention outputs are exactly
  zero and every tap is finite.  Returns (n, rec)."""
  n, rec = engine_head_reference(e, cfg, w)
  D = int(cfg.fpn_frcnn_fc_head_dim)
  K = int(cfg.rpn_test_post_nms_topk)
  for name, ref in (("rm_r1_attn", rec["r1"]["attn"].reshape(n, -1)), ("rm_r1", rec["rm_r1"]),
                    ("rm_r2_attn", rec["r2"]["attn"].reshape(n, -1)), ("rm_r2", rec["rm_r2"])):
    got = e.tap(name)
    assert got.shape == (1, 1, K, ref.shape[1]) and ref.shape[1] in (D, 16 * D), (name, got.shape)
    got = got.reshape(K, -1)
    assert np.isfinite(got).all(), name
    err = _rel(got[:n].astype(np.float64), ref)
    print("relation tap %s: rel err %.3g (tolerance %.3g)" % (name, err, tol))
    assert err < tol, (name, err)
    if name.endswith("_attn"):
      assert not got[n:].any(), name + ": padded rows are not zero"
  return n, rec


def describe_ok(cfg, d):
  assert d["box_head"] == "2fc+relation" and d["relation_modules"] == 2, d
  assert d["use_gn"] == int(bool(cfg.use_gn)), d


def run_single(lib, cfg, H, W, tol=2e-5, check=None, seed=0):
  """conv_head_reference.run_single against the relation oracle: the production handle against the keep_taps handle bit for bit,
  trunk taps tol of the tensor maximum, the relation taps (check_relation_taps) TAP_TOL, proposals and detections pair by pair
  (boxes 1e-3 px, scores 1e-4, features 10x the tap tolerance); mismatch budget 0."""
  w = weights(cfg, seed)
  fr = synthetic_frames(1, H, W)
  m0 = models.get_model(cfg, 0, weights=w, lib=lib)        # (first: a tree without the feature raises NotImplementedError here)
  try:
    prod = m0.predict(fr[0])
    d0 = m0.engine(1, H, W).describe()
    assert d0["memory"]["keep_taps"] == 0
  finally:
    m0.close()
  with relation_oracle(cfg) as rec:
    ref = G.OracleModel(cfg, w).forward(fr[0])
  weights_informative(rec, ref["proposals"].shape[0])
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
    assert np.abs(e.tap("proposals")[0, 0, :n] - ref["proposals"]).max() <= 1e-3
    check_relation_taps(e, cfg, w)
    for name in ("rm_r1", "rm_r2"):
      print("  %s against the end-to-end oracle's (not asserted): %.3g" % (name, _rel(e.tap(name).reshape(-1, rec[name].shape[1])[:n], rec[name])))
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


def tol_measure(e, cfg, w):
  """d of the module docstring on one engine: the float32 against the float64 torch evaluation of the literal head on the
  engine's roi_feat and proposals, relative to the tensor maximum, per relation tap."""
  n, r64 = engine_head_reference(e, cfg, w, torch.float64)
  _, r32 = engine_head_reference(e, cfg, w, torch.float32)
  return {"rm_r1_attn": _rel(r32["r1"]["attn"].astype(np.float64), r64["r1"]["attn"]), "rm_r1": _rel(r32["rm_r1"].astype(np.float64), r64["rm_r1"]),
          "rm_r2_attn": _rel(r32["r2"]["attn"].astype(np.float64), r64["r2"]["attn"]), "rm_r2": _rel(r32["rm_r2"].astype(np.float64), r64["rm_r2"])}
