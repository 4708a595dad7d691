"""Reference side of the --use_gn tests: a literal torch restatement of the reference's group_norm (nn.py:81-108: reshape to
[B,32,C/32,h,w], tf.nn.moments over (2,3,4), tf.nn.batch_normalization with gamma / beta reshaped to [1,32,C/32,1,1], eps 1e-5),
a context manager that runs an OracleModel on the GroupNorm graph without editing oracle/ (oracle/graph.py calls batch_norm and
fpn by module-level name), a float64 evaluation of the op for the op-level tests, and the end-to-end comparisons of
deformable_reference.py restated with this feature's describe() check.  A helper module, not a conftest: the tests import it
by name."""
import contextlib

import numpy as np
import pytest
import torch

import oracle.graph as G
from common import assert_same_detections, match_detections
from object_detection_tracking_amd import models
from object_detection_tracking_amd.weights import group_norm_scopes, synthetic_frames, synthetic_weights
from test_e2e import _check_trunk, _rel, _with_taps

_W = {}
EPS = 1e-5


def weights(cfg, seed=0):
  key = (tuple(cfg.resnet_num_block), cfg.num_class, seed, bool(cfg.use_gn))
  if key not in _W:
    _W[key] = synthetic_weights(cfg, seed)
  return _W[key]


# ------------------------------------------------------------------------------------------------- the literal op

def group_norm(x, gamma, beta, group=32, eps=EPS):
  """nn.py:81-108 on NCHW x [B,C,h,w] (torch, any float dtype); gamma, beta [C]."""
  B, C, h, w = x.shape
  gs = C // group
  xr = x.reshape(B, group, gs, h, w)
  mean = xr.mean(dim=(2, 3, 4), keepdim=True)
  var = xr.var(dim=(2, 3, 4), unbiased=False, keepdim=True)
  g = gamma.reshape(1, group, gs, 1, 1); b = beta.reshape(1, group, gs, 1, 1)
  inv = torch.rsqrt(var + eps) * g                      # tf.nn.batch_normalization's operand order
  out = xr * inv + (b - mean * inv)
  return out.reshape(B, C, h, w)


def _gn_scope(weights, x, scope):
  return group_norm(x, G._w(weights, scope + "/gamma"), G._w(weights, scope + "/beta"))


def gn_fpn(c2345, weights):
  """nn.py:947-1014 with use_gn: lateral 1x1 -> fpn/gn_cN -> top-down sums (no ReLU); posthoc 3x3 -> fpn/gn_pN on the full maps;
  P6 = the subsample of the normalised P5."""
  lat = [_gn_scope(weights, G.conv2d(c, weights, "fpn/lateral_1x1_c%d" % (i + 2)), "fpn/gn_c%d" % (i + 2)) for i, c in enumerate(c2345)]
  sums = []
  for idx, l in enumerate(lat[::-1]):
    if idx > 0:
      l = l + sums[-1].repeat_interleave(2, 2).repeat_interleave(2, 3)
    sums.append(l)
  p = [_gn_scope(weights, G.conv2d(c, weights, "fpn/posthoc_3x3_p%d" % (i + 2)), "fpn/gn_p%d" % (i + 2)) for i, c in enumerate(sums[::-1])]
  return p + [p[-1][:, :, ::2, ::2]]


@contextlib.contextmanager
def gn_oracle():
  """While active, oracle.graph.batch_norm dispatches a scope X/bn to GroupNorm over X/gn/{gamma,beta} (the backbone: conv0
  and every conv of a bottleneck; the zero row / column of a dilated stage entry is padded behind it, as in the reference) and
  oracle.graph.fpn is the GroupNorm form."""
  saved = (G.batch_norm, G.fpn)

  def bn(x, weights, scope, eps=EPS):
    assert scope.endswith("/bn"), scope
    return _gn_scope(weights, x, scope[:-3] + "/gn")

  G.batch_norm, G.fpn = bn, gn_fpn
  try:
    yield
  finally:
    G.batch_norm, G.fpn = saved


# ------------------------------------------------------------------------------------------------- float64, op level

def group_norm64(x, gamma, beta, res=None, upsample=False, relu=False, eps=EPS):
  """The op in float64 on NHWC x [B,h,w,C].  Returns (out, mean [B,32], var [B,32], a [B,C], E[x^2] [B,32], mean|x| [B,32]),
  all float64."""
  B, h, w, C = x.shape
  gs = C // 32
  xd = x.astype(np.float64).reshape(B, h * w, 32, gs)
  mean = xd.mean(axis=(1, 3)); var = ((xd - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
  ex2 = (xd ** 2).mean(axis=(1, 3)); mabs = np.abs(xd).mean(axis=(1, 3))
  a = (1.0 / np.sqrt(var + float(np.float32(eps))))[:, :, None] * gamma.astype(np.float64).reshape(1, 32, gs)
  s = beta.astype(np.float64).reshape(1, 32, gs) - mean[:, :, None] * a
  out = (xd * a[:, None] + s[:, None]).reshape(B, h, w, C)
  if res is not None:
    r = res.astype(np.float64)
    if upsample:
      r = r.repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w]
    out = out + r
  if relu:
    out = np.maximum(out, 0.0)
  return out, mean, var, a.reshape(B, C), ex2, mabs


# ------------------------------------------------------------------------------------------------- end to end

def _describe_ok(cfg, d):
  assert d["block_kind"] == "bottleneck" and d["use_se"] == 0 and d["use_deformable"] == 0, d
  assert d["use_gn"] == 1 and d["group_norms"] == len(group_norm_scopes(cfg)) == 3 * sum(cfg.resnet_num_block) + 4 + 1 + 8, d
  # the fusions a normalisation cuts through are off
  assert d["stem_fused"] == 0 and d["bottleneck_tails_fused"] == 0 and d["bottleneck_blocks_fused"] == 0, d


def run_single(lib, cfg, H, W, tol=2e-5, w=None, check=None, seed=0):
  """deformable_reference.run_single against the GroupNorm oracle: the production handle against the keep_taps handle bit for
  bit, trunk taps 2e-5 of the tensor maximum, proposals and detections pair by pair (boxes 1e-3 px, scores 1e-4, features 10x
  the trunk tolerance); mismatch budget 0."""
  w = weights(cfg, seed) if w is None else w
  fr = synthetic_frames(1, H, W)
  with gn_oracle():
    ref = G.OracleModel(cfg, w).forward(fr[0])
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
    out = m.predict(fr[0])
    boxes, labels, probs, feats = out[:4]
    for a, b in zip(prod, out):
      assert np.array_equal(a, b), "arena and keep_taps handles disagree"
    e = m.engine(1, H, W)
    for t in ("conv0", "pool0", "c2", "c3", "c4", "c5", "p2", "p3", "p4", "p5", "p6"):
      r = ref[t]
      got = e.tap(t).transpose(0, 3, 1, 2)[:, :, :r.shape[2], :r.shape[3]]
      print("trunk %s: rel err %.3g (tolerance %.3g)" % (t, _rel(got, r), tol))
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
    _describe_ok(cfg, d0); _describe_ok(cfg, d)
    if check is not None:
      check(m, e, d0, d, out, fr, ref)
    return out
  finally:
    m.close()


def run_multi(lib, cfg, B, H, W, tol=2e-5, check=None, seed=0):
  """deformable_reference.run_multi against the GroupNorm oracle (statistics per image)."""
  w = weights(cfg, seed)
  fr = synthetic_frames(B, H, W)
  with gn_oracle():
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
    _describe_ok(cfg, d0); _describe_ok(cfg, d)
    if check is not None:
      check(m, e, d0, d, (boxes, labels, probs, valid, feats), fr)
  finally:
    m.close()
