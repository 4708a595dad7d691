"""Reference side of the --use_deformable tests: a literal torch restatement of the reference's deformable stage-entry
bottleneck (nn.py:459-521 with deformable=True, deformable_conv2d nn.py:1642-1712, deformable_helper.py) -- gather-based and
following the helper module's steps, except that each image is sampled at its OWN offsets (the helper tiles the coordinates
batch-minor against batch-major image planes) -- a context manager that runs an OracleModel on it, float64
evaluations of the two kernels for the op-level tests, and the end-to-end comparisons of block_reference.py restated with this
feature's describe() check.  A helper module, not a conftest: the tests import it by name."""
import contextlib

import numpy as np
import pytest
import torch

import oracle.graph as G
from common import assert_same_detections, match_detections
from object_detection_tracking_amd import models
from object_detection_tracking_amd.weights import deformable_groups, synthetic_frames, synthetic_weights
from test_e2e import _check_trunk, _rel, _with_taps

_W = {}
captured = {}      # pre -> (offsets [B,H,W,18] as the last oracle forward computed them, H, W)


def weights(cfg, seed=0):
  key = (tuple(cfg.resnet_num_block), cfg.num_class, seed, bool(cfg.use_deformable))
  if key not in _W:
    _W[key] = synthetic_weights(cfg, seed)
  return _W[key]


# ------------------------------------------------------------------------------------------------- the literal block

def map_offsets(inputs, offsets):
  """_tf_batch_map_offsets + _tf_batch_map_coordinates on NHWC tensors, per-image offsets: inputs [B,H,W,C], offsets
  [B,H,W,18] -> [B,H,W,9,C]."""
  B, H, W, C = inputs.shape
  ky, kx = torch.meshgrid(torch.arange(3), torch.arange(3), indexing="ij")
  initial = torch.stack([ky, kx]).reshape(2, -1).t().to(torch.float32)                       # [9, 2]: (0,0), (0,1) ...
  gy, gx = torch.meshgrid(torch.arange(-1, H - 1), torch.arange(-1, W - 1), indexing="ij")
  grid = torch.stack([gy, gx], dim=-1).to(torch.float32)[:, :, None, :]                      # [H, W, 1, 2]
  grid_offset = grid + initial[None, None]                                                   # [H, W, 9, 2]
  coords = grid_offset[None] + offsets.reshape(B, H, W, 9, 2)
  coords = torch.stack([torch.clamp(coords[..., 0], 0.0, float(H - 1)), torch.clamp(coords[..., 1], 0.0, float(W - 1))], dim=-1)
  lt = torch.floor(coords).to(torch.int64)
  rb = torch.ceil(coords).to(torch.int64)
  idx = torch.arange(B)[:, None, None, None].expand(B, H, W, 9)

  def vals(r, c):
    return inputs[idx, r, c]                                                                 # gather_nd: [B,H,W,9,C]

  v_lt = vals(lt[..., 0], lt[..., 1]); v_rb = vals(rb[..., 0], rb[..., 1])
  v_lb = vals(lt[..., 0], rb[..., 1]); v_rt = vals(rb[..., 0], lt[..., 1])
  frac = coords - lt.to(torch.float32)
  v_t = v_lt + (v_rt - v_lt) * frac[..., 0:1]
  v_b = v_lb + (v_rb - v_lb) * frac[..., 0:1]
  return v_t + (v_b - v_t) * frac[..., 1:2]


def deformable_conv2d(l, offset, W):
  """nn.py:1642-1712 on NCHW l [B,C,H,W] and offset [B,18,H,W]; W HWIO [3,3,C,Cout]: conv3d of the mapped values with a
  [1,1,9] kernel and strides (2,2,1), VALID."""
  mapped = map_offsets(l.permute(0, 2, 3, 1).contiguous(), offset.permute(0, 2, 3, 1).contiguous())
  m = mapped[:, ::2, ::2]                                                                    # [B,Ho,Wo,9,C]
  B, Ho, Wo = m.shape[:3]
  out = m.reshape(B * Ho * Wo, -1) @ W.reshape(-1, W.shape[-1])
  return out.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


def deform_block(x, weights, pre, ch_out, stride, dilation):
  """resnet_bottleneck(deformable=True, stride=2), nn.py:459-521 (+ ReLU nn.py:587)."""
  assert stride == 2 and dilation == 1, "the reference graph does not build for a dilated deformable block"
  sc = x
  l = torch.relu(G.batch_norm(G.conv2d(x, weights, pre + "/conv1"), weights, pre + "/conv1/bn"))
  offset = G.conv2d(l, weights, pre + "/conv2_offset")                # 3x3, stride 1, SAME, + b; no norm, no activation
  captured[pre] = (offset.permute(0, 2, 3, 1).numpy().copy(), l.shape[2], l.shape[3])
  l = deformable_conv2d(l, offset, G._w(weights, pre + "/conv2/W"))   # no bias, no BN, no ReLU
  l = G.batch_norm(G.conv2d(l, weights, pre + "/conv3"), weights, pre + "/conv3/bn")
  sc = G.conv2d(sc[:, :, :-1, :-1], weights, pre + "/convshortcut", stride=2, padding="VALID")
  sc = G.batch_norm(sc, weights, pre + "/convshortcut/bn")
  return torch.relu(l + sc)


@contextlib.contextmanager
def deform_oracle(cfg):
  """While active, oracle.graph's backbone runs deform_block where the reference would (resnet_group, nn.py:574-585: block 0
  of a stride-2 group with at most three blocks), decided from the scope, the stride and resnet_num_block."""
  saved = G.bottleneck

  def block(x, weights, pre, ch_out, stride, dilation):
    g = int(pre[len("group")])
    if cfg.use_deformable and stride == 2 and pre.endswith("/block0") and cfg.resnet_num_block[g] <= 3:
      return deform_block(x, weights, pre, ch_out, stride, dilation)
    return saved(x, weights, pre, ch_out, stride, dilation)

  G.bottleneck = block
  captured.clear()
  try:
    yield
  finally:
    G.bottleneck = saved


# ------------------------------------------------------------------------------------------------- float64, op level

def offsets64(x, w_off, b_off):
  """conv2_offset at the even positions in float64: 3x3, stride 2, one zero row / column in front (what is needed behind).
  Returns (offsets [B,Ho,Wo,18], sum |x w| + |b| per output)."""
  B, H, W, C = x.shape
  Ho, Wo = (H + 1) // 2, (W + 1) // 2

  def conv(xa, wa, ba):
    xt = torch.from_numpy(xa).double().permute(0, 3, 1, 2)
    xt = torch.nn.functional.pad(xt, (1, 2 * (Wo - 1) + 2 - W, 1, 2 * (Ho - 1) + 2 - H))
    y = torch.nn.functional.conv2d(xt, torch.from_numpy(wa).double().permute(3, 2, 0, 1), torch.from_numpy(ba).double(), stride=2)
    return y.permute(0, 2, 3, 1).numpy()

  ref = conv(x, w_off, b_off)
  assert ref.shape == (B, Ho, Wo, 18)
  return ref, conv(np.abs(x), np.abs(w_off), np.abs(b_off))


def sample_coords(off, H, W):
  """The clamped f32 sample coordinates for offsets [B,Ho,Wo,18] at the even positions: the coordinate is formed by ONE f32
  addition, as in the reference.  Returns (r, c) [B,Ho,Wo,9] float32 and the unclamped pair."""
  B, Ho, Wo, _ = off.shape
  n = np.arange(9)
  y = (2 * np.arange(Ho))[None, :, None, None] - 1 + (n // 3)[None, None, None, :]
  x = (2 * np.arange(Wo))[None, None, :, None] - 1 + (n % 3)[None, None, None, :]
  o = off.astype(np.float32).reshape(B, Ho, Wo, 9, 2)
  r_raw = y.astype(np.float32) + o[..., 0]
  c_raw = x.astype(np.float32) + o[..., 1]
  assert r_raw.dtype == np.float32 and c_raw.dtype == np.float32
  return np.clip(r_raw, 0, np.float32(H - 1)), np.clip(c_raw, 0, np.float32(W - 1)), r_raw, c_raw


def deform64(x, off, w):
  """The deformable conv in float64 at the given f32 offsets.  Returns (out [B,Ho,Wo,C], the bound's magnitude
  sum_n |W_n|^T (|lt| + |rt| + |lb| + |rb|))."""
  B, H, W, C = x.shape
  r, c, _, _ = sample_coords(off, H, W)
  r0 = np.floor(r).astype(np.int64); r1 = np.ceil(r).astype(np.int64)
  c0 = np.floor(c).astype(np.int64); c1 = np.ceil(c).astype(np.int64)
  fr = (r.astype(np.float64) - r0)[..., None]; fc = (c.astype(np.float64) - c0)[..., None]
  bi = np.arange(B)[:, None, None, None]
  xd = x.astype(np.float64)
  lt = xd[bi, r0, c0]; rt = xd[bi, r1, c0]; lb = xd[bi, r0, c1]; rb = xd[bi, r1, c1]          # [B,Ho,Wo,9,C]
  vt = lt + (rt - lt) * fr
  vb = lb + (rb - lb) * fr
  s = vt + (vb - vt) * fc
  wd = w.astype(np.float64).reshape(9 * C, -1)
  Ho, Wo = r.shape[1:3]
  out = s.reshape(B * Ho * Wo, 9 * C) @ wd
  mag = (np.abs(lt) + np.abs(rt) + np.abs(lb) + np.abs(rb)).reshape(B * Ho * Wo, 9 * C) @ np.abs(wd)
  return out.reshape(B, Ho, Wo, -1), mag.reshape(B, Ho, Wo, -1)


# ------------------------------------------------------------------------------------------------- end to end

def _describe_ok(cfg, d):
  assert d["block_kind"] == "bottleneck" and d["group_conv_launches"] == 0 and d["use_se"] == 0, d
  assert d["use_deformable"] == 1 and d["deform_conv_launches"] == len(deformable_groups(cfg)), d


def run_single(lib, cfg, H, W, tol=2e-5, w=None, check=None):
  """block_reference.run_single against deform_block: the production handle against the keep_taps handle bit for bit, trunk
  taps 2e-5 of the tensor maximum, proposals and detections pair by pair (boxes 1e-3 px, scores 1e-4, features 10x the trunk
  tolerance); mismatch budget 0."""
  w = weights(cfg) if w is None else w
  fr = synthetic_frames(1, H, W)
  with deform_oracle(cfg):
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
    for t in ("c2", "c3", "c4", "c5"):
      print("trunk %s: rel err %.3g (tolerance %.3g)" % (t, _rel(e.tap(t).transpose(0, 3, 1, 2), ref[t]), tol))
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


def run_multi(lib, cfg, B, H, W, tol=2e-5, check=None):
  """block_reference.run_multi against deform_block (per-image offsets)."""
  w = weights(cfg)
  fr = synthetic_frames(B, H, W)
  with deform_oracle(cfg):
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
