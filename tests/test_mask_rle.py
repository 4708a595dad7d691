"""Mask paste + COCO RLE on the device (csrc/mask_rle.hip: odt_op_mask_rle, odt_mask_rle, Mask_RCNN_FPN.masks_rle) against
the reference restated here: obj_detect_tracking.py:715-739 divides final_boxes by scale, fill_full_mask (nn.py:1565-1584)
resizes each 28x28 mask to its integer box with cv2.resize (INTER_LINEAR) and pastes it into an all-zero frame, and
pycocotools encodes the frame column-major (rleEncode) into its compressed string (rleToString).

Geometry: the frame decoded from the device counts must equal the reference frame except at pixels whose float64
interpolant lies within 1e-6 of 0.5 (the number excluded is reported); against nn.fill_full_mask -- the float32 host
restatement whose operations the kernel follows -- it must be equal outright.  Encoding (exact): re-encoding the decoded
frame gives the device counts, the device string is rleToString of those counts, rleFrString gives them back.  Rectangles
past the frame: the reference raises, the device clips (include/odt.h).  Every odt_op_mask_rle call checks the guard
regions behind its buffers: a write past the end fails the call.
"""
import os

import numpy as np
import pytest

from common import small_config, weights_for
from object_detection_tracking_amd import models, nn, ops
from object_detection_tracking_amd._lib import OdtError
from object_detection_tracking_amd.weights import synthetic_frames
from oracle import imgproc

F = np.float32
NEAR = 1e-6


# ------------------------------------------------------------------------------------------- reference restatement

def _taps64(n_src, n_dst):
  f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / n_dst) - 0.5
  i0 = np.floor(f).astype(np.int64)
  fr = f - i0
  fr[i0 < 0] = 0.0
  i0 = np.maximum(i0, 0)
  over = i0 >= n_src - 1
  i0[over] = n_src - 1
  fr[over] = 0.0
  return i0, np.minimum(i0 + 1, n_src - 1), fr


def resize64(m, h, w):
  """separable INTER_LINEAR in float64, the horizontal pass first (cv2.resize(m, (w, h)))."""
  m = np.asarray(m, np.float64)
  x0, x1, fx = _taps64(m.shape[1], w)
  y0, y1, fy = _taps64(m.shape[0], h)
  hc = m[:, x0] * (1.0 - fx) + m[:, x1] * fx
  return hc[y0] * (1.0 - fy)[:, None] + hc[y1] * fy[:, None]


def rect(box, scale):
  """fill_full_mask's integer rectangle of final_boxes[j] / scale (float32 arithmetic as numpy does it)."""
  b = np.asarray(box, F) / F(scale)
  x0, y0 = int(b[0] + F(0.5)), int(b[1] + F(0.5))
  x1, y1 = int(b[2] - F(0.5)), int(b[3] - F(0.5))
  return x0, y0, max(x0, x1), max(y0, y1)


def paste64(box, mask, H, W, scale=1.0):
  """(frame uint8, float64 interpolant on the frame, NaN outside the rectangle); the rectangle clipped to the frame."""
  x0, y0, x1, y1 = rect(box, scale)
  v = resize64(mask, y1 + 1 - y0, x1 + 1 - x0)
  full = np.full((H, W), np.nan)
  cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
  if cx0 <= cx1 and cy0 <= cy1:
    full[cy0:cy1 + 1, cx0:cx1 + 1] = v[cy0 - y0:cy1 + 1 - y0, cx0 - x0:cx1 + 1 - x0]
  return (full > 0.5).astype(np.uint8), full


def rle_encode(frame):
  """pycocotools rleEncode of one [H, W] frame: run lengths of the column-major flattening, zeros first."""
  f = np.asarray(frame, np.uint8).T.reshape(-1).astype(np.int8)
  t = np.flatnonzero(np.diff(np.concatenate([[0], f])))
  return np.diff(np.concatenate([[0], t, [f.size]])).astype(np.uint32)


def rle_decode(counts, H, W):
  v = np.repeat(np.arange(len(counts)) % 2, np.asarray(counts, np.int64)).astype(np.uint8)
  assert v.size == H * W, (v.size, H, W)
  return v.reshape(W, H).T


def rle_to_string(cnts):
  """pycocotools rleToString."""
  s = []
  for i in range(len(cnts)):
    x = int(cnts[i])
    if i > 2:
      x -= int(cnts[i - 2])
    more = True
    while more:
      c = x & 0x1f
      x >>= 5
      more = (x != -1) if (c & 0x10) else (x != 0)
      if more:
        c |= 0x20
      s.append(chr(c + 48))
  return "".join(s)


def rle_fr_string(s):
  """pycocotools rleFrString."""
  cnts, p = [], 0
  while p < len(s):
    x, k, more = 0, 0, True
    while more:
      c = ord(s[p]) - 48
      x |= (c & 0x1f) << (5 * k)
      more = bool(c & 0x20)
      p += 1
      k += 1
      if not more and (c & 0x10):
        x |= -1 << (5 * k)
    if len(cnts) > 2:
      x += cnts[-2]
    cnts.append(x)
  return cnts


def check(rles, counts, boxes, masks, H, W, scale=1.0, exact_host=True):
  """Geometry and encoding of every detection; returns the number of pixels excluded near 0.5."""
  assert len(rles) == len(boxes) == len(counts)
  excluded = 0
  for j, (r, c) in enumerate(zip(rles, counts)):
    assert r["size"] == [H, W], r["size"]
    dev = rle_decode(c, H, W)
    ref, v64 = paste64(boxes[j], masks[j], H, W, scale)
    bad = dev != ref
    near = np.abs(v64 - 0.5) <= NEAR          # (NaN outside the rectangle: never near)
    assert not np.any(bad & ~near), (j, int(np.sum(bad & ~near)), rect(boxes[j], scale))
    excluded += int(np.sum(bad & near))
    if exact_host:      # the float32 host restatement, where the reference does not raise: bit for bit
      b = np.asarray(boxes[j], F) / F(scale)
      x0, y0, x1, y1 = rect(boxes[j], scale)
      if x0 >= 0 and y0 >= 0 and x1 < W and y1 < H:
        assert np.array_equal(dev, nn.fill_full_mask(b, masks[j], (H, W))), j
    assert np.array_equal(rle_encode(dev), c), j
    assert r["counts"] == rle_to_string(c), j
    assert rle_fr_string(r["counts"]) == [int(x) for x in c], j
  return excluded


# ------------------------------------------------------------------------------------------- the restatement itself

@pytest.mark.parametrize("h,w", [(1, 1), (5, 9), (28, 28), (41, 17), (63, 80)])
def test_resize64_matches_oracle_inter_linear(h, w):
  m = np.random.default_rng(h * 100 + w).random((28, 28)).astype(F)
  assert np.array_equal(resize64(m, h, w).astype(F), imgproc.inter_linear(m, h, w))


def test_rle_restatement_round_trip():
  rng = np.random.default_rng(1)
  fr = (rng.random((13, 17)) > 0.6).astype(np.uint8)
  c = rle_encode(fr)
  assert np.array_equal(rle_decode(c, 13, 17), fr) and int(c.sum()) == 13 * 17
  assert rle_fr_string(rle_to_string(c)) == [int(x) for x in c]
  assert list(rle_encode(np.zeros((4, 6), np.uint8))) == [24]
  assert list(rle_encode(np.ones((4, 6), np.uint8))) == [0, 24]
  big = [0, 3, 70000, 5, 1 << 20, 12, 2]      # negative deltas (i > 2) and multi-group values
  assert rle_fr_string(rle_to_string(big)) == big


def test_host_fill_full_mask_raises_like_the_reference():
  m = np.full((28, 28), 0.9, F)
  out = nn.fill_full_mask(np.array([2.2, 3.7, 9.6, 12.1], F), m, (20, 16))
  assert out.dtype == np.uint8 and out[4:12, 2:10].all() and out.sum() == 8 * 8
  with pytest.raises(ValueError):
    nn.fill_full_mask(np.array([2.0, 3.0, 19.0, 12.0], F), m, (20, 16))     # past the right edge


# ------------------------------------------------------------------------------------------- stand-alone op

def _masks(kind, rng, n=1):
  if kind == "zero":
    return np.zeros((n, 28, 28), F)
  if kind == "one":
    return np.ones((n, 28, 28), F)
  if kind == "half":
    return np.full((n, 28, 28), 0.5, F)
  if kind == "smooth":
    yy, xx = np.mgrid[0:28, 0:28]
    out = []
    for _ in range(n):
      cy, cx, s = rng.uniform(6, 22), rng.uniform(6, 22), rng.uniform(3, 9)
      out.append(np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)))
    return np.asarray(out, F)
  if kind == "noise":
    return rng.random((n, 28, 28)).astype(F)
  if kind == "rows":        # row-alternating: every source interval of every column crosses 0.5
    m = np.zeros((n, 28, 28), F)
    m[:, 1::2] = 1.0
    return m
  raise ValueError(kind)


def _edge_boxes(H, W):
  return np.array([
      [10.3, 7.8, 9.1, 6.0],                    # x2 < x1, y2 < y1: the 1 x 1 box after max()
      [4.2, 3.1, 20.7, 14.9],                   # under 28 px: downscale
      [0.0, 0.0, W, H],                         # the full frame
      [0.0, 5.0, 12.0, 20.0],                   # left edge
      [W - 13.0, 2.0, W, 15.0],                 # right edge
      [7.0, 0.0, 25.0, 9.0],                    # top edge
      [3.0, H - 11.0, 30.0, H],                 # bottom edge
      [W - 9.0, H - 8.0, W + 14.0, H + 20.0],   # past the bottom-right corner (clipped)
      [-6.0, -9.0, 12.0, 10.0],                 # past the top-left corner (clipped)
      [-4.0, 3.0, W + 6.0, H + 3.0],            # wider and taller than the frame (clipped)
      [W + 5.0, 2.0, W + 20.0, 9.0],            # entirely outside: nothing
  ], F)


def _round_across_boxes(rng, scale, n):
  """boxes whose float32 b = v / scale gives int(b + 0.5f) or int(b - 0.5f) other than float64 would: the +/- 0.5 rounds
  across an integer"""
  vals = []
  for k in range(1, 400):
    c = F((k + 0.5) * scale)
    for _ in range(8):
      c = np.nextafter(c, F(0))
    for _ in range(16):
      b = c / F(scale)
      if int(b + F(0.5)) != int(float(c) / scale + 0.5) or int(b - F(0.5)) != int(float(c) / scale - 0.5):
        vals.append(c)
      c = np.nextafter(c, F(1e9))
  assert len(vals) >= 4 * n, len(vals)
  v = rng.permutation(np.asarray(vals, F))[:4 * n].reshape(n, 4)
  return np.stack([np.minimum(v[:, 0], v[:, 2]), np.minimum(v[:, 1], v[:, 3]),
                   np.maximum(v[:, 0], v[:, 2]), np.maximum(v[:, 1], v[:, 3])], 1).astype(F)


@pytest.mark.parametrize("kind", ["zero", "one", "half", "smooth", "noise", "rows"])
def test_op_boxes_and_masks(backend, kind):
  """Every edge case of the rectangle (1 x 1, downscale, full frame, each edge, clipped, outside) under every mask pattern."""
  name, lib = backend
  H, W = 45, 61
  rng = np.random.default_rng(len(kind))
  boxes = _edge_boxes(H, W)
  masks = _masks(kind, rng, len(boxes))
  rles, counts = ops.mask_rle(masks, boxes, (H, W), 1.0, want_counts=True, lib=lib)
  ex = check(rles, counts, boxes, masks, H, W)
  print("%s: %d pixels within %g of 0.5 excluded" % (kind, ex, NEAR))
  if kind == "zero":
    assert all(r["counts"] == rle_to_string([H * W]) for r in rles)
  if kind == "one":
    assert [int(x) for x in counts[2]] == [0, H * W]          # the full-frame box: one run of ones
    assert [int(x) for x in counts[10]] == [H * W]            # outside the frame
  if kind == "half":
    assert all(len(c) == 1 for c in counts)                   # exactly 0.5 is not > 0.5


def test_op_float32_rounding_of_the_rectangle(backend):
  """Coordinates whose float32 b +/- 0.5 rounds across an integer (float64 would give another rectangle), at scale != 1."""
  name, lib = backend
  rng = np.random.default_rng(5)
  H, W, scale = 50, 70, 0.37
  boxes = _round_across_boxes(rng, scale, 6)
  masks = _masks("smooth", rng, len(boxes))
  rles, counts = ops.mask_rle(masks, boxes, (H, W), scale, want_counts=True, lib=lib)
  check(rles, counts, boxes, masks, H, W, scale)


def test_op_transition_bound_tall_frame(backend):
  """The row-alternating mask stretched over a tall box: 27 crossings per column plus entry and exit -- close to the
  static bound of 32 per frame column -- and columns that run into each other across a full-height rectangle."""
  name, lib = backend
  H, W = 300, 24
  boxes = np.array([[0, 0, W, H], [2, 0, 20, H], [1, 0, 3, H]], F)
  masks = np.concatenate([_masks("rows", None, 2), _masks("one", None, 1)])
  rles, counts = ops.mask_rle(masks, boxes, (H, W), 1.0, want_counts=True, lib=lib)
  check(rles, counts, boxes, masks, H, W)
  assert len(counts[0]) - 1 == 28 * W - 1                     # 28 per column, the last one at the end of the frame


def test_op_zero_and_full_result_count(backend):
  """R = 0, and R = result_per_im (100) random detections; device inputs (on_device = 1) give the same result."""
  name, lib = backend
  assert ops.mask_rle(np.zeros((0, 28, 28), F), np.zeros((0, 4), F), (30, 40), 1.0, lib=lib) == []
  rng = np.random.default_rng(9)
  H, W, n = 72, 96, 100
  xy = rng.uniform(-4, [W, H], size=(n, 2))
  wh = rng.uniform(0.2, 40, size=(n, 2))
  boxes = np.concatenate([xy, xy + wh], 1).astype(F)
  masks = np.concatenate([_masks(k, rng, n // 4) for k in ("smooth", "noise", "rows", "one")])
  rles, counts = ops.mask_rle(masks, boxes, (H, W), 1.0, want_counts=True, lib=lib)
  ex = check(rles, counts, boxes, masks, H, W)
  print("R = 100: %d pixels within %g of 0.5 excluded" % (ex, NEAR))
  if name == "emu":         # the simulator's device memory is host memory
    keep = (np.ascontiguousarray(masks), np.ascontiguousarray(boxes))
    ptrs = (keep[0].ctypes.data, keep[1].ctypes.data, n)
  else:
    import torch
    keep = (torch.from_numpy(masks).cuda(), torch.from_numpy(boxes).cuda())
    torch.cuda.synchronize()
    ptrs = (keep[0].data_ptr(), keep[1].data_ptr(), n)
  rles2 = ops.mask_rle(None, None, (H, W), 1.0, device_ptrs=ptrs, lib=lib)
  assert rles2 == rles


def test_op_rejects_bad_arguments(backend):
  name, lib = backend
  m, b = np.zeros((1, 28, 28), F), np.array([[0, 0, 4, 4]], F)
  with pytest.raises(OdtError, match="scale"):
    ops.mask_rle(m, b, (10, 10), 0.0, lib=lib)
  with pytest.raises(OdtError, match="frame size"):
    ops.mask_rle(m, b, (0, 10), 1.0, lib=lib)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_mask_rle_kernels_use_no_scratch_memory():
  from test_kernel_resources import _resources
  res = _resources("mask_rle.hip")
  ks = {k: v for k, v in res.items() if "mask_rle_" in k}
  assert len(ks) == 2, sorted(res)
  for k, v in ks.items():
    assert v.get("scratch", 0) == 0, (k, v)


# ------------------------------------------------------------------------------------------- end to end

def _mask_cfg(name, **kw):
  small = dict(result_per_im=6, mrcnn_head_dim=64) if name == "emu" else {}   # simulator cost
  small.update(kw)
  return small_config(resnet_num_block=[1, 1, 1, 1], add_mask=True, rpn_test_post_nms_topk=32, **small)


def test_masks_rle_end_to_end(backend):
  """masks_rle of a forward = the restatement on that forward's final_masks and final_boxes / scale: through predict
  (frame of the plan's size, scale 1) and through predict_raw at another source size (device resize, scale != 1)."""
  name, lib = backend
  cfg = _mask_cfg(name)
  w = weights_for(cfg)
  m = models.get_model(cfg, 0, weights=w, lib=lib)
  try:
    fr = synthetic_frames(1, 96, 128)[0]
    boxes, labels, probs, feats = m.predict(fr)
    assert len(boxes) > 0
    rles, counts = m.masks_rle((96, 128), 1.0, want_counts=True)
    check(rles, counts, boxes, m.last_masks, 96, 128)
    assert m.masks_rle((96, 128), 1.0) == rles
    # a frame larger than the plan: 120 x 160 -> 96 x 128 on the device, boxes / 0.8 in the frame
    raw = synthetic_frames(1, 120, 160, seed=4)[0]
    out = m.predict_raw(raw, mask_rle=True)
    assert len(out) == 6 and len(m.predict_raw(raw)) == 5
    boxes2, scale, rles2 = out[0], out[4], out[5]
    assert scale != 1.0 and len(rles2) == len(boxes2) > 0
    e = m._last_forward[0]
    fm = e._masks[:len(boxes2)].copy()
    rles3, counts3 = m.masks_rle((120, 160), scale, want_counts=True)
    assert rles3 == rles2
    check(rles3, counts3, boxes2, fm, 120, 160, scale)
  finally:
    m.close()


def test_masks_rle_stale_and_without_mask_head(backend):
  """A second forward on the handle invalidates the first frame's call; a model without add_mask raises."""
  name, lib = backend
  cfg = _mask_cfg(name)
  m = models.get_model(cfg, 0, weights=weights_for(cfg), lib=lib)
  try:
    with pytest.raises(OdtError, match="no forward"):
      m.masks_rle((96, 128), 1.0)
    f1, f2 = synthetic_frames(2, 96, 128)
    m.predict(f1)
    e, s1 = m._last_forward
    first = m.masks_rle((96, 128), 1.0)
    assert e.mask_rle((96, 128), 1.0, serial=s1) == first
    m.predict(f2)
    with pytest.raises(OdtError, match="most recent"):
      e.mask_rle((96, 128), 1.0, serial=s1)
    assert e.forward_serial() == s1 + 1
    m.masks_rle((96, 128), 1.0)                               # the second frame's own call
  finally:
    m.close()
  cfg0 = small_config(resnet_num_block=[1, 1, 1, 1], rpn_test_post_nms_topk=32, **(dict(result_per_im=6) if name == "emu" else {}))
  m0 = models.get_model(cfg0, 0, weights=weights_for(cfg0), lib=lib)
  try:
    m0.predict(synthetic_frames(1, 96, 128)[0])
    with pytest.raises(OdtError, match="add_mask"):
      m0.masks_rle((96, 128), 1.0)
  finally:
    m0.close()


@pytest.mark.gpu
def test_masks_rle_1080p_result_per_im_100(hip_lib):
  """One 1080p frame through a plan of that size with result_per_im = 100."""
  cfg = small_config(resnet_num_block=[1, 1, 1, 1], add_mask=True, rpn_test_post_nms_topk=256, result_per_im=100,
                     max_size=1920, short_edge_size=1080)
  m = models.get_model(cfg, 0, weights=weights_for(cfg), lib=hip_lib)
  try:
    fr = synthetic_frames(1, 1080, 1920, seed=2)[0]
    boxes, labels, probs, feats = m.predict(fr)
    assert len(boxes) > 0
    rles, counts = m.masks_rle((1080, 1920), 1.0, want_counts=True)
    ex = check(rles, counts, boxes, m.last_masks, 1080, 1920)
    print("1080p: %d detections, %d pixels within %g of 0.5 excluded" % (len(boxes), ex, NEAR))
  finally:
    m.close()
