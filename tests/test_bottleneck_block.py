"""conv_block_kernel (csrc/conv_block.hip): a whole stride-1 identity bottleneck in one launch, at the op level
(odt_op_bottleneck_block), against an f64 reference and against the three launches it replaces.

Error measure, as in test_bottleneck_tail_fused_vs_f64: |got - ref| divided by the magnitude propagated through the block,
mag = |w3| . (|w2| * (|w1| . |x| + |b1|) + |b2|) + |b3| + |x|.  The reference rounds both intermediate tensors to f32, as
every path stores or splits them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from object_detection_tracking_amd import ops

F = np.float32
C = 64

SHAPES = [
    (1, 16, 16),      # one whole tile
    (1, 19, 27),      # partial tiles in y and x
    (2, 9, 17),       # two images, every tile partial, patch halo on all four image borders
    (1, 33, 20),      # three tile rows
]


def _weights(rng, b1_positive=False):
  w1 = (rng.standard_normal((4 * C, C)) * np.sqrt(2.0 / (4 * C))).astype(F)
  w2 = (rng.standard_normal((3, 3, C, C)) * np.sqrt(2.0 / (9 * C))).astype(F)
  w3 = (rng.standard_normal((C, 4 * C)) * np.sqrt(2.0 / C)).astype(F)
  b1 = (rng.standard_normal(C) * 0.1).astype(F)
  if b1_positive:
    b1 = (np.abs(b1) + F(0.5)).astype(F)
  b2 = (rng.standard_normal(C) * 0.1).astype(F)
  b3 = (rng.standard_normal(4 * C) * 0.1).astype(F)
  return w1, b1, w2, b2, w3, b3


def _input(rng, B, H, W):
  # post-ReLU block input with a log-normal spread over pixels
  return (np.maximum(rng.standard_normal((B, H, W, 4 * C)), 0) * np.exp(rng.standard_normal((B, H, W, 1)))).astype(F)


def _ref(x, w1, b1, w2, b2, w3, b3, pad_value=None):
  """f64 block and its propagated magnitude, NHWC.  pad_value: what conv2 sees outside the image in place of zero, per channel
  (the wrong block of test (c))."""
  d = lambda a: torch.from_numpy(np.asarray(a)).double()
  xt = d(x)
  t1 = (torch.einsum("bhwk,kc->bhwc", xt, d(w1)) + d(b1)).relu().float().double()
  m1 = torch.einsum("bhwk,kc->bhwc", xt.abs(), d(w1).abs()) + d(b1).abs()
  w2t = d(w2).permute(3, 2, 0, 1)

  def conv3x3(t, w, pad):
    t = t.permute(0, 3, 1, 2)
    if pad is None:
      t = TF.pad(t, (1, 1, 1, 1))
    else:
      B, Cc, H, W = t.shape
      full = pad.view(1, Cc, 1, 1).expand(B, Cc, H + 2, W + 2).clone()
      full[:, :, 1:-1, 1:-1] = t
      t = full
    return TF.conv2d(t, w).permute(0, 2, 3, 1)

  t2 = (conv3x3(t1, w2t, None if pad_value is None else d(pad_value)) + d(b2)).relu().float().double()
  m2 = conv3x3(m1, w2t.abs(), None) + d(b2).abs()
  z = (torch.einsum("bhwc,cn->bhwn", t2, d(w3)) + d(b3) + xt).relu()
  mag = torch.einsum("bhwc,cn->bhwn", m2, d(w3).abs()) + d(b3).abs() + xt.abs()
  return z.numpy(), mag.numpy()


_CACHE = {}


def _case(shape):
  """inputs, weights and the f64 reference of a shape: computed once, shared, never modified"""
  if shape not in _CACHE:
    B, H, W = shape
    rng = np.random.default_rng(B * 10000 + H * 100 + W)
    x = _input(rng, B, H, W)
    wts = _weights(rng)
    ref, mag = _ref(x, *wts)
    for a in (x, ref, mag) + wts:
      a.setflags(write=False)
    _CACHE[shape] = (x, wts, ref, mag)
  return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_bottleneck_block_fused_vs_f64(backend, shape):
  """(a) the one-launch block against f64 within 1.5 x the three launches' own maximum error on the same inputs + 1.2e-7
  (test_conv2d_split_matches_f32_kernel_at_f32_rounding's rule), the three launches alone under the tail test's 4e-7;
  (b) the two forms agree within the same margin."""
  name, lib = backend
  x, wts, ref, mag = _case(shape)
  got = {}
  for f in (False, True):
    got[f] = ops.bottleneck_block(x, *wts, fuse=f, lib=lib)
    # the record odt_op_bottleneck_block launched last: conv_block_kernel runs conv2's fused-tail record | conv3's own launch
    got_row = ops.last_conv(lib)
    assert (got_row["name"], got_row["splitk"]) == (("H2KF_256x64", 1) if f else ("H2_256x256", 1)), got_row
  e0 = float((np.abs(got[False] - ref) / mag).max())
  e1 = float((np.abs(got[True] - ref) / mag).max())
  d01 = float((np.abs(got[True] - got[False]) / mag).max())
  print("bottleneck_block %s %s: three launches %.3e, one launch %.3e, between them %.3e" % (name, shape, e0, e1, d01))
  assert e0 < 4e-7, e0
  bound = 1.5 * e0 + 1.2e-7
  assert e1 <= bound, (e1, bound)
  assert d01 <= bound, (d01, bound)


def test_bottleneck_block_zero_padding(backend):
  """(c) conv2 pads conv1's OUTPUT with zeros.  With a positive conv1 bias a patch pixel outside the image would hold
  relu(bias1) > 0 if conv1 were simply run on a zero-padded x: the block built that way differs from the true one at the image
  border by far more than the tolerance (asserted first), and the kernel matches the true one there."""
  name, lib = backend
  B, H, W = 2, 9, 17
  rng = np.random.default_rng(917)
  x = _input(rng, B, H, W)
  wts = _weights(rng, b1_positive=True)
  ref, mag = _ref(x, *wts)
  wrong, _ = _ref(x, *wts, pad_value=np.maximum(wts[1], 0))
  border = np.zeros((B, H, W, 1), bool)
  border[:, 0] = border[:, -1] = border[:, :, 0] = border[:, :, -1] = True
  tol = 4e-7
  sep = np.abs(wrong - ref) / mag
  assert float(sep[np.broadcast_to(border, sep.shape)].max()) > 1e3 * tol      # the construction separates the two paddings ...
  for yx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0)):
    assert float(sep[:, yx[0], yx[1]].max()) > 1e3 * tol, yx                     # ... on every side and corner
  assert float(sep[:, 1:-1, 1:-1].max()) == 0.0
  got = ops.bottleneck_block(x, *wts, fuse=True, lib=lib)
  err = np.abs(got - ref) / mag
  e0 = float((np.abs(ops.bottleneck_block(x, *wts, fuse=False, lib=lib) - ref) / mag).max())
  print("bottleneck_block zero padding %s: one launch %.3e, three launches %.3e" % (name, float(err.max()), e0))
  assert e0 < tol
  assert float(err.max()) <= 1.5 * e0 + 1.2e-7, float(err.max())


def test_bottleneck_block_tile_scale(backend):
  """(d) conv2's operand gets its power of two per 16 x 16 TILE, from the tile's own 18 x 18 patch of conv1's output: with the
  image rows scaled from 2^0 down to 2^-14, every 16-row band keeps the fp16x2 error level relative to ITS OWN magnitude
  (the largest propagated magnitude inside the band -- the pieces carry 2^-22 of the tile's maximum, so an element far below
  its tile's maximum is held to the band, not to itself), while the band magnitudes themselves fall by 2^-5 per band.
  Bound: the tail tests' 4e-7."""
  name, lib = backend
  B, H, W = 1, 45, 16
  rng = np.random.default_rng(4516)
  x = (np.maximum(rng.standard_normal((B, H, W, 4 * C)), 0) + F(0.01)).astype(F)
  for r in range(H):
    x[0, r] *= F(2.0 ** (-14.0 * r / (H - 1)))
  w1, b1, w2, b2, w3, b3 = _weights(rng)
  b1 = np.zeros_like(b1); b2 = np.zeros_like(b2); b3 = np.zeros_like(b3)      # magnitudes scale with the rows
  ref, mag = _ref(x, w1, b1, w2, b2, w3, b3)
  got = ops.bottleneck_block(x, w1, b1, w2, b2, w3, b3, fuse=True, lib=lib)
  err = np.abs(got - ref)
  for y0 in range(0, H, 16):
    band = slice(y0, min(y0 + 16, H))
    e = float(err[0, band].max() / mag[0, band].max())
    print("bottleneck_block tile scale %s rows %d..: %.3e of the band's magnitude %.3e" % (name, y0, e, float(mag[0, band].max())))
    assert e < 4e-7, (y0, e)
  assert float(mag[0, 32:].max()) < 2.0 ** -9 * float(mag[0, :16].max())        # the bands really are far apart
