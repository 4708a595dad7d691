"""Op-level parity of the EfficientDet kernels (effnet.hip, effnet_mbconv.hip, effdet_post.hip) through the stand-alone
odt_op_* entry points, against plain float64 references (numpy / torch-CPU) or the oracle where the semantics are
TensorFlow's.

Exact-arithmetic cases use small-integer inputs, weights and biases: every f32 partial sum is then exact and the device
must equal the reference bit for bit, so a missing or misplaced tap fails outright.  Random-float cases bound the error
of each output by c * taps * eps * sum|x * w| (not by the tensor's max); swish / sigmoid outputs get a few ulp over the
float64 function of the exact pre-activation.  Pad channels of inputs are poisoned (NaN / 1e30) where a kernel must not
read them.  Every entry point checks the guard regions behind its buffers: a write past the end fails the call.
"""
import numpy as np
import pytest
import torch

from object_detection_tracking_amd import ops
from object_detection_tracking_amd._lib import OdtError
from oracle import effnet

F = np.float32
EPS = float(np.finfo(np.float32).eps)


def _ints(rng, shape, lo=-4, hi=4):
  return rng.integers(lo, hi + 1, size=shape).astype(F)


def _same(n, k, s):
  out = -(-n // s)
  tot = max((out - 1) * s + k - n, 0)
  return out, tot // 2


def _swish64(v):
  return v / (1.0 + np.exp(-v))


def _sigmoid64(v):
  return 1.0 / (1.0 + np.exp(-v))


def _ulps_ok(dev, ref64, n_ulp, floor=0.0):
  """|dev - ref| <= n_ulp ulp of the f32 reference (+ floor), elementwise."""
  r = ref64.astype(F)
  tol = n_ulp * np.spacing(np.abs(r)).astype(np.float64) + floor
  err = np.abs(dev.astype(np.float64) - ref64)
  return bool(np.all(err <= tol)), float((err / np.maximum(tol, 1e-45)).max())


# ----------------------------------------------------------------------------------------------------- depthwise

def dw_ref(x, wt, bias, k, s, pt, pl, Ho, Wo):
  """float64 depthwise conv: (pre-activation, sum of |x * w| + |bias| per output)."""
  B, H, W, C = x.shape
  Hp, Wp = max(pt + H, (Ho - 1) * s + k), max(pl + W, (Wo - 1) * s + k)
  xp = np.zeros((B, Hp, Wp, C)); xp[:, pt:pt + H, pl:pl + W] = x
  acc = np.zeros((B, Ho, Wo, C)); mag = np.zeros((B, Ho, Wo, C))
  w64 = wt.astype(np.float64)
  for ky in range(k):
    for kx in range(k):
      v = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] * w64[ky * k + kx]
      acc += v; mag += np.abs(v)
  b = bias.astype(np.float64)
  return acc + b, mag + np.abs(b)


def _dw_case(rng, B, H, W, ldc, k, s, ints=True, valid=None):
  x = _ints(rng, (B, H, W, ldc)) if ints else rng.standard_normal((B, H, W, ldc)).astype(F)
  wt = _ints(rng, (k * k, ldc)) if ints else rng.standard_normal((k * k, ldc)).astype(F)
  bias = _ints(rng, (ldc,)) if ints else rng.standard_normal(ldc).astype(F)
  if valid is not None:       # the plan's zero pad channels of weights and bias
    wt[:, valid:] = 0; bias[valid:] = 0
  Ho, pt = _same(H, k, s); Wo, pl = _same(W, k, s)
  return x, wt, bias, Ho, Wo, pt, pl


def _dw(lib, x, wt, bias, k, s, pt, pl, Ho, Wo, act=0, se_w=None, env=None, monkeypatch=None):
  for key in ("ODT_DW_PX", "ODT_DW_XCD", "ODT_DW_SUMCAP"):
    monkeypatch.delenv(key, raising=False)
  for key, v in (env or {}).items():
    monkeypatch.setenv(key, v)
  return ops.dwconv(x, wt, bias, k, s, pt, pl, (Ho, Wo), act=act, se_w=se_w, lib=lib)


# (k, stride, px): every template instance of dwconv_kernel
DW_VARIANTS = [(3, 1, 4), (3, 1, 8), (5, 1, 4), (5, 1, 8), (3, 2, 2), (5, 2, 2)]


@pytest.mark.parametrize("k,s,px", DW_VARIANTS)
@pytest.mark.parametrize("H,W", [(9, 13), (3, 3), (1, 1), (1, 7), (6, 11)])
def test_dwconv_exact_integers(backend, monkeypatch, k, s, px, H, W):
  """Small-integer operands: bit-exact with the float64 reference for every variant, Wo not a multiple of PX, Wo < PX,
  1x1 and 1xN maps, odd sizes at stride 2 (asymmetric SAME pads), 36 channels = 9 channel quads (not a multiple of 16)."""
  name, lib = backend
  rng = np.random.default_rng(k * 100 + s * 10 + H * 7 + W)
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 1, H, W, 36, k, s)
  out, info = _dw(lib, x, wt, bias, k, s, pt, pl, Ho, Wo, env={"ODT_DW_PX": str(px)} if s == 1 else None,
                  monkeypatch=monkeypatch)
  assert info["px"] == px, info
  ref, _ = dw_ref(x, wt, bias, k, s, pt, pl, Ho, Wo)
  assert np.array_equal(out, ref.astype(F)), float(np.abs(out - ref).max())
  # swish: a few ulp over the float64 swish of the exact pre-activation
  out2, _ = _dw(lib, x, wt, bias, k, s, pt, pl, Ho, Wo, act=2, env={"ODT_DW_PX": str(px)} if s == 1 else None,
                monkeypatch=monkeypatch)
  ok, worst = _ulps_ok(out2, _swish64(ref), 4, floor=1e-30)
  assert ok, worst


@pytest.mark.parametrize("k,s,px", DW_VARIANTS)
def test_dwconv_random_floats_bound_and_poisoned_pad(backend, monkeypatch, k, s, px):
  """Random floats, per-output bound 2 * (taps + 1) * eps * sum|x w|; pad channels of the input are NaN / 1e30 and must
  not leak into the valid ones; with zero input pads the pad outputs come out exactly 0 (what the 1x1 convs rely on)."""
  name, lib = backend
  rng = np.random.default_rng(7 + k + s + px)
  valid, ldc = 98, 100
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 1, 11, 10, ldc, k, s, ints=False, valid=valid)
  env = {"ODT_DW_PX": str(px)} if s == 1 else None
  ref, mag = dw_ref(x, wt, bias, k, s, pt, pl, Ho, Wo)
  x0 = x.copy(); x0[..., valid:] = 0
  out, info = _dw(lib, x0, wt, bias, k, s, pt, pl, Ho, Wo, env=env, monkeypatch=monkeypatch)
  assert info["px"] == px
  assert np.all(np.abs(out[..., :valid] - ref[..., :valid]) <= 2 * (k * k + 1) * EPS * mag[..., :valid])
  assert np.array_equal(out[..., valid:], np.zeros_like(out[..., valid:]))
  xp = x.copy(); xp[..., valid] = np.nan; xp[..., valid + 1] = 1e30
  outp, _ = _dw(lib, xp, wt, bias, k, s, pt, pl, Ho, Wo, env=env, monkeypatch=monkeypatch)
  assert np.array_equal(outp[..., :valid], out[..., :valid])


@pytest.mark.parametrize("k,s,px", DW_VARIANTS)
def test_dwconv_single_quad_xcd_off_batch1(backend, monkeypatch, k, s, px):
  """ldc = 4 (one channel quad in a 16-quad workgroup) at B = 1, XCD banding on and off: bit-exact both ways."""
  name, lib = backend
  rng = np.random.default_rng(40 + k + s + px)
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 1, 7, 10, 4, k, s)
  ref, _ = dw_ref(x, wt, bias, k, s, pt, pl, Ho, Wo)
  env = {"ODT_DW_PX": str(px)} if s == 1 else {}
  for xcd in ("1", "0"):
    out, info = _dw(lib, x, wt, bias, k, s, pt, pl, Ho, Wo, env=dict(env, ODT_DW_XCD=xcd), monkeypatch=monkeypatch)
    assert (info["px"], info["xcd_bands"], info["cqn"]) == (px, int(xcd), 16), info
    assert np.array_equal(out, ref.astype(F))


@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_px4_px8_and_xcd_bands_bit_identical(backend, monkeypatch, k):
  """PX 4 and 8 give the same bits (same tap order), and so do XCD banding on and off; B = 3 with a workgroup total
  that is not a multiple of 8."""
  name, lib = backend
  rng = np.random.default_rng(k)
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 3, 13, 21, 100, k, 1, ints=False)
  o8, i8 = _dw(lib, x, wt, bias, k, 1, pt, pl, Ho, Wo, act=2, monkeypatch=monkeypatch)
  o4, i4 = _dw(lib, x, wt, bias, k, 1, pt, pl, Ho, Wo, act=2, env={"ODT_DW_PX": "4"}, monkeypatch=monkeypatch)
  ox, ix = _dw(lib, x, wt, bias, k, 1, pt, pl, Ho, Wo, act=2, env={"ODT_DW_XCD": "0"}, monkeypatch=monkeypatch)
  assert (i8["px"], i4["px"]) == (8, 4)
  assert i8["xcd_bands"] == 1 and ix["xcd_bands"] == 0
  cblocks = -(-(100 // 4) // 16)
  assert (cblocks * i8["nsplit"] * 3) % 8 != 0, i8
  assert np.array_equal(o8, o4) and np.array_equal(o8, ox)
  for b in range(3):        # every image is its own: B = 1 calls give the same bits
    o1, _ = _dw(lib, x[b:b + 1], wt, bias, k, 1, pt, pl, Ho, Wo, act=2, monkeypatch=monkeypatch)
    assert np.array_equal(o1[0], o8[b])


def test_dwconv_multi_map_matches_single_maps(backend, monkeypatch):
  """The multi-map launch (5 maps, the smallest 1x1) equals 5 single-map calls bit for bit."""
  name, lib = backend
  for key in ("ODT_DW_PX", "ODT_DW_XCD", "ODT_DW_SUMCAP"):
    monkeypatch.delenv(key, raising=False)
  rng = np.random.default_rng(5)
  ldc = 68
  sizes = [(12, 17), (6, 9), (3, 5), (2, 3), (1, 1)]
  maps = [rng.standard_normal((h, w, ldc)).astype(F) for h, w in sizes]
  for k in (3, 5):
    wt = rng.standard_normal((k * k, ldc)).astype(F); bias = rng.standard_normal(ldc).astype(F)
    outs, info = ops.dwconv_maps(maps, wt, bias, k, act=2, lib=lib)
    for m, o in zip(maps, outs):
      single, _ = ops.dwconv(m[None], wt, bias, k, 1, k // 2, k // 2, m.shape[:2], act=2, lib=lib)
      assert np.array_equal(o, single[0])


def _se_weights(rng, ldc, mid, se, ints=False):
  g = (lambda s: _ints(rng, s, -2, 2) * F(0.25)) if ints else (lambda s: (rng.standard_normal(s) * 0.2).astype(F))
  w1 = g((se, ldc)); w2t = g((se, ldc)); b1 = g((se,)); b2 = g((mid,))
  w1[:, mid:] = 0; w2t[:, mid:] = 0
  return w1, b1, w2t, b2


def se_ref(mean64, mid, se_w):
  """float64 gate from a float64 mean, with a per-channel error bound for the device's f32 evaluation."""
  w1, b1, w2t, b2 = (a.astype(np.float64) for a in se_w)
  ldc = mean64.shape[-1]
  pre_r = mean64 @ w1.T + b1
  r = _swish64(pre_r)
  err_r = 1.2 * 3 * EPS * ldc * (np.abs(mean64) @ np.abs(w1).T + np.abs(b1)) + 4 * EPS * np.abs(r)
  s = r @ w2t[:, :mid] + b2
  err_s = 3 * EPS * w1.shape[0] * (np.abs(r) @ np.abs(w2t[:, :mid]) + np.abs(b2)) + err_r @ np.abs(w2t[:, :mid])
  g = _sigmoid64(s)
  return g, 0.25 * err_s + 4 * EPS * g + 1e-30


def _check_gate(gate, mean_dev, mid, se_w):
  g, tol = se_ref(mean_dev.astype(np.float64), mid, se_w)
  assert np.all(np.abs(gate[:, :mid] - g) <= tol), float((np.abs(gate[:, :mid] - g) / tol).max())
  assert np.array_equal(gate[:, mid:], np.zeros_like(gate[:, mid:])), "pad gates must be exactly 0"


@pytest.mark.parametrize("k,s,H,W,env,nsplit", [
    (3, 1, 5, 7, None, 1),                      # one split
    (5, 2, 23, 19, {"ODT_DW_SUMCAP": "9"}, 2),  # a small cap: cap // (cblocks * B) splits
    (3, 1, 40, 65, None, None),                 # several splits
])
def test_dwconv_fused_squeeze(backend, monkeypatch, k, s, H, W, env, nsplit):
  """The fused squeeze: the per-split sums folded into the mean bit-exact (integer outputs, sums < 2^24), the gate from
  the parts against float64 and equal to the gate of the activation path (launch_se_gate) on the same output."""
  name, lib = backend
  rng = np.random.default_rng(H * W + k)
  B, ldc, mid, se = 2, 72, 70, 6
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, B, H, W, ldc, k, s, valid=mid)
  se_w = _se_weights(rng, ldc, mid, se, ints=True)
  out, mean, gate, info = _dw(lib, x, wt, bias, k, s, pt, pl, Ho, Wo, se_w=se_w, env=env, monkeypatch=monkeypatch)
  if nsplit is not None:
    assert info["nsplit"] == nsplit, info
  else:
    assert info["nsplit"] > 1, info
  ref, _ = dw_ref(x, wt, bias, k, s, pt, pl, Ho, Wo)
  assert np.array_equal(out, ref.astype(F))
  sums = ref.sum(axis=(1, 2))
  assert np.abs(sums).max() < 2 ** 24
  assert np.array_equal(mean, (sums.astype(F) / F(Ho * Wo)).astype(F))
  _check_gate(gate, mean, mid, se_w)
  m2, g2, _, _ = ops.se_gate(out.reshape(B, Ho * Wo, ldc), mid, se_w, lib=lib)
  assert np.array_equal(m2, mean) and np.array_equal(g2, gate)


@pytest.mark.gpu
def test_dwconv_fused_squeeze_at_split_cap(hip_lib, monkeypatch):
  """nsplit at its 1024 cap (one channel block, one image, a 256 x 512 map)."""
  rng = np.random.default_rng(11)
  ldc, mid, se = 64, 64, 8
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 1, 256, 512, ldc, 3, 1)
  se_w = _se_weights(rng, ldc, mid, se, ints=True)
  out, mean, gate, info = _dw(hip_lib, x, wt, bias, 3, 1, pt, pl, Ho, Wo, se_w=se_w, monkeypatch=monkeypatch)
  assert info["nsplit"] == 1024, info
  ref, _ = dw_ref(x, wt, bias, 3, 1, pt, pl, Ho, Wo)
  assert np.array_equal(out, ref.astype(F))
  sums = ref.sum(axis=(1, 2))
  assert np.abs(sums).max() < 2 ** 24
  assert np.array_equal(mean, (sums.astype(F) / F(Ho * Wo)).astype(F))
  _check_gate(gate, mean, mid, se_w)


# ----------------------------------------------------------------------------------------------------- SE gate

@pytest.mark.parametrize("B,HW,ldc,mid,se", [(2, 37, 40, 36, 1), (1, 300, 96, 90, 24), (3, 4000, 64, 64, 4)])
def test_se_gate_and_channel_scale(backend, B, HW, ldc, mid, se):
  """launch_se_gate (channel sum -> fold -> reduce -> expand) + launch_channel_scale: HW below 64 (one split), several
  channel_mean_splits, a tiny se, mid < ldc (pad gates exactly 0).  Integer activations: the mean is exact."""
  name, lib = backend
  rng = np.random.default_rng(HW + ldc)
  x = _ints(rng, (B, HW, ldc)); x[..., mid:] = 0
  se_w = _se_weights(rng, ldc, mid, se)
  mean, gate, scaled, ns = ops.se_gate(x, mid, se_w, scale=True, lib=lib)
  assert (ns == 1) == (HW < 128), ns
  sums = x.astype(np.float64).sum(1)
  assert np.array_equal(mean, (sums.astype(F) / F(HW)).astype(F))
  _check_gate(gate, mean, mid, se_w)
  assert np.array_equal(scaled, x * gate[:, None, :])


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,ldc,mid,se", [(2, 49, 4096, 4090, 256), (1, 4096, 1040, 1040, 32)])
def test_se_gate_at_lds_limits_and_scale_past_grid_cap(hip_lib, B, HW, ldc, mid, se):
  """ldc 4096 / se 256 (the LDS staging limits) and a channel scale of 1 064 960 quads (past the 4096-workgroup grid)."""
  rng = np.random.default_rng(ldc)
  x = _ints(rng, (B, HW, ldc)); x[..., mid:] = 0
  se_w = _se_weights(rng, ldc, mid, se)
  mean, gate, scaled, _ = ops.se_gate(x, mid, se_w, scale=True, lib=hip_lib)
  assert np.array_equal(mean, (x.astype(np.float64).sum(1).astype(F) / F(HW)).astype(F))
  _check_gate(gate, mean, mid, se_w)
  assert np.array_equal(scaled, x * gate[:, None, :])


def test_se_gate_launchers_reject_lds_overflow(emu_lib, monkeypatch):
  """launch_se_gate (ldc > 4096) and launch_se_gate_from_parts (se > 256) refuse sizes their LDS staging cannot hold;
  the entry points leave that check to the launchers the plan uses."""
  rng = np.random.default_rng(0)
  with pytest.raises(OdtError, match="LDS"):
    ops.se_gate(np.zeros((1, 4, 4100), F), 4100, _se_weights(rng, 4100, 4100, 4), lib=emu_lib)
  x, wt, bias, Ho, Wo, pt, pl = _dw_case(rng, 1, 5, 5, 8, 3, 1)
  with pytest.raises(OdtError, match="LDS"):
    _dw(emu_lib, x, wt, bias, 3, 1, pt, pl, Ho, Wo, se_w=_se_weights(rng, 8, 8, 257), monkeypatch=monkeypatch)


# ----------------------------------------------------------------------------------------------------- BiFPN fuse

def _nchw(a):
  return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def _nhwc(t):
  return np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))


def fuse_ref(inputs, modes, h, w, wsm):
  """f32 in the kernel's operand order (exact where the terms are), as the graph combines them."""
  vals = []
  for a, m in zip(inputs, modes):
    if m == 0:
      v = a
    elif m == 1:
      v = _nhwc(effnet.nearest_resize(_nchw(a), h, w))
    else:
      v = _nhwc(effnet.max_pool_same_3x3_s2(_nchw(a)))
    vals.append(v.astype(F))
  if wsm is not None:
    wg = [F(max(x, 0.0)) for x in wsm]
    den = wg[0]
    for x in wg[1:]:
      den = F(den + x)
    den = F(den + F(1e-4))
    vals = [((v * wgt) / den).astype(F) for v, wgt in zip(vals, wg)]
  acc = vals[0]
  for v in vals[1:]:
    acc = (acc + v).astype(F)
  return acc


def _pool_pads(n):
  return max((-(-n // 2) - 1) * 2 + 3 - n, 0) // 2


@pytest.mark.parametrize("case", [
    # (out h, w), [(in h, w, mode)], 'fastattn' WSM scalars or None (plain sum)
    ((17, 13), [(9, 7, 1)], None),                                      # non-integer nearest ratios
    ((70, 9), [(35, 9, 1), (70, 9, 0)], None),
    ((9, 6), [(17, 11, 2)], None),                                      # odd inputs: pads 0 / 1
    ((8, 5), [(16, 10, 2), (8, 5, 0)], None),                           # even: pad 0
    ((9, 6), [(9, 6, 0), (17, 11, 2), (5, 3, 1)], [0.75, 0.5, 1.25]),   # all three modes, every input weighted
    ((9, 6), [(17, 11, 2), (9, 6, 0)], [1.5, -2.0]),                    # weighted pool, the relu clamps the other
    ((12, 12), [(12, 12, 0), (12, 12, 0), (6, 6, 1)], [-0.25, 1.5, 0.75]),
])
@pytest.mark.parametrize("act", [0, 2])
def test_bifpn_fuse(backend, case, act):
  """Each mode alone and mixed, n = 1 / 2 / 3, plain and weighted sums, B = 2, swish: bit-exact on integer inputs
  against oracle.effnet.nearest_resize / max_pool_same_3x3_s2 (act 0), a few ulp of the float64 swish (act 2)."""
  name, lib = backend
  (h, w), spec, wsm = case
  rng = np.random.default_rng(h * 31 + w + len(spec))
  B, ldc = 2, 20
  ins = [_ints(rng, (B, ih, iw, ldc), -8, 8) for ih, iw, _ in spec]
  modes = [m for _, _, m in spec]
  pads = [(_pool_pads(ih), _pool_pads(iw)) if m == 2 else (0, 0) for ih, iw, m in spec]
  out = ops.bifpn_fuse(ins, modes, (h, w), pads=pads, wsm=wsm, act=act, lib=lib)
  ref = fuse_ref(ins, modes, h, w, wsm)
  if act == 0:
    assert np.array_equal(out, ref), float(np.abs(out - ref).max())
  else:
    ok, worst = _ulps_ok(out, _swish64(ref.astype(np.float64)), 4, floor=1e-30)
    assert ok, worst


@pytest.mark.gpu
def test_bifpn_fuse_past_grid_cap(hip_lib):
  """B * h * w * ldc / 4 = 1 310 720 quads, past the 4096 x 256 threads of the capped grid: the grid-stride loop of
  bifpn_fuse_kernel runs (two iterations for most threads)."""
  rng = np.random.default_rng(3)
  B, h, w, ldc = 2, 128, 160, 128
  assert B * h * w * ldc // 4 > 4096 * 256
  ins = [_ints(rng, (B, h, w, ldc)), _ints(rng, (B, 2 * h - 1, 2 * w - 1, ldc)), _ints(rng, (B, 67, 80, ldc))]
  modes = [0, 2, 1]
  pads = [(0, 0), (_pool_pads(2 * h - 1), _pool_pads(2 * w - 1)), (0, 0)]
  out = ops.bifpn_fuse(ins, modes, (h, w), pads=pads, lib=hip_lib)
  assert np.array_equal(out, fuse_ref(ins, modes, h, w, None))


# ----------------------------------------------------------------------------------------------------- MBConv

def mb_ref(x, e_wt, e_bias, dw_wt, dw_bias, k, s, pt, pl, Ho, Wo, lmid):
  """float64 expand 1x1 + swish -> depthwise + swish; returns (out, bound on |device - out|)."""
  B, H, W, _ = x.shape
  mid = e_wt.shape[0]
  e = np.einsum("bhwc,mc->bhwm", x.astype(np.float64), e_wt.astype(np.float64)) + e_bias
  assert np.all(np.abs(e) < 2 ** 20) and np.all(e == np.round(e))     # integer GEMM: exact in the bf16x3 pieces
  ex = np.zeros((B, H, W, lmid)); ex[..., :mid] = _swish64(e)
  pre, mag = dw_ref(ex, dw_wt, dw_bias, k, s, pt, pl, Ho, Wo)
  # mb_swish is within ~3 ulp of each expanded value, the stencil rounds each of its k*k fused multiply-adds
  err_pre = (k * k + 4) * 2 * EPS * mag
  return _swish64(pre), 1.1 * err_pre + 4 * EPS * np.abs(_swish64(pre)) + 1e-30


@pytest.mark.parametrize("k,s,H,W,in_ldc,lmid", [(3, 1, 5, 7, 32, 64), (5, 1, 18, 30, 64, 64), (3, 2, 20, 17, 96, 128),
                                                 (5, 2, 9, 33, 64, 192), (3, 1, 17, 18, 128, 128)])
def test_mbconv_expand_dw(backend, monkeypatch, k, s, H, W, in_ldc, lmid):
  """The fused MBConv front half: maps smaller than one 16 x 16 patch and tiles cut by the border on both axes, against
  float64 (integer expand GEMM: exact in bf16 pieces) and against odt_op_conv2d + odt_op_dwconv (the two launches it
  replaces); several input and expanded widths; the squeeze mean per channel against the float64 mean of the fused
  output, bounded by the depth of the kernel's summation, and the gate from it."""
  name, lib = backend
  for key in ("ODT_DW_PX", "ODT_DW_XCD", "ODT_DW_SUMCAP"):
    monkeypatch.delenv(key, raising=False)
  rng = np.random.default_rng(k * 1000 + H * W)
  B, mid, se = 2, lmid - 4, 5
  cin = in_ldc - 2
  x = _ints(rng, (B, H, W, in_ldc), -2, 2); x[..., cin:] = 0
  e_wt = _ints(rng, (mid, in_ldc), -2, 2); e_wt[:, cin:] = 0
  e_bias = _ints(rng, (mid,), -2, 2)
  dw_wt = (rng.standard_normal((k * k, lmid)) * 0.3).astype(F); dw_wt[:, mid:] = 0
  dw_bias = (rng.standard_normal(lmid) * 0.1).astype(F); dw_bias[mid:] = 0
  Ho, pt = _same(H, k, s); Wo, pl = _same(W, k, s)
  se_w = _se_weights(rng, lmid, mid, se)
  out, mean, gate, nsplit = ops.mbconv_expand_dw(x, e_wt, e_bias, dw_wt, dw_bias, k, s, pt, pl, (Ho, Wo), se_w=se_w,
                                                 lib=lib)
  assert nsplit >= 1
  ref, tol = mb_ref(x, e_wt, e_bias, dw_wt, dw_bias, k, s, pt, pl, Ho, Wo, lmid)
  assert np.all(np.abs(out - ref) <= tol), float((np.abs(out - ref) / tol).max())
  assert np.array_equal(out[..., mid:], np.zeros_like(out[..., mid:]))
  # the unfused pair: expand on the conv kernels (swish epilogue), then the stand-alone depthwise kernel
  w_hwio = np.zeros((1, 1, in_ldc, lmid), F); w_hwio[0, 0, :, :mid] = e_wt.T
  eb = np.zeros(lmid, F); eb[:mid] = e_bias
  ex = ops.conv2d(x, w_hwio, eb, relu=2, lib=lib)
  two, _ = ops.dwconv(ex, dw_wt, dw_bias, k, s, pt, pl, (Ho, Wo), act=2, lib=lib)
  assert np.all(np.abs(out - two) <= 2 * tol)
  # squeeze: per thread its outputs in walk order (tiles of its range x slots, up to two outputs per slot step), a fixed
  # tree over the 16 slots, the splits folded in 4 phases; one rounding per addition along that chain
  HW = Ho * Wo
  to = (16 - k) // s + 1
  tiles = -(-Ho // to) * -(-Wo // to)
  depth = 2 * -(-tiles // nsplit) * -(-(to * to) // 16) + 16 + nsplit + 4
  o64 = out.astype(np.float64).reshape(B, HW, lmid)
  want, mag = o64.sum(1) / HW, np.abs(o64).sum(1) / HW
  assert np.all(np.abs(mean - want) <= depth * EPS * mag + np.spacing(np.abs(want.astype(F)))), \
      float(np.abs(mean - want).max())
  m2, g2, _, ns = ops.se_gate(out.reshape(B, HW, lmid), mid, se_w, lib=lib)
  assert np.all(np.abs(m2 - want) <= (-(-HW // 16) + 16 + ns + 4) * EPS * mag + np.spacing(np.abs(want.astype(F))))
  _check_gate(gate, mean, mid, se_w)


# ----------------------------------------------------------------------------------------------------- detection tail

def _tail_inputs(rng, npix, ncls, B, ldc_cls, ldc_box, logits=None):
  """Per-level class / box tensors with NaN / 1e30 in the pad lanes, distinct anchors."""
  cls, box = [], []
  nanch = 9 * sum(npix)
  flat = logits if logits is not None else rng.standard_normal((B, nanch * ncls)).astype(F) * F(3)
  off = 0
  for n in npix:
    c = np.full((B, n, ldc_cls), np.nan, F); c[..., 9 * ncls + 1:] = F(1e30)
    c[..., :9 * ncls] = flat[:, off:off + n * 9 * ncls].reshape(B, n, 9 * ncls)
    off += n * 9 * ncls
    bx = np.full((B, n, ldc_box), np.nan, F)
    bx[..., :36] = (rng.standard_normal((B, n, 36)) * 0.3).astype(F)
    cls.append(c); box.append(bx)
  yc = rng.uniform(0, 200, nanch); xc = rng.uniform(0, 300, nanch)
  hh = rng.uniform(4, 60, nanch); ww = rng.uniform(4, 60, nanch)
  anchors = np.stack([yc - hh / 2, xc - ww / 2, yc + hh / 2, xc + ww / 2], 1).astype(F)
  return cls, box, anchors, flat


def _decode(box_all, anchors, idx):
  """oracle.effnet.detect's decode (float32) for the anchors idx."""
  a = anchors[idx]; rel = box_all[idx]
  yc_a = (a[:, 0] + a[:, 2]) / F(2); xc_a = (a[:, 1] + a[:, 3]) / F(2)
  ha = a[:, 2] - a[:, 0]; wa = a[:, 3] - a[:, 1]
  wd = np.exp(rel[:, 3]) * wa; h = np.exp(rel[:, 2]) * ha
  yc = rel[:, 0] * ha + yc_a; xc = rel[:, 1] * wa + xc_a
  return np.stack([yc - h / F(2), xc - wd / F(2), yc + h / F(2), xc + wd / F(2)], 1).astype(F), \
      np.abs(yc) + np.abs(xc) + np.abs(h) + np.abs(wd)


def _check_tail(r, cls, box, anchors, flat, npix, ncls, k, max_out, score_thr, iou, scale):
  B = flat.shape[0]
  lvl_of_anchor = np.concatenate([np.full(9 * n, l + 3, np.int32) for l, n in enumerate(npix)])
  for b in range(B):
    order = np.lexsort((np.arange(flat.shape[1]), -flat[b].astype(np.float64)))[:k]
    assert np.array_equal(r["cand_idx"][b], order), "top-k indices differ (image %d)" % b
    anc, cl = order // ncls, order % ncls
    assert np.array_equal(r["cand_cls"][b], cl) and np.array_equal(r["cand_lvl"][b], lvl_of_anchor[anc])
    ok, worst = _ulps_ok(r["cand_scores"][b], _sigmoid64(flat[b][order].astype(np.float64)), 3, floor=1e-38)
    assert ok, ("scores", worst)
    box_all = np.concatenate([bx[b, :, :36].reshape(-1, 4) for bx in box], 0)
    want, mag = _decode(box_all, anchors, anc)
    assert np.all(np.abs(r["cand_boxes"][b] - want) <= 8 * EPS * mag[:, None]), "decoded boxes"
    # NMS on the device's own candidates: the keep list bit-exact
    keep = effnet.nms_with_scores(r["cand_boxes"][b], r["cand_scores"][b], max_out, iou, score_thr)
    n = len(keep)
    assert r["valid"][b] == n, (r["valid"][b], n)
    cb = r["cand_boxes"][b][keep] * F(scale)
    assert np.array_equal(r["boxes"][b, :n], np.stack([cb[:, 1], cb[:, 0], cb[:, 3], cb[:, 2]], 1))
    assert np.array_equal(r["scores"][b, :n], r["cand_scores"][b][keep])
    assert np.array_equal(r["labels"][b, :n], r["cand_cls"][b][keep] + 1)
    assert np.array_equal(r["levels"][b, :n], r["cand_lvl"][b][keep])
    # padding rows: zero box, score 0, label 0, level 3
    assert np.all(r["boxes"][b, n:] == 0) and np.all(r["scores"][b, n:] == 0)
    assert np.all(r["labels"][b, n:] == 0) and np.all(r["levels"][b, n:] == 3)


NPIX = [64, 16, 4, 4, 1]        # 89 cells, 801 anchors


@pytest.mark.parametrize("case", ["distinct", "plateau", "signed_zero", "all_equal"])
def test_effdet_tail_topk_ties(backend, case):
  """Top-k bit-exact against np.lexsort (value desc, index asc): distinct logits, a k-th logit shared by hundreds of
  entries straddling the level-0 / level-1 boundary (the index passes of the radix select run), -0.0 / +0.0 at the
  threshold (sortable_key folds them: equal values, index order), all logits equal; non-power-of-two k."""
  name, lib = backend
  rng = np.random.default_rng(len(case))
  ncls = 7
  nlog = 9 * sum(NPIX) * ncls
  flat = (rng.standard_normal((1, nlog)) * 3).astype(F)
  boundary = 9 * NPIX[0] * ncls
  k = 300
  if case == "plateau":
    flat[0, boundary - 200:boundary + 200] = F(0.5)
    k = int((flat[0] > 0.5).sum()) + 150
  elif case == "signed_zero":
    flat[0] = np.where(flat[0] > 0, flat[0], F(-5))
    z = rng.permutation(np.arange(boundary - 300, boundary + 300))[:400]
    flat[0, z[:200]] = F(0.0); flat[0, z[200:]] = F(-0.0)
    k = int((flat[0] > 0).sum()) + 211
  elif case == "all_equal":
    flat[0] = F(1.5)
  cls, box, anchors, flat = _tail_inputs(rng, NPIX, ncls, 1, 9 * ncls + 3, 40, logits=flat)
  r = ops.effdet_post(cls, box, anchors, ncls, k, 100, score_thresh=0.0, lib=lib)
  _check_tail(r, cls, box, anchors, flat, NPIX, ncls, k, 100, 0.0, 0.5, 1.0)


@pytest.mark.parametrize("k,max_out,score_thr,scale,ncls", [
    (None, 1, 0.0, 1.0, 5),           # k = ntot, one detection
    (8192, 1024, 0.3, 1.0, 12),       # the sort cap, max_out cap, a threshold that cuts mid-list
    (1000, 800, 0.9, 2.5, 3),         # max_out above the survivors: padding rows; image_scale != 1
])
def test_effdet_tail_caps_threshold_scale(backend, k, max_out, score_thr, scale, ncls):
  name, lib = backend
  rng = np.random.default_rng(ncls)
  npix = NPIX if ncls != 5 else [9, 4, 1, 1, 1]
  cls, box, anchors, flat = _tail_inputs(rng, npix, ncls, 1, 9 * ncls + 4, 37)
  k = k or flat.shape[1]
  assert k <= flat.shape[1]
  r = ops.effdet_post(cls, box, anchors, ncls, k, max_out, score_thresh=score_thr, image_scale=scale, lib=lib)
  _check_tail(r, cls, box, anchors, flat, npix, ncls, k, max_out, score_thr, 0.5, scale)
  if score_thr > 0:
    assert 0 < int((r["cand_scores"][0] > score_thr).sum()) < k
  if max_out == 800:
    assert r["valid"][0] < max_out


def test_effdet_tail_batch_images_independent(backend):
  """B = 3 images with different content (one all-equal): each equals its own B = 1 run and its own reference -- the
  keys, state and hist scratch reused per image carry nothing over."""
  name, lib = backend
  rng = np.random.default_rng(33)
  ncls = 4
  nlog = 9 * sum(NPIX) * ncls
  flat = (rng.standard_normal((3, nlog)) * 3).astype(F)
  flat[1] = F(0.25)
  flat[2, :nlog // 2] = F(-9)
  cls, box, anchors, flat = _tail_inputs(rng, NPIX, ncls, 3, 9 * ncls + 2, 36, logits=flat)
  r = ops.effdet_post(cls, box, anchors, ncls, 400, 50, score_thresh=0.1, lib=lib)
  _check_tail(r, cls, box, anchors, flat, NPIX, ncls, 400, 50, 0.1, 0.5, 1.0)
  for b in range(3):
    r1 = ops.effdet_post([c[b:b + 1] for c in cls], [x[b:b + 1] for x in box], anchors, ncls, 400, 50, score_thresh=0.1,
                         lib=lib)
    for key in r:
      assert np.array_equal(r1[key][0], r[key][b]), (b, key)


@pytest.mark.gpu
def test_effdet_tail_d0_512_past_pack_grid_cap(hip_lib):
  """EfficientDet-D0 @ 512: 49 104 anchors x 90 classes (eff_pack_kernel's grid-stride loop), k = 5000, B = 2."""
  rng = np.random.default_rng(512)
  npix = [64 * 64, 32 * 32, 16 * 16, 8 * 8, 4 * 4]
  cls, box, anchors, flat = _tail_inputs(rng, npix, 90, 2, 816, 36)
  r = ops.effdet_post(cls, box, anchors, 90, 5000, 100, score_thresh=0.0, lib=hip_lib)
  _check_tail(r, cls, box, anchors, flat, npix, 90, 5000, 100, 0.0, 0.5, 1.0)


# ----------------------------------------------------------------------------------------------------- preprocess

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_preprocess_rgb(backend, dtype):
  """launch_preprocess_rgb against oracle.effnet.preprocess: bit-exact (same operation order), u8 and f32 frames, the
  stem's SAME pads and a padded right edge zero in all four channels."""
  name, lib = backend
  rng = np.random.default_rng(1)
  fr = rng.integers(0, 256, size=(2, 13, 18, 3)).astype(dtype)
  if dtype == np.float32:
    fr = fr + rng.uniform(0, 1, size=fr.shape).astype(F)
  out = ops.preprocess_rgb(fr, 0, 1, 14, 26, lib=lib)
  ref = effnet.preprocess(fr).numpy().transpose(0, 2, 3, 1)
  assert np.array_equal(out[:, :13, 1:19, :3], ref)
  inside = np.zeros(out.shape[:3], bool); inside[:, :13, 1:19] = True
  assert np.all(out[..., 3] == 0) and np.all(out[~inside] == 0)


@pytest.mark.parametrize("src,dst", [((37, 50), (24, 32)), ((19, 23), (40, 48)), ((30, 17), (30, 40))])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_preprocess_rgb_resize(backend, src, dst, dtype):
  """launch_preprocess_rgb_resize against oracle.effnet.preprocess_resized, down- and up-scaling: bit-exact (the
  kernel interpolates the normalised corners in the oracle's operation order)."""
  name, lib = backend
  rng = np.random.default_rng(src[0] * dst[1])
  fr = rng.integers(0, 256, size=(1,) + src + (3,)).astype(dtype)
  ref, _ = effnet.preprocess_resized(fr[0], dst)
  ref = ref.numpy()[0].transpose(1, 2, 0)
  sc = min(F(dst[1]) / F(src[1]), F(dst[0]) / F(src[0]))
  sh, sw = int(F(src[0]) * sc), int(F(src[1]) * sc)
  out = ops.preprocess_rgb(fr, 0, 0, dst[0], dst[1], resize_hw=(sh, sw), lib=lib)
  assert np.array_equal(out[0, ..., :3], ref), float(np.abs(out[0, ..., :3] - ref).max())
  assert np.all(out[..., 3] == 0)
