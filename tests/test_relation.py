"""Relation-network box heads (--add_relation_nn; reference relation_network nn.py:115-190, geometric_encoding nn.py:273-298,
from models.py:1044-1054): end to end against the oracle running the literal head (relation_reference.relation_oracle: torch,
float64 inside the head), and the two kernels of csrc/relation.hip on their own against float64 evaluations, exact data and the
softmax's invariances.

Tolerances: trunk taps 2e-5 of the tensor maximum, boxes 1e-3 px, scores 1e-4, appearance features 10x the tap tolerance,
mismatch budget 0; the relation taps and the attention op relation_reference.TAP_TOL (its docstring says how it was arrived at).
The geometric bias ends in log(max(relu(a), 1e-6)), which divides an error of a by a: _geo_allowed states the bound.
96 x 128 frames, blocks [1, 1, 1, 1], 32 proposals, the real head width 1024."""
import numpy as np
import pytest
import torch

import relation_reference as R
from common import small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights

F = np.float32
K = 32


def _cfg(**kw):
  base = dict(add_relation_nn=True, resnet_num_block=[1, 1, 1, 1], rpn_test_post_nms_topk=K)
  base.update(kw)
  return small_config(**base)


def _cfg_dim(dim, **kw):
  cfg = _cfg(**kw)
  cfg.fpn_frcnn_fc_head_dim = dim
  return cfg


# ------------------------------------------------------------------------------------------------- end to end

def _check_shapes(m, e, d0, d, out, fr, ref):
  for x in (d0, d):
    assert x["box_head"] == "2fc+relation" and x["relation_modules"] == 2, x
  assert e.tap("rm_r1").shape == (1, 1, K, 1024) and e.tap("rm_r2_attn").shape == (1, 1, K, 16 * 1024)


def test_relation_forward_single(backend):
  """RM_r1 / RM_r2 on the single-image graph: detections, the four relation taps, and what describe() says.  Fails on a tree
  without the feature: get_model raises NotImplementedError."""
  name, lib = backend
  R.run_single(lib, _cfg(), 96, 128, check=_check_shapes)


def test_relation_class_agnostic(backend):
  name, lib = backend
  R.run_single(lib, _cfg(use_frcnn_class_agnostic=True), 96, 128, check=_check_shapes)


def test_relation_with_group_norm(backend):
  """use_gn with the 2-FC head and the relation modules: the normalisation stops in front of the head."""
  name, lib = backend

  def check(m, e, d0, d, out, fr, ref):
    _check_shapes(m, e, d0, d, out, fr, ref)
    assert d["use_gn"] == 1 and d["group_norms"] == 25 and d["roi_group_norms"] == 0, d

  R.run_single(lib, _cfg(use_gn=True), 96, 128, check=check)


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_relation_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test.  "auto" ends on
  fp16x2 with a healthy guard.  (At 32 proposals no layer of the head has the 256 rows the fp16x2 kernels want: whether
  output_linear runs on them behind the attention kernel's range record shows at 300 / 1000 proposals, tools/bench_backbones.py.)"""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]

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

  R.run_single(lib, _cfg(**kw), 96, 128, check=check)


def test_relation_two_forwards_bit_identical(backend):
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


def test_relation_padded_rows(backend):
  """A frame with fewer proposals than K: the padded rows of the attention outputs are exactly zero, every tap is finite, and
  the real rows agree with the literal module.  (The standard synthetic frames fill all 32 rows; a flat frame leaves 30.)"""
  name, lib = backend
  cfg = _cfg()
  w = R.weights(cfg)
  frame = np.full((96, 128, 3), 110, np.uint8)
  m = models.get_model(R._with_taps(cfg), 0, weights=w, lib=lib)
  try:
    out = m.predict(frame)
    e = m.engine(1, 96, 128)
    n, rec = R.check_relation_taps(e, cfg, w)
    assert 0 < n < K, n
    for t in ("fc6", "fc7", "rm_r1", "rm_r2", "rm_r1_attn", "rm_r2_attn", "head_out"):
      assert np.isfinite(e.tap(t)).all(), t
    assert not e.tap("rm_r1_attn").reshape(K, -1)[n:].any() and not e.tap("rm_r2_attn").reshape(K, -1)[n:].any()
    assert len(out[0]) > 0 and all(np.isfinite(np.asarray(x, np.float64)).all() for x in out[:4])
  finally:
    m.close()


# ------------------------------------------------------------------------------------------------- op level

def _boxes(n, rng):
  """n boxes with w, h in [1, 500] px inside a 1080p frame; from the third on, box 2 repeats box 0 (|dx| = |dy| = 0 hits the 1e-3
  floor and the size ratios are 1) and box 3 shares box 1's centre at another size."""
  w = rng.uniform(1.0, 500.0, n); h = rng.uniform(1.0, 500.0, n)
  cx = rng.uniform(0.0, 1920.0, n); cy = rng.uniform(0.0, 1080.0, n)
  b = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], 1).astype(F)
  if n > 2:
    b[2] = b[0]
  if n > 3:
    c = 0.5 * (b[1, :2] + b[1, 2:])
    b[3] = np.concatenate([c - F(8.0), c + F(8.0)])
  return b


def _geo_weights(rng):
  return ((rng.standard_normal((4, 64)) * 0.5).astype(F), (rng.standard_normal(64) * 0.1).astype(F)), \
         ((rng.standard_normal((1, 1, 64, 16)) * 0.25).astype(F), (rng.standard_normal(16) * 0.1).astype(F))


def _geo_allowed(a_ref, geo_conv):
  """Bound on |bias - bias64| for an f32 evaluation.  a[h] = b[h] + sum_k g_k Wc[k,h] with |g| <= 1: 65 f32 operations on partial
  sums below S_h = |b[h]| + sum_k |Wc[k,h]| err by at most 65 * 2^-24 * S_h; g itself carries the error of its argument (four
  products of |e| <= 8 with |We| < 2.5, a sum of five terms: < 2e-6, and tanh' <= 1) plus tanhf's few ulp: 3e-6, times sum_k |Wc|.
  log(max(relu(a), 1e-6)) turns an error da of a into at most da / max(a, 1e-6) (to first order; a factor 2 covers the rest for
  da < a / 2, and where a is smaller than that every value between the floor and log(a + da) is as right as the other).  On top,
  logf's ulp at |bias| <= 13.9: 2e-6."""
  S = np.abs(np.asarray(geo_conv[1], np.float64)) + np.abs(np.asarray(geo_conv[0], np.float64).reshape(64, 16)).sum(0)      # [16]
  da = (65 * 2.0 ** -24 + 3e-6) * S                                                                                          # [16]
  return 2e-6 + 2.0 * da[None, None, :] / np.maximum(a_ref, 1e-6)


@pytest.mark.parametrize("n,Kk", [(1, 1), (2, 2), (17, 17), (64, 64), (65, 65), (17, 32)])
def test_relation_geo_against_float64(backend, n, Kk):
  """The geometric bias against the float64 restatement; padded boxes are NaN and the entries they would touch come back as they
  went in (a sentinel), those with i, j < n unaffected."""
  name, lib = backend
  rng = np.random.default_rng(100 + n + Kk)
  boxes = np.full((Kk, 4), np.nan, F)
  boxes[:n] = _boxes(n, rng)
  ge, gc = _geo_weights(rng)
  Kp = (Kk + 3) // 4 * 4
  init = np.full((16, Kk, Kp), 777.0, F)
  got = ops.relation_geo(boxes, n, ge, gc, bias_init=init, lib=lib)
  with torch.no_grad():
    ref, a = R.geometric_bias(boxes[:n], ge, gc)
  ref = ref.numpy().transpose(1, 0, 2); a = a.numpy()                # bias [16,n,n], a [n,n,16]
  assert np.isfinite(got[:, :n, :n]).all()
  err = np.abs(got[:, :n, :n].astype(np.float64) - ref)
  allowed = _geo_allowed(a, gc).transpose(2, 0, 1)
  print("relation_geo n=%d K=%d: max err %.3g, max err / allowed %.3g, share of relu(a) > 0 %.2f" %
        (n, Kk, err.max(), (err / allowed).max(), (a > 0).mean()))
  assert (err <= allowed).all(), float((err / allowed).max())
  # where a is well away from zero the bound is a tight one: the kernel is not hiding behind the floor
  far = (a.transpose(2, 0, 1) > 0.05)
  if far.any():
    assert err[far].max() < 2e-3, err[far].max()
  rest = np.ones_like(got, bool); rest[:, :n, :n] = False
  assert (got[rest] == F(777.0)).all()
  if n >= 4:
    # box 2 is box 0: the two rows see the same geometry
    assert np.array_equal(got[:, 0, :n], got[:, 2, :n])


ATT_SHAPES = [(1, 1, 64), (2, 4, 64), (17, 32, 256), (64, 64, 1024), (65, 96, 1024), (0, 8, 64)]


def _att_inputs(n, Kk, D, rng, pad=np.nan):
  """q, k with logits of a few units, v ~ N(0,1), a bias with the module's floor in it; rows / entries past n hold `pad`."""
  dh = D // 16
  q = np.full((Kk, D), pad, F); k = np.full((Kk, D), pad, F); v = np.full((Kk, D), pad, F)
  q[:n] = rng.standard_normal((n, D)) * 1.2; k[:n] = rng.standard_normal((n, D)) * 1.2; v[:n] = rng.standard_normal((n, D))
  Kp = (Kk + 3) // 4 * 4
  bias = np.full((16, Kk, Kp), pad, F)
  b = np.log(np.maximum(rng.standard_normal((16, n, n)), 1e-6))
  bias[:, :n, :n] = b
  return q, k, v, bias


def _att_ref(q, k, v, bias, n):
  with torch.no_grad():
    o, p = R.attention(q[:n], k[:n], v[:n], bias[:, :n, :n].transpose(1, 0, 2))
  return o.numpy(), p.numpy()


def _rel(a, b):
  return float(np.abs(a - b).max() / max(1e-6, np.abs(b).max()))


@pytest.mark.parametrize("n,Kk,D", ATT_SHAPES)
def test_relation_attention_against_float64(backend, n, Kk, D):
  """Rows < n within tolerance of float64, rows >= n exactly zero, nothing written past [K,16,D] (a sentinel behind it), padded
  rows of q, k, v and padded bias entries NaN; the recorded |max| is max |out| bit for bit."""
  name, lib = backend
  rng = np.random.default_rng(7 * n + Kk + D)
  q, k, v, bias = _att_inputs(n, Kk, D, rng)
  size = Kk * 16 * D
  init = np.full(size + 4096, 31337.0, F)
  flat, amax = ops.relation_attention(q, k, v, bias, n, out_init=init, lib=lib)
  assert (flat[size:] == F(31337.0)).all(), "written past [K,16,D]"
  out = flat[:size].reshape(Kk, 16, D)
  assert np.isfinite(out).all()
  assert not out[n:].any(), "rows >= n are not zero"
  assert amax == float(np.abs(out).max())
  if n > 0:
    ref, p = _att_ref(q, k, v, bias, n)
    err = _rel(out[:n].astype(np.float64), ref)
    print("relation_attention n=%d K=%d D=%d: rel err %.3g, median max_j P %.3f" % (n, Kk, D, err, np.median(p.max(-1))))
    assert err < R.TAP_TOL, err


@pytest.mark.parametrize("n", [1, 2, 4, 64])
def test_relation_attention_exact_case(backend, n):
  """q = 0 and a bias that is constant along j: every softmax row is 1 / n exactly, and with small integers in v every output
  is the column mean of v bit for bit."""
  name, lib = backend
  rng = np.random.default_rng(n)
  D = 128
  q = np.zeros((n, D), F); k = rng.standard_normal((n, D)).astype(F)
  v = rng.integers(-8, 9, (n, D)).astype(F)
  Kp = (n + 3) // 4 * 4
  bias = np.zeros((16, n, Kp), F)
  bias[:, :, :] = rng.standard_normal((16, n, 1)).astype(F)
  out, amax = ops.relation_attention(q, k, v, bias, n, lib=lib)
  mean = (v.sum(0) / F(n)).astype(F)
  assert np.array_equal(out, np.broadcast_to(mean, (n, 16, D)))


def test_relation_attention_bias_shift(backend):
  """softmax is shift-invariant: a constant added to bias[h, i, :] leaves the result within tolerance."""
  name, lib = backend
  rng = np.random.default_rng(5)
  n, Kk, D = 17, 20, 128
  q, k, v, bias = _att_inputs(n, Kk, D, rng, pad=0.0)
  a, _ = ops.relation_attention(q, k, v, bias, n, lib=lib)
  shifted = bias + rng.uniform(-5.0, 5.0, (16, Kk, 1)).astype(F)
  b, _ = ops.relation_attention(q, k, v, shifted, n, lib=lib)
  assert _rel(b.astype(np.float64), a.astype(np.float64)) < R.TAP_TOL


def test_relation_attention_large_logit(backend):
  """One logit of 1e4 in a row: the maximum is subtracted before exp, so the row's output is that column's v and nothing is NaN."""
  name, lib = backend
  rng = np.random.default_rng(6)
  n, D = 9, 64
  q, k, v, bias = _att_inputs(n, n, D, rng, pad=0.0)
  col = rng.integers(0, n, (16, n))
  for h in range(16):
    for i in range(n):
      bias[h, i, col[h, i]] = 1e4
  out, _ = ops.relation_attention(q, k, v, bias, n, lib=lib)
  assert np.isfinite(out).all()
  want = v[col.T]                                    # [n,16,D]
  assert np.array_equal(out, want)


def test_relation_attention_permutation(backend):
  """Permuting the proposals permutes the output rows (another summation order: within tolerance)."""
  name, lib = backend
  rng = np.random.default_rng(8)
  n, D = 19, 128
  q, k, v, bias = _att_inputs(n, n, D, rng, pad=0.0)
  a, _ = ops.relation_attention(q, k, v, bias, n, lib=lib)
  perm = rng.permutation(n)
  pb = np.zeros_like(bias)
  pb[:, :n, :n] = bias[:, perm][:, :, perm]
  b, _ = ops.relation_attention(q[perm], k[perm], v[perm], pb, n, lib=lib)
  assert _rel(b.astype(np.float64), a[perm].astype(np.float64)) < R.TAP_TOL


def test_relation_ops_reject_bad_arguments(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  lib = emu_lib
  rng = np.random.default_rng(0)
  ge, gc = _geo_weights(rng)
  with pytest.raises(OdtError, match=r"at most 1024 proposals \(K = 1028\)"):
    ops.relation_geo(np.ones((1028, 4), F), 4, ge, gc, lib=lib)
  with pytest.raises(OdtError, match=r"n = 9 is not in \[0, K = 8\]"):
    ops.relation_geo(np.ones((8, 4), F), 9, ge, gc, lib=lib)
  z = lambda Kk, D: (np.zeros((Kk, D), F), np.zeros((Kk, D), F), np.zeros((Kk, D), F), np.zeros((16, Kk, (Kk + 3) // 4 * 4), F))
  with pytest.raises(OdtError, match=r"at most 1024 proposals \(K = 1028\)"):
    ops.relation_attention(*z(1028, 64), 4, out_init=np.zeros(1028 * 16 * 64, F), lib=lib)
  with pytest.raises(OdtError, match=r"D must be a multiple of 64 in \[64, 1024\] \(D = 96\)"):
    ops.relation_attention(*z(8, 96), 4, lib=lib)
  with pytest.raises(OdtError, match=r"\(D = 1088\)"):
    ops.relation_attention(*z(8, 1088), 4, lib=lib)
  with pytest.raises(OdtError, match=r"n = 9 is not in \[0, K = 8\]"):
    ops.relation_attention(*z(8, 64), 9, lib=lib)


# ------------------------------------------------------------------------------------------------- weights

def test_relation_synthetic_weights():
  """synthetic_weights under the flag draws exactly relation_variables(cfg) on top of an otherwise bit-identical dict."""
  from object_detection_tracking_amd.weights import relation_variables
  cfg = _cfg_dim(128)
  base_cfg = _cfg_dim(128, add_relation_nn=False)
  w = synthetic_weights(cfg, 3)
  base = synthetic_weights(base_cfg, 3)
  names = relation_variables(cfg)
  assert len(names) == 14 and len(set(names)) == 14 and relation_variables(base_cfg) == []
  assert names[0] == "fastrcnn/RM_r1/geo_emb/W" and names[-1] == "fastrcnn/RM_r2/output_linear/W"
  assert set(w) - set(base) == set(names) and set(base) <= set(w)
  for k, v in base.items():
    assert np.array_equal(v, w[k]), k
  for s in ("fastrcnn/RM_r1", "fastrcnn/RM_r2"):
    assert w[s + "/geo_emb/W"].shape == (4, 64) and w[s + "/geo_emb/b"].shape == (64,)
    assert w[s + "/geo_conv/W"].shape == (1, 1, 64, 16) and w[s + "/geo_conv/b"].shape == (16,)
    assert w[s + "/query_linear/W"].shape == (128, 128) and w[s + "/key_linear/W"].shape == (128, 128)
    assert w[s + "/output_linear/W"].shape == (16 * 128, 128)
  assert not np.array_equal(w["fastrcnn/RM_r1/geo_emb/W"], w["fastrcnn/RM_r2/geo_emb/W"])
  assert all(v.dtype == np.float32 for v in w.values())


def test_relation_weights_survive_the_writers(tmp_path):
  """The RM variables come back from every writer / reader pair of the repository (.npz, TF checkpoint, frozen .pb), and
  config_from_weights reads the flag off fastrcnn/RM_r1/query_linear/W.  D = 64: output_linear/W is 64 MB at 1024."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz, relation_variables
  cfg = _cfg_dim(64)
  w = synthetic_weights(cfg, 0)
  np.savez(str(tmp_path / "r.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-3"), w)
  write_frozen_pb(str(tmp_path / "r.pb"), w)
  for got in (load_npz(str(tmp_path / "r.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "r.pb"))):
    assert set(got) >= set(w)
    for k in relation_variables(cfg):
      assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "r.pb")))
  assert c.add_relation_nn and c.fpn_frcnn_fc_head_dim == 64 and not c.use_conv_frcnn_head
  c = models.config_from_weights(synthetic_weights(_cfg_dim(64, add_relation_nn=False), 0))
  assert not c.add_relation_nn


# ------------------------------------------------------------------------------------------------- errors

def test_relation_errors(emu_lib, monkeypatch):
  from object_detection_tracking_amd._lib import OdtError
  cfg = _cfg()
  w = R.weights(cfg)
  plain = {k: v for k, v in w.items() if "/RM_r" not in k}
  with pytest.raises(NotImplementedError, match=r"add_relation_nn\) cannot be built from weights without its variables: missing "
                                                r"fastrcnn/RM_r1/geo_emb/W, fastrcnn/RM_r1/geo_emb/b"):
    models.get_model(cfg, 0, weights=plain, lib=emu_lib)
  part = {k: v for k, v in w.items() if k != "fastrcnn/RM_r2/key_linear/W"}
  with pytest.raises(NotImplementedError, match=r"missing fastrcnn/RM_r2/key_linear/W$"):
    models.get_model(cfg, 0, weights=part, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="add_relation_nn together with use_conv_frcnn_head"):
    models.get_model(_cfg(use_conv_frcnn_head=True), 0, weights=w, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="add_relation_nn is built for the single-image graph"):
    models.get_model(_cfg(im_batch_size=2), 0, weights=w, lib=emu_lib, is_multi=True)
  with pytest.raises(NotImplementedError, match="rpn_test_post_nms_topk = 1025"):
    models.get_model(_cfg(rpn_test_post_nms_topk=1025), 0, weights=w, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="use_att_frcnn_head"):
    models.get_model(_cfg(add_relation_nn=False, use_att_frcnn_head=True), 0, weights=plain, lib=emu_lib)
  with pytest.raises(NotImplementedError, match="use_att_frcnn_head"):
    models.get_model(_cfg(use_att_frcnn_head=True), 0, weights=w, lib=emu_lib)
  # the library's own messages: a variable that is there in another shape
  bad = dict(w); bad["fastrcnn/RM_r2/geo_conv/W"] = bad["fastrcnn/RM_r2/geo_conv/W"][..., :8]
  m = models.get_model(cfg, 0, weights=bad, lib=emu_lib)
  try:
    with pytest.raises(OdtError, match=r"bad shape for fastrcnn/RM_r2/geo_conv/W \(\[1,1,64,16\]"):
      m.engine(1, 96, 128)
    m.weights = dict(w); m.weights["fastrcnn/RM_r1/output_linear/W"] = w["fastrcnn/RM_r1/output_linear/W"][:64]
    with pytest.raises(OdtError, match=r"bad shape for fastrcnn/RM_r1/output_linear/W \(\[16 D,D\] with D = 1024\)"):
      m.engine(1, 96, 128)
  finally:
    m.close()
  # finalize_config pins fpn_frcnn_fc_head_dim to the reference's 1024; a config that reaches get_model with another width (a
  # caller with a finalize of its own) is refused by number
  monkeypatch.setattr(models, "finalize_config", lambda c: c)
  for dim in (96, 2048):
    with pytest.raises(NotImplementedError, match="add_relation_nn with fpn_frcnn_fc_head_dim = %d" % dim):
      models.get_model(_cfg_dim(dim), 0, weights=w, lib=emu_lib)


def test_relation_builds_with_basic_blocks_and_mask_head(backend):
  """The head is independent of the backbone and of the mask head: a basic-block backbone builds and runs, on the GPU with
  --add_mask on top (the simulator takes a minute and a half for the mask head's convs)."""
  name, lib = backend
  kw = dict(use_basic_block=True, add_mask=(name == "hip"))
  fr = synthetic_frames(1, 96, 128)
  w = synthetic_weights(_cfg(add_relation_nn=False, **kw), 0)
  w.update({k: v for k, v in R.weights(_cfg()).items() if "/RM_r" in k})
  m = models.get_model(_cfg(**kw), 0, weights=w, lib=lib)
  try:
    out = m.predict(fr[0])
    assert len(out[0]) > 0 and m.engine(1, 96, 128).describe()["box_head"] == "2fc+relation"
    assert all(np.isfinite(np.asarray(x, np.float64)).all() for x in out[:4])
  finally:
    m.close()
