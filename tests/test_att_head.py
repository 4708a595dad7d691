"""Attention box heads (--use_att_frcnn_head; reference fastrcnn_2fc_head, models.py:1064-1089 / :2682-2707): end to end against
the oracle running the literal branch (att_head_reference.att_oracle: conv, softmax over the last axis, product, reduce_sum,
dense + ReLU, add) behind the 2-FC, the 4conv1fc + GroupNorm and the relation heads, on both graphs; the fact the design rests on
-- the reference's attention map is exactly 1 -- on the literal restatement alone; and the two kernels of csrc/att_head.hip on
their own.

Tolerances are the project's own (test_conv_head.py): trunk and head taps 2e-5 of the tensor maximum, boxes 1e-3 px, scores 1e-4,
appearance features 10x the trunk tolerance, mismatch budget 0.  The head taps are held to their 2e-5 against the literal head
evaluated on the engine's own RoI features (conv_head_reference.check_head_taps says why).  96 x 128 frames, blocks [1, 1, 1, 1],
32 proposals, conv_frcnn_head_dim = 64.

att_pool is held bit for bit to a numpy loop that adds the 49 positions one after another in float32, and to the bound of
sequential summation against float64, |s - s64| <= 48 u sum|x| with u = 2^-24 (48 additions that round; the first, to +0, is
exact) -- a bound of the number format, not of the kernel: the numpy loop sits at about 0.04 of it on normal data."""
import numpy as np
import pytest
import torch

import att_head_reference as A
from common import small_config
from object_detection_tracking_amd import models, ops
from object_detection_tracking_amd.weights import att_head_variables, synthetic_frames, synthetic_weights
from test_e2e import _with_taps

F = np.float32
K = 32
U = 2.0 ** -24


def _cfg(**kw):
  base = dict(use_att_frcnn_head=True, conv_frcnn_head_dim=64, resnet_num_block=[1, 1, 1, 1], rpn_test_post_nms_topk=K)
  base.update(kw)
  return small_config(**base)


# ------------------------------------------------------------------------------------------------- end to end

def test_att_head_forward_single(backend):
  """The branch behind the 2-FC head on the single-image graph: detections, the fc7 / att_pool / att_trans / att_hidden taps, and
  what describe() says -- the floor bytes worked out by hand for K = 32.  Fails on a tree without the feature: get_model raises
  NotImplementedError."""
  name, lib = backend
  cfg = _cfg()

  def check(m, e, d0, d, out, fr, ref):
    for x in (d0, d):
      assert x["box_head"] == "2fc" and x["att_frcnn_head"] == 1, x
      # roi_feat [32,49,256] read + [32,256] written; fc7 and att_trans [32,1024] read + att_hidden written
      assert x["att_head_floor_bytes"] == 4 * 32 * 49 * 256 + 4 * 32 * 256 + 3 * 4 * 32 * 1024 == 2031616, x
      assert x["att_head_profiled_ms"] == [0.0, 0.0, 0.0], x
    assert e.tap("att_pool").shape == (1, 1, K, 256) and e.tap("att_trans").shape == (1, 1, K, 1024)
    assert e.tap("att_hidden").shape == (1, 1, K, 1024)
    # the pooled tensor is the plain sum of the RoI features, in the kernel's order, bit for bit
    roi = e.tap("roi_feat").reshape(K, 49, 256)
    assert np.array_equal(e.tap("att_pool").reshape(K, 256), _seq_sum(roi))

  A.run_single(lib, cfg, 96, 128, check=check)


def test_att_head_conv_gn_forward_single(backend):
  """Behind the 4conv1fc head under use_gn: hidden is fastrcnn/fc's output."""
  name, lib = backend
  cfg = _cfg(use_conv_frcnn_head=True, use_gn=True)

  def check(m, e, d0, d, out, fr, ref):
    for x in (d0, d):
      assert x["box_head"] == "4conv1fc" and x["roi_group_norms"] == 4 and x["att_frcnn_head"] == 1, x

  A.run_single(lib, cfg, 96, 128, check=check)


def test_att_head_relation_forward_single(backend):
  """Behind RM_r2 under add_relation_nn (single graph, as that head is)."""
  name, lib = backend
  cfg = _cfg(add_relation_nn=True)

  def check(m, e, d0, d, out, fr, ref):
    for x in (d0, d):
      assert x["box_head"] == "2fc+relation" and x["relation_modules"] == 2 and x["att_frcnn_head"] == 1, x

  A.run_single(lib, cfg, 96, 128, check=check)


def test_att_head_forward_multi(backend):
  """The batched graph at b = 2; each image -- its trunk taps, its rows of the head taps, its detections -- is bit-identical at
  either position of the batch, and the two images differ."""
  from block_reference import check_batch_swap
  name, lib = backend
  cfg = _cfg(im_batch_size=2)
  swap = check_batch_swap(["c2", "c5", "p2", "p5"])

  def check(m, e, d0, d, out, fr):
    a = {t: e.tap(t).copy() for t in ("fc7", "att_pool", "att_trans", "att_hidden")}
    swap(m, e, d0, d, out, fr)                       # (leaves the engine on the swapped batch)
    for t, x in a.items():
      x = x.reshape(2, K, -1)
      y = e.tap(t).reshape(x.shape)
      assert not np.array_equal(x[0], x[1]), t
      assert np.array_equal(x[0], y[1]) and np.array_equal(x[1], y[0]), t

  A.run_multi(lib, cfg, 2, 96, 128, check=check)


@pytest.mark.parametrize("mode", ["f32", "split3", "auto"])
def test_att_head_arithmetic_modes(backend, mode):
  """conv_arith = "f32", conv_split_family = 3 and the guarded default pass the checks of the default test; "auto" ends on fp16x2
  with one passed check of a healthy guard.  Behind the 4conv1fc + GroupNorm head, whose convs over 32 x 49 RoI pixels are the
  only layers of a 32-proposal head with the rows the fp16x2 kernels want: att_trans and fastrcnn/outputs have 32 rows here and
  run on the exact-f32 kernel whatever their inputs' range slots hold.  That the two kernels record what they store is asserted
  bit for bit at the op level (amax, below); that att_trans takes the fp16x2 kernels behind att_pool's record shows at 300 / 1000
  proposals (tools/bench_backbones.py prints the fp16x2 launch counts of r101 and r101_att; profiles/att_head_b8_1080p.txt)."""
  name, lib = backend
  kw = {"f32": dict(conv_arith="f32"), "split3": dict(conv_split_family=3), "auto": dict(conv_split_family="auto")}[mode]
  cfg = _cfg(use_conv_frcnn_head=True, use_gn=True, **kw)

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

  A.run_single(lib, cfg, 96, 128, check=check)


def test_att_head_partial_classes(backend):
  """The branch is independent of the output layers' class subset: version 2 (no dilations), 81 classes reduced to seven by
  --use_partial_classes."""
  name, lib = backend
  names = ["BG"] + ["c%d" % i for i in range(1, 81)]
  cfg = _cfg(version=2, use_dilations=False, num_class=81, is_coco_model=True, use_partial_classes=True,
             partial_classes=["c1", "c3", "c4", "c6", "c8", "c17", "c80"], classname2id={n: i for i, n in enumerate(names)})
  out = A.run_single(lib, cfg, 96, 128)
  assert out[1].min() >= 1 and out[1].max() <= 7


@pytest.mark.gpu
def test_att_head_mask_head_gpu(hip_lib):
  """... and of the mask head (--add_mask; on the GPU alone: the simulator takes a minute and a half for the mask head's convs)."""
  def check(m, e, d0, d, out, fr, ref):
    masks = m.last_masks
    assert masks.shape == (len(out[0]), 28, 28) and np.isfinite(masks).all() and masks.max() > 0

  A.run_single(hip_lib, _cfg(add_mask=True), 96, 128, check=check)


def test_att_head_two_forwards_bit_identical(backend):
  name, lib = backend
  cfg = _cfg()
  fr = synthetic_frames(1, 96, 128)
  m = models.get_model(cfg, 0, weights=A.weights(cfg), lib=lib)
  try:
    a = m.predict(fr[0]); b = m.predict(fr[0])
    assert len(a[0]) > 0
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  finally:
    m.close()


def test_att_head_branch_is_live(backend):
  """Control: the same weights with the flag off give the same fc7 bit for bit -- the branch changes nothing in front of it --
  while att_hidden differs from fc7 and the class scores move."""
  name, lib = backend
  cfg = _cfg()
  w = A.weights(cfg)
  fr = synthetic_frames(1, 96, 128)
  taps = {}
  for flag in (True, False):
    m = models.get_model(_with_taps(_cfg(use_att_frcnn_head=flag)), 0, weights=w, lib=lib)
    try:
      m.predict(fr[0])
      e = m.engine(1, 96, 128)
      taps[flag] = {t: e.tap(t).copy() for t in (("fc7", "head_out", "att_hidden", "att_trans") if flag else ("fc7", "head_out"))}
      assert e.describe()["att_frcnn_head"] == int(flag)
      if not flag:
        with pytest.raises(Exception, match="att_hidden"):
          e.tap("att_hidden")
    finally:
      m.close()
  on, off = taps[True], taps[False]
  assert np.array_equal(on["fc7"], off["fc7"])
  assert on["att_trans"].max() > 0 and not np.array_equal(on["att_hidden"], on["fc7"])
  n_cls = cfg.num_class
  moved = np.abs(on["head_out"][..., :n_cls] - off["head_out"][..., :n_cls]).max()
  print("class logits moved by up to %.3g (|max| %.3g)" % (moved, np.abs(off["head_out"][..., :n_cls]).max()))
  assert moved > 1e-2 * np.abs(off["head_out"][..., :n_cls]).max()


# ------------------------------------------------------------------------------------------------- the reference's map is 1

@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3, 1e15, 1e30])
def test_reference_attention_map_is_one(scale):
  """The literal restatement in float32 on random features: whatever the size of attention/W, every weight of the map is exactly
  1.0 and `attended` is torch.sum of the plain feature, bit for bit."""
  g = torch.Generator().manual_seed(int(np.log10(scale)) + 40)
  feature = torch.randn(6, 7, 7, 64, generator=g)
  W = torch.randn(3, 3, 64, 1, generator=g) * scale
  b = torch.randn(1, generator=g)
  with torch.no_grad():
    a, att = A.attended(feature, W, b)
    logits = torch.nn.functional.conv2d(feature.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1).contiguous(), b, padding=1)
  assert torch.isfinite(logits).all() and float(logits.abs().max()) > 0.5 * scale
  assert att.shape == (6, 7, 7, 1) and att.dtype == torch.float32
  assert np.array_equal(att.numpy(), np.ones((6, 7, 7, 1), F))
  assert np.array_equal(a.numpy(), torch.sum(feature.reshape(6, 49, 64), 1).numpy())


def test_reference_attention_map_of_a_non_finite_logit_is_nan():
  """The one deviation: an infinite logit -- an infinite attention/W here -- gives NaN in the reference's map and
  NaN rows in `attended`, where this path sums the plain feature.  get_model refuses such weights."""
  g = torch.Generator().manual_seed(7)
  feature = torch.randn(2, 7, 7, 8, generator=g)
  W = torch.randn(3, 3, 8, 1, generator=g)
  W[1, 1, 0, 0] = float("inf")
  with torch.no_grad():
    a, att = A.attended(feature, W, torch.zeros(1))
  assert torch.isnan(att).all() and torch.isnan(a).all()
  for l in (1e30, -3.4e38, 0.0, 1e-45):
    assert float(torch.softmax(torch.tensor([l], dtype=torch.float32), dim=-1)[0]) == 1.0
  for l in (float("inf"), float("-inf"), float("nan")):
    assert torch.isnan(torch.softmax(torch.tensor([l], dtype=torch.float32), dim=-1)[0])


# ------------------------------------------------------------------------------------------------- errors

def test_att_head_errors(emu_lib):
  from object_detection_tracking_amd._lib import OdtError
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  # the class-agnostic head of the reference has no such branch (models.py:1126): set by hand, and by version
  for kw in (dict(use_frcnn_class_agnostic=True), dict(version=5)):
    c = _cfg(**kw)
    with pytest.raises(NotImplementedError, match=r"use_att_frcnn_head together with use_frcnn_class_agnostic .*the reference's "
                                                  r"class-agnostic head has no attention branch"):
      models.get_model(c, 0, weights=synthetic_weights(c, 0), lib=emu_lib)
  for n in att_head_variables(cfg):
    with pytest.raises(NotImplementedError, match=r"use_att_frcnn_head\) cannot be built from weights without its variables: missing " + n + "$"):
      models.get_model(cfg, 0, weights={k: v for k, v in w.items() if k != n}, lib=emu_lib)
  bad = dict(w); bad["fastrcnn/att_trans/W"] = bad["fastrcnn/att_trans/W"][:, :512]
  with pytest.raises(ValueError, match=r"bad shape for fastrcnn/att_trans/W: \[256, 512\], the graph has \[256, 1024\]"):
    models.get_model(cfg, 0, weights=bad, lib=emu_lib)
  bad = dict(w); bad["fastrcnn/attention/W"] = bad["fastrcnn/attention/W"][:, :, :, [0, 0]]
  with pytest.raises(ValueError, match=r"bad shape for fastrcnn/attention/W: \[3, 3, 256, 2\], the graph has \[3, 3, 256, 1\]"):
    models.get_model(cfg, 0, weights=bad, lib=emu_lib)
  bad = dict(w); bad["fastrcnn/attention/W"] = bad["fastrcnn/attention/W"].copy(); bad["fastrcnn/attention/W"][2, 0, 17, 0] = np.nan
  with pytest.raises(ValueError, match="fastrcnn/attention/W holds a non-finite value"):
    models.get_model(cfg, 0, weights=bad, lib=emu_lib)
  # the library's own messages, behind get_model's checks: the plan does not build
  m = models.get_model(cfg, 0, weights=w, lib=emu_lib)
  try:
    m.weights = {k: v for k, v in w.items() if k != "fastrcnn/attention/b"}
    with pytest.raises(OdtError, match=r"missing attention box head variable fastrcnn/attention/b \(odt_config.use_att_frcnn_head\)"):
      m.engine(1, 96, 128)
    m.weights = dict(w); m.weights["fastrcnn/att_trans/b"] = w["fastrcnn/att_trans/b"][:512]
    with pytest.raises(OdtError, match=r"bad shape for fastrcnn/att_trans/b \(\[1024\]\)"):
      m.engine(1, 96, 128)
    m.weights = dict(w); m.weights["fastrcnn/attention/b"] = np.array([np.inf], F)
    with pytest.raises(OdtError, match="fastrcnn/attention/b holds a non-finite value"):
      m.engine(1, 96, 128)
  finally:
    m.close()
  # what stays refused, as before (use_small_object_head, the other name of that list, is forced off by finalize_config as by
  # every inference driver of the reference)
  with pytest.raises(NotImplementedError, match=r"graph variants not built on this path \(SURVEY.md 8, out of scope\): use_cascade_rcnn$"):
    models.get_model(_cfg(use_cascade_rcnn=True), 0, weights=w, lib=emu_lib)


# ------------------------------------------------------------------------------------------------- weights

def test_att_head_synthetic_weights_leave_the_rest_alone():
  for kw in (dict(), dict(use_conv_frcnn_head=True, use_gn=True), dict(add_relation_nn=True), dict(add_mask=True)):
    cfg = _cfg(**kw)
    w = synthetic_weights(cfg, 3)
    base = synthetic_weights(_cfg(use_att_frcnn_head=False, **kw), 3)
    head = att_head_variables(cfg)
    assert head == ["fastrcnn/attention/W", "fastrcnn/attention/b", "fastrcnn/att_trans/W", "fastrcnn/att_trans/b"]
    assert set(w) - set(base) == set(head) and set(base) <= set(w)
    for k, v in base.items():
      assert np.array_equal(v, w[k]), k
    assert w["fastrcnn/attention/W"].shape == (3, 3, 256, 1) and w["fastrcnn/attention/b"].shape == (1,)
    assert w["fastrcnn/att_trans/W"].shape == (256, 1024) and w["fastrcnn/att_trans/b"].shape == (1024,)
    assert all(np.isfinite(w[k]).all() and w[k].dtype == F for k in head)
  assert att_head_variables(_cfg(use_att_frcnn_head=False)) == []


def test_att_head_weights_survive_the_writers(tmp_path):
  """The four variables come back from every writer / reader pair of the repository (.npz, TF checkpoint, frozen .pb), and
  config_from_weights reads the flag off fastrcnn/att_trans/W."""
  from object_detection_tracking_amd.frozen_pb import load_frozen_pb, write_frozen_pb
  from object_detection_tracking_amd.tf_checkpoint import load_checkpoint, write_checkpoint
  from object_detection_tracking_amd.weights import load_npz
  cfg = _cfg()
  w = synthetic_weights(cfg, 0)
  np.savez(str(tmp_path / "h.npz"), **{k + ":0": v for k, v in w.items()})
  (tmp_path / "ck").mkdir()
  write_checkpoint(str(tmp_path / "ck" / "model-3"), w)
  write_frozen_pb(str(tmp_path / "h.pb"), w)
  for got in (load_npz(str(tmp_path / "h.npz")), load_checkpoint(str(tmp_path / "ck")), load_frozen_pb(str(tmp_path / "h.pb"))):
    assert set(got) >= set(w)
    for k in att_head_variables(cfg):
      assert np.array_equal(np.asarray(got[k], np.float32).reshape(w[k].shape), w[k]), k
  c = models.config_from_weights(load_frozen_pb(str(tmp_path / "h.pb")))
  assert c.use_att_frcnn_head and not c.use_conv_frcnn_head and not c.use_frcnn_class_agnostic
  assert list(c.resnet_num_block) == [1, 1, 1, 1]
  assert not models.config_from_weights(synthetic_weights(_cfg(use_att_frcnn_head=False), 0)).use_att_frcnn_head


# ------------------------------------------------------------------------------------------------- op level

def _seq_sum(x):
  """x [R,49,C] float32 -> [R,C]: the 49 positions added to +0 one after another, every addition rounded to float32."""
  s = np.zeros((x.shape[0], x.shape[2]), F)
  for k in range(x.shape[1]):
    s = (s + x[:, k, :]).astype(F)
  return s


def _bits(a):
  return np.asarray(a, F).view(np.uint32)


# (1, 4): one thread; (3, 256): the plans' width, 192 of a workgroup's 256 threads; (5, 64): RoIs that share a wave; (33, 260): nine
# workgroups, the last ragged, a quad count (65) that no power of two divides
POOL_SHAPES = [(1, 4), (3, 256), (5, 64), (33, 260)]


@pytest.mark.parametrize("R,C", POOL_SHAPES)
def test_att_pool_against_the_sequential_sum(backend, R, C):
  name, lib = backend
  rng = np.random.default_rng(100 * R + C)
  x = (rng.standard_normal((R, 49, C)) * rng.uniform(0.5, 2.0, (R, 1, C)) + 0.3 * rng.standard_normal((R, 1, C))).astype(F)
  out, amax = ops.att_pool(x, lib=lib)
  ref = _seq_sum(x)
  assert out.shape == (R, C) and np.array_equal(_bits(out), _bits(ref))
  s64 = x.astype(np.float64).sum(axis=1)
  bound = 48 * U * np.abs(x.astype(np.float64)).sum(axis=1)
  err = np.abs(out.astype(np.float64) - s64)
  print("att_pool (%d, %d): worst error / bound %.3g" % (R, C, float((err / bound).max())))
  assert (err <= bound).all()
  assert _bits(amax) == _bits(np.abs(out).max())
  out2, amax2 = ops.att_pool(x.reshape(R, 7, 7, C), lib=lib)
  assert np.array_equal(_bits(out), _bits(out2)) and amax == amax2


@pytest.mark.parametrize("R,C", POOL_SHAPES)
def test_att_pool_exact_on_integer_data(backend, R, C):
  """Small integers: every partial sum is exact, so a position read twice, skipped or taken from another RoI or channel shows.
  Position k of channel c of RoI r holds (k + 1) * s + c % 7 - r % 3 with s = 1 or -1 by channel parity."""
  name, lib = backend
  k = np.arange(49).reshape(1, 49, 1); c = np.arange(C).reshape(1, 1, C); r = np.arange(R).reshape(R, 1, 1)
  x = ((k + 1) * np.where(c % 2 == 0, 1, -1) + c % 7 - r % 3).astype(F)
  out, amax = ops.att_pool(x, lib=lib)
  want = (1225 * np.where(c % 2 == 0, 1, -1) + 49 * (c % 7 - r % 3)).reshape(R, C).astype(F)
  assert np.array_equal(out, want)
  assert np.float32(amax) == np.abs(want).max()


def test_att_pool_zero_rows_and_row_independence(backend):
  """An all-zero RoI (a row past the proposal count) gives zeros; a RoI gives the same bits at another row of a tensor of another
  R."""
  name, lib = backend
  rng = np.random.default_rng(9)
  x = rng.standard_normal((5, 49, 64)).astype(F)
  x[1] = 0; x[4] = 0
  out, amax = ops.att_pool(x, lib=lib)
  assert not out[1].any() and not out[4].any() and not np.signbit(out[1]).any()
  perm = np.array([3, 0, 4, 2, 1])
  outp, amaxp = ops.att_pool(x[perm], lib=lib)
  assert np.array_equal(_bits(outp), _bits(out[perm])) and amaxp == amax
  out1, _ = ops.att_pool(x[3:4], lib=lib)
  assert np.array_equal(_bits(out1[0]), _bits(out[3]))
  z, az = ops.att_pool(np.zeros((2, 49, 8), F), lib=lib)
  assert not z.any() and az == 0.0


@pytest.mark.parametrize("R,D,ldh", [(1, 64, 64), (7, 1024, 1024), (5, 64, 128)])
def test_att_add_against_numpy(backend, R, D, ldh):
  """Bit for bit numpy's float32 addition; with ldh > D the columns of h past D are NaN and are never read."""
  name, lib = backend
  rng = np.random.default_rng(R + D + ldh)
  h = np.full((R, ldh), np.nan, F)
  h[:, :D] = np.maximum(rng.standard_normal((R, D)), 0) * 3
  a = np.maximum(rng.standard_normal((R, D)), 0).astype(F)
  out, amax = ops.att_add(h, a, view=D, lib=lib)
  want = h[:, :D] + a
  assert out.shape == (R, D) and want.dtype == F and np.array_equal(_bits(out), _bits(want))
  assert _bits(amax) == _bits(np.abs(want).max())
  hs = (rng.standard_normal((R, D)) * 1e3).astype(F); as_ = rng.standard_normal((R, D)).astype(F)      # signed, rounding additions
  out, amax = ops.att_add(hs, as_, lib=lib)
  assert np.array_equal(_bits(out), _bits(hs + as_)) and _bits(amax) == _bits(np.abs(hs + as_).max())


def test_att_ops_reject_bad_arguments(emu_lib):
  """Null pointers, C % 4 != 0, ldh < D and non-positive sizes: an error string and no launch."""
  import ctypes as C
  from object_detection_tracking_amd._lib import OdtError
  from object_detection_tracking_amd.ops import fptr
  z = lambda *s: np.zeros(s, F)
  dll = emu_lib.dll
  x, o, am = z(2, 49, 8), z(2, 8), z(1)
  null = C.POINTER(C.c_float)()
  for args in ((null, 2, 8, fptr(o), fptr(am)), (fptr(x), 2, 8, null, fptr(am)), (fptr(x), 2, 8, fptr(o), null)):
    with pytest.raises(OdtError, match="odt_op_att_pool: null argument"):
      emu_lib.check(dll.odt_op_att_pool(0, *args))
  for R_, C_ in ((0, 8), (2, 0), (-1, 8)):
    with pytest.raises(OdtError, match="odt_op_att_pool: bad sizes"):
      emu_lib.check(dll.odt_op_att_pool(0, fptr(x), R_, C_, fptr(o), fptr(am)))
  with pytest.raises(OdtError, match=r"odt_op_att_pool: C must be a multiple of 4 \(C = 6\)"):
    ops.att_pool(z(2, 49, 6), lib=emu_lib)
  h, a, o = z(2, 8), z(2, 8), z(2, 8)
  for args in ((null, 8, fptr(a), 2, 8, fptr(o), fptr(am)), (fptr(h), 8, null, 2, 8, fptr(o), fptr(am)),
               (fptr(h), 8, fptr(a), 2, 8, null, fptr(am)), (fptr(h), 8, fptr(a), 2, 8, fptr(o), null)):
    with pytest.raises(OdtError, match="odt_op_att_add: null argument"):
      emu_lib.check(dll.odt_op_att_add(0, *args))
  for ldh, R_, D_ in ((8, 0, 8), (8, 2, 0), (0, 2, 8), (8, -2, 8)):
    with pytest.raises(OdtError, match="odt_op_att_add: bad sizes"):
      emu_lib.check(dll.odt_op_att_add(0, fptr(h), ldh, fptr(a), R_, D_, fptr(o), fptr(am)))
  with pytest.raises(OdtError, match=r"odt_op_att_add: D must be a multiple of 4 \(D = 6\)"):
    ops.att_add(z(2, 6), z(2, 6), lib=emu_lib)
  with pytest.raises(OdtError, match=r"odt_op_att_add: ldh must be a multiple of 4 and at least D \(ldh = 4, D = 8\)"):
    emu_lib.check(dll.odt_op_att_add(0, fptr(h), 4, fptr(a), 2, 8, fptr(o), fptr(am)))
  with pytest.raises(OdtError, match=r"odt_op_att_add: ldh must be a multiple of 4 and at least D \(ldh = 10, D = 8\)"):
    ops.att_add(z(2, 10), z(2, 8), view=8, lib=emu_lib)


@pytest.mark.gpu
def test_att_ops_real_width_gpu(hip_lib):
  """The reference's sizes: 1000 proposals, 256 FPN channels, a 1024-wide hidden vector (64000 and 256000 threads)."""
  rng = np.random.default_rng(1000)
  x = rng.standard_normal((1000, 49, 256)).astype(F)
  x[997:] = 0
  out, amax = ops.att_pool(x, lib=hip_lib)
  ref = _seq_sum(x)
  assert np.array_equal(_bits(out), _bits(ref)) and _bits(amax) == _bits(np.abs(ref).max()) and not out[997:].any()
  h = np.maximum(rng.standard_normal((1000, 1024)), 0).astype(F); a = np.maximum(rng.standard_normal((1000, 1024)), 0).astype(F)
  o, am = ops.att_add(h, a, lib=hip_lib)
  assert np.array_equal(_bits(o), _bits(h + a)) and _bits(am) == _bits((h + a).max())
