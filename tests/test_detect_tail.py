"""The detection tail (csrc/detections.hip) on its own: head_post_kernel, class_nms_kernel, class_nms_big_kernel and
final_select_kernel.

The selection half takes caller-supplied boxes and scores through ops.class_nms, so no device expf stands between the
inputs and the picks: every output is compared bit for bit with the oracle (oracle/graph.fastrcnn_predictions for
ODT_GRAPH_SINGLE, oracle/tfops.combined_non_max_suppression over the zero-padded [B, M, C] layout of reference
models.py:2937-2950 for ODT_GRAPH_MULTI).  head_post_kernel is seen whole through ops.detections with suppression off.

Oracle results are computed once per case list and shared by the two backends.
"""
import functools

import numpy as np
import pytest

from object_detection_tracking_amd import ops
from object_detection_tracking_amd._lib import ODT_GRAPH_MULTI, ODT_GRAPH_SINGLE, OdtError
from oracle import graph as og
from oracle import tfops

F = np.float32
SINGLE_THRESH = 0.3          # ODT_GRAPH_SINGLE: some rows are non-candidates (MULTI takes every row)


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _boxes(rng, B, N, Cn):
  """Per class: clustered boxes, N // 6 centres in a 100 px square, sigma 5, sides 4..50."""
  out = np.zeros((B, N, Cn, 4), F)
  for b in range(B):
    for c in range(Cn):
      ctr = rng.uniform(0, 100, (max(1, N // 6), 2))
      xy = ctr[rng.integers(0, ctr.shape[0], N)] + rng.normal(0, 5, (N, 2))
      wh = rng.uniform(4, 50, (N, 2))
      out[b, :, c] = np.concatenate([xy - wh / 2, xy + wh / 2], 1)
  return out


def _scores(rng, shape, zero_frac=0.0):
  """Half quantised to k / 8 (exact ties across RoIs and classes), half uniform in [0.01, 1); zero_frac set to 0."""
  q = rng.integers(1, 9, shape) / 8.0
  u = rng.uniform(0.01, 1.0, shape)
  s = np.where(rng.random(shape) < 0.5, q, u).astype(F)
  if zero_frac:
    s[rng.random(shape) < zero_frac] = F(0)
  return s


def _case(graph, B, N, Cn, per_im, iou, rng, ncand=None, zero_frac=0.0):
  return dict(graph=graph, B=B, N=N, Cn=Cn, per_im=per_im, iou=iou, boxes=_boxes(rng, B, N, Cn),
              scores=_scores(rng, (B, N, Cn), zero_frac),
              ncand=np.asarray(ncand if ncand is not None else rng.integers(1, N + 1, B), np.int32))


def _fuzz_case(seed, family):
  rng = np.random.default_rng(seed)
  graph = ODT_GRAPH_MULTI if seed % 2 else ODT_GRAPH_SINGLE
  B = int(rng.integers(1, 4)) if graph == ODT_GRAPH_MULTI else 1
  if family == "small":
    N, Cn, per_im = int(rng.integers(1, 40)), int(rng.integers(1, 7)), int(rng.integers(1, 12))
  elif family == "wide":
    N, Cn = int(rng.integers(1, 200)), int(rng.choice([1, 2, 5, 17, 63]))
    per_im = int(rng.integers(1, 4096 // Cn + 1)) if seed % 3 == 0 else int(rng.integers(1, 30))
  else:                # "zeros": 40 % of the scores exactly 0, batched graph only (section "zero-score ties" below)
    graph, B = ODT_GRAPH_MULTI, int(rng.integers(2, 4))
    N, Cn, per_im = int(rng.integers(2, 20)), 2, int(rng.integers(4, 40))
  iou = float(rng.choice([0.3, 0.5, 0.7]))
  return _case(graph, B, N, Cn, per_im, iou, rng, zero_frac=0.4 if family == "zeros" else 0.0)


# ---- oracle ---------------------------------------------------------------------------------------------------------------
def _multi_layout(case):
  """The real rows (j < ncand[b]) of all images scattered into the zero-padded [B, M, C] arrays, as test_detections_multi
  does.  Returns (boxes, scores, first row of each image)."""
  B, Cn, nc = case["B"], case["Cn"], case["ncand"]
  rows = [(b, j) for b in range(B) for j in range(nc[b])]
  M = len(rows)
  bidx = np.array([b for b, _ in rows]); jidx = np.array([j for _, j in rows])
  pbx = np.zeros((B, M, Cn, 4), F); ppr = np.zeros((B, M, Cn), F)
  pbx[bidx, np.arange(M)] = case["boxes"][bidx, jidx]; ppr[bidx, np.arange(M)] = case["scores"][bidx, jidx]
  return pbx, ppr, np.r_[0, np.cumsum(nc)]


def _oracle(case):
  """(boxes [B,per_im,4], scores [B,per_im], classes [B,per_im], valid [B]), zero-padded."""
  per_im, iou = case["per_im"], case["iou"]
  if case["graph"] == ODT_GRAPH_MULTI:
    pbx, ppr, _ = _multi_layout(case)
    return tfops.combined_non_max_suppression(pbx, ppr, per_im, per_im, iou)
  n = int(case["ncand"][0])
  bx, sc = case["boxes"][0, :n], case["scores"][0, :n]
  probs = np.concatenate([np.zeros((n, 1), F), sc], 1)
  pi, fp, _ = og.fastrcnn_predictions(bx, probs, SINGLE_THRESH, per_im, iou)
  r = pi.shape[0]
  ob = np.zeros((1, per_im, 4), F); os_ = np.zeros((1, per_im), F); oc = np.zeros((1, per_im), F)
  ob[0, :r] = bx[pi[:, 0], pi[:, 1]]; os_[0, :r] = fp; oc[0, :r] = pi[:, 1]
  return ob, os_, oc, np.array([r], np.int32)


def _oracle_traced(case):
  """_oracle(case) and, for _events, the per-class NMS calls the oracle made on the way: [(scores, selected)] in (image,
  class) order."""
  calls = []
  real = tfops.non_max_suppression

  def traced(boxes, scores, *args, **kw):
    sel = real(boxes, scores, *args, **kw)
    calls.append((np.asarray(scores, F).reshape(-1), sel))
    return sel
  tfops.non_max_suppression = traced
  try:
    want = _oracle(case)
  finally:
    tfops.non_max_suppression = real
  assert len(calls) == case["B"] * case["Cn"]
  return want, calls


def _events(case, calls):
  """What the case exercises, from the oracle's own per-class NMS calls (any image counts):
  cap     -- a class reaches the per-class cap with candidates left unexamined
  union   -- the union of the class lists exceeds per_im
  tie     -- the scores at merged ranks per_im - 1 and per_im are equal and their classes differ
  supp    -- at least one candidate is suppressed
  slots   -- MULTI: zero slots of other images are among the picks (valid > number of real survivors)"""
  per_im, Cn = case["per_im"], case["Cn"]
  ev = dict(cap=False, union=False, tie=False, supp=False, slots=False)
  first = np.r_[0, np.cumsum(case["ncand"])]
  for b in range(case["B"]):
    merged = []
    for c in range(Cn):
      sc, sel = calls[b * Cn + c]
      examined = sc.size
      if sel.size == per_im:
        examined = int(np.where(np.argsort(-sc, kind="stable") == sel[-1])[0][0]) + 1
        ev["cap"] |= examined < sc.size
      ev["supp"] |= examined > sel.size
      merged += [(-float(sc[i]), c, o, int(i)) for o, i in enumerate(sel)]
    merged.sort()
    ev["union"] |= len(merged) > per_im
    if len(merged) > per_im:
      ev["tie"] |= merged[per_im - 1][0] == merged[per_im][0] and merged[per_im - 1][1] != merged[per_im][1]
    if case["graph"] == ODT_GRAPH_MULTI:
      ev["slots"] |= any(not first[b] <= i < first[b + 1] for _, _, _, i in merged[:per_im])
  return ev


def _check(lib, case, want):
  thr = SINGLE_THRESH if case["graph"] == ODT_GRAPH_SINGLE else 0.0
  gb, gs, gc, gv = ops.class_nms(case["graph"], case["boxes"], case["scores"], case["per_im"], case["iou"], score_thresh=thr,
                                 ncand=case["ncand"], lib=lib)
  wb, ws, wc, wv = want
  tag = {k: case[k] for k in ("graph", "B", "N", "Cn", "per_im", "iou")}, case["ncand"].tolist()
  assert np.array_equal(gv, wv), (tag, gv, wv)
  assert np.array_equal(gs, ws), tag
  assert np.array_equal(gb, wb), tag
  for b in range(case["B"]):
    assert np.array_equal(gc[b, :wv[b]], wc[b, :wv[b]].astype(np.int32)), (tag, b)
    if case["graph"] == ODT_GRAPH_SINGLE:
      assert not gb[b, wv[b]:].any() and not gs[b, wv[b]:].any(), tag


# ---- 1. fuzz of the selection half ------------------------------------------------------------------------------------------
FUZZ_CHUNKS, FUZZ_CHUNK = 3, 100       # seeds per family, in chunks; graph = seed parity: 150 cases per family per graph


@functools.lru_cache(maxsize=None)
def _fuzz(family, chunk):
  """(cases, oracle results, events) of seeds chunk * 100 .. + 99."""
  cases = [_fuzz_case(seed, family) for seed in range(chunk * FUZZ_CHUNK, (chunk + 1) * FUZZ_CHUNK)]
  traced = [_oracle_traced(c) for c in cases]
  return cases, [w for w, _ in traced], [_events(c, calls) for c, (_, calls) in zip(cases, traced)]


@pytest.mark.parametrize("family", ["small", "wide"])
def test_class_nms_fuzz_is_not_vacuous(family):
  """Over the cases of each graph, each event the fuzz is there for happens in at least 5 % of them (_events)."""
  cases, evs = [], []
  for chunk in range(FUZZ_CHUNKS):
    c, _, e = _fuzz(family, chunk)
    cases += c; evs += e
  for graph in (ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI):
    ge = [e for c, e in zip(cases, evs) if c["graph"] == graph]
    assert len(ge) >= 150
    for name in ("cap", "union", "tie", "supp") + (("slots",) if graph == ODT_GRAPH_MULTI else ()):
      share = sum(e[name] for e in ge) / len(ge)
      print("%s graph %d %s: %.0f %%" % (family, graph, name, 100 * share))
      assert share >= 0.05, (family, graph, name, share)


@pytest.mark.parametrize("chunk", range(FUZZ_CHUNKS))
@pytest.mark.parametrize("family", ["small", "wide"])
def test_class_nms_fuzz_bit_exact(backend, family, chunk):
  """Tie order of final_select_kernel across classes, per-class and total caps, ncand < N, up to 63 classes, (C-1) * per_im
  up to 4096, the batched graph's padding slots: boxes, scores, valid and classes equal the oracle's, bit for bit."""
  name, lib = backend
  cases, want, _ = _fuzz(family, chunk)
  for case, w in zip(cases, want):
    _check(lib, case, w)


# ---- 2. more than 1024 candidates: class_nms_big_kernel ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_cases(N, graph):
  """N rows, all real; C - 1 in {1, 2}; per_im stops the paneled walk inside a panel and after the last one.  MULTI gets a
  second image of 7 real rows, so both images see slots.  With the SINGLE threshold fewer candidates than rows remain (the
  keys == 0 rows of the rank sort)."""
  out = []
  for Cn in (1, 2):
    for per_im in (5, 100, 600, 2048 // Cn):
      rng = np.random.default_rng(N * 8 + Cn * 4 + per_im % 4)
      B = 2 if graph == ODT_GRAPH_MULTI else 1
      case = _case(graph, B, N, Cn, per_im, 0.5, rng, ncand=[N, 7][:B])
      out.append((case, _oracle(case)))
  return out


@pytest.mark.parametrize("graph", [ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI], ids=["single", "multi"])
@pytest.mark.parametrize("N", [1025, 1536, 1537, 2049])      # one past a panel pair, three panels, three panels + 1, four + 1
def test_class_nms_big_bit_exact(backend, N, graph):
  name, lib = backend
  for case, want in _big_cases(N, graph):
    _check(lib, case, want)


@pytest.mark.gpu
def test_class_nms_big_4096(hip_lib):
  rng = np.random.default_rng(4096)
  case = _case(ODT_GRAPH_SINGLE, 1, 4096, 1, 4096, 0.7, rng, ncand=[4096])
  _check(hip_lib, case, _oracle(case))


# ---- 3. limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,per_im", [(63, 65), (1, 4096), (2, 2048), (16, 256)], ids=lambda v: str(v))
@pytest.mark.parametrize("graph", [ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI], ids=["single", "multi"])
def test_class_nms_at_the_limits(backend, graph, Cn, per_im):
  """63 foreground classes (s_off[64]) and (C-1) * per_im == 4096 (kMaxFinal) are accepted and right."""
  name, lib = backend
  rng = np.random.default_rng(Cn)
  B = 2 if graph == ODT_GRAPH_MULTI else 1
  case = _case(graph, B, 90, Cn, per_im, 0.5, rng, ncand=[90, 60][:B])
  _check(lib, case, _oracle(case))


def _tiny_call(lib, N, Cn, per_im):
  return ops.class_nms(ODT_GRAPH_SINGLE, np.zeros((1, N, Cn, 4), F), np.ones((1, N, Cn), F), per_im, 0.5, lib=lib)


@pytest.mark.parametrize("Cn,per_im", [(1, 4097), (17, 241)], ids=lambda v: str(v))
def test_rejects_final_list_over_4096(backend, Cn, per_im):
  name, lib = backend
  with pytest.raises(OdtError, match=r"\(C-1\)\*result_per_im too large"):
    _tiny_call(lib, 3, Cn, per_im)


def test_rejects_64_foreground_classes(backend):
  name, lib = backend
  with pytest.raises(OdtError, match="2..64 classes"):
    _tiny_call(lib, 3, 64, 2)


def test_rejects_more_than_4096_rows(backend):
  name, lib = backend
  with pytest.raises(OdtError, match=r"K must be in \[1,4096\]"):
    _tiny_call(lib, 4097, 1, 2)


# ---- 4. zero-score real rows against the other images' zero slots (ODT_GRAPH_MULTI) -----------------------------------------
def test_zero_score_row_and_slots_hand_case(backend):
  """Image 1's rows come after image 0's one row in the [B, M, C] layout, so that row's slot (score 0, zero box, position 0)
  wins the (score desc, position asc) tie against image 1's own zero-score rows: per class, positive rows, the slot, the
  zero-score row.  Merged: .9 (class 0), .8 (class 1), then the zeros of class 0 -- its slot, then its zero-score row."""
  name, lib = backend
  boxes = np.zeros((2, 2, 2, 4), F)
  boxes[0, 0] = [[70, 70, 90, 90], [72, 72, 92, 92]]
  boxes[1, 0] = [[10, 10, 30, 30], [40, 40, 60, 60]]                # row 0: class 0 (.9), class 1 (0)
  boxes[1, 1] = [[40, 40, 60, 60], [11, 11, 31, 31]]                # row 1: class 0 (0), class 1 (.8)
  scores = np.zeros((2, 2, 2), F)
  scores[0, 0] = [.7, .6]
  scores[1] = [[.9, 0], [0, .8]]
  ncand = np.array([1, 2], np.int32)
  gb, gs, gc, gv = ops.class_nms(ODT_GRAPH_MULTI, boxes, scores, 4, 0.5, ncand=ncand, lib=lib)
  case = dict(graph=ODT_GRAPH_MULTI, B=2, N=2, Cn=2, per_im=4, iou=0.5, boxes=boxes, scores=scores, ncand=ncand)
  wb, ws, wc, wv = _oracle(case)
  # the oracle's values, written out
  assert wv.tolist() == [4, 4]
  assert wb[1].tolist() == [[10, 10, 30, 30], [11, 11, 31, 31], [0, 0, 0, 0], [40, 40, 60, 60]]
  assert ws[1].tolist() == [F(.9), F(.8), 0, 0] and wc[1].tolist() == [0, 1, 0, 0]
  assert wb[0].tolist() == [[70, 70, 90, 90], [72, 72, 92, 92], [0, 0, 0, 0], [0, 0, 0, 0]]
  assert ws[0].tolist() == [F(.7), F(.6), 0, 0] and wc[0].tolist() == [0, 1, 0, 0]
  assert gv.tolist() == [4, 4]
  assert np.array_equal(gb, wb) and np.array_equal(gs, ws) and np.array_equal(gc, wc.astype(np.int32))


def test_class_nms_fuzz_zero_scores_bit_exact(backend):
  """The fuzz with 40 % of the scores exactly 0: B 2..3, N 2..19, C - 1 = 2, per_im 4..39."""
  name, lib = backend
  cases, want, _ = _fuzz("zeros", 0)
  assert all(c["graph"] == ODT_GRAPH_MULTI and c["B"] >= 2 for c in cases)
  for case, w in zip(cases, want):
    _check(lib, case, w)


def test_detections_multi_exact_zero_probabilities(backend):
  """Through ops.detections: class logits 250 below the row maximum make the f32 softmax exactly 0 on the device and in numpy
  alike; per_im exceeds the real survivors, so zero-score rows and slots of the other image are both picked."""
  name, lib = backend
  rng = np.random.default_rng(41)
  B, K, Cn, img_hw = 2, 8, 3, (96, 128)
  nprops = np.array([3, 5], np.int32)
  props = np.zeros((B, K, 4), F)
  for b in range(B):
    props[b] = og.clip_boxes(_boxes(rng, 1, K, 1)[0, :, 0], img_hw)
  cls = (rng.standard_normal((B * K, Cn)) * 2.0).astype(F)
  box = (rng.standard_normal((B * K, Cn, 4)) * 0.8).astype(F)
  for r, c in ((0, 1), (2, 2), (K + 0, 2), (K + 1, 1), (K + 3, 1), (K + 3, 2), (K + 4, 1)):
    cls[r, c] = cls[r].max() - F(250)
  rw = np.array([10, 10, 5, 5], F)
  clip = float(np.log(1333 / 16.0))
  per_im = 12
  gb, gp, gl, gv = ops.detections(ODT_GRAPH_MULTI, cls, box, props, nprops, img_hw, rw, clip, 1e-4, 0.5, per_im, lib=lib)
  rows = [(b, j) for b in range(B) for j in range(nprops[b])]
  M = len(rows)
  rb = np.stack([props[b, j] for b, j in rows]); sel = [b * K + j for b, j in rows]
  dec, probs = og.head_decode(rb, box[sel][:, 1:], cls[sel], img_hw, rw)
  assert (probs[:, 1:] == 0).sum() == 7                           # exact zeros among the real rows' foreground classes
  bidx = np.array([b for b, _ in rows])
  pbx = np.zeros((B, M, Cn - 1, 4), F); ppr = np.zeros((B, M, Cn - 1), F)
  pbx[bidx, np.arange(M)] = dec; ppr[bidx, np.arange(M)] = probs[:, 1:]
  nb, ns, nc, nv = tfops.combined_non_max_suppression(pbx, ppr, per_im, per_im, 0.5)
  # image 1 (rows after image 0's): a zero-score real row follows a slot in the oracle's picks
  z = np.where(ns[1] == 0)[0]
  assert nb[1, z[0]].max() == 0 and nb[1, z].max() > 0
  assert np.array_equal(gv, nv)
  assert np.array_equal(gl, (nc + 1).astype(np.int32))
  np.testing.assert_allclose(gp, ns, rtol=0, atol=5e-6)
  np.testing.assert_allclose(gb, nb, rtol=0, atol=1e-3)


# ---- 5. head_post_kernel, every (RoI, class) pair ---------------------------------------------------------------------------
HEAD_POST_SEED = 18     # one whose 39 reference probabilities are pairwise 1e-4 apart (asserted below)


def _head_post_inputs(seed):
  rng = np.random.default_rng(seed)
  K, C, img_hw = 16, 4, (96, 128)
  n = 13                                                          # nprops < K: rows 13..15 must not appear
  H, W = img_hw
  props = np.zeros((1, K, 4), F)
  ctr = rng.uniform(30, 66, (K, 2)); wh = rng.uniform(6, 40, (K, 2))
  props[0] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
  props[0, 0] = [0, 0, 30, 20]; props[0, 1] = [100, 70, W, H]      # at the frame border
  props[0, 2] = [0, 60, 25, H]; props[0, 3] = [90, 0, W, 30]
  props[0, 4] = [50, 40, 50, 70]                                   # zero width
  props[0, 5] = [60, 45, 60.5, 45.5]                               # small: the clipped exp stays inside the frame
  cls = rng.uniform(-1.5, 1.5, (K, C)).astype(F)
  box = (rng.standard_normal((K, C, 4)) * 0.8).astype(F)
  box[0, 1:, :2] = -20; box[1, 1:, :2] = 20                        # shifted out of the frame: x1, y1 < 0 / x2, y2 > frame
  box[2, 1:, 2:] = 9; box[3, 1:, 2:] = 9                           # grown past the frame
  box[5, 1:, 2:] = [[30, 23], [25, 40], [22.5, 100]]               # tw / th = logit / 5 above decode_clip = 4.42
  box[6, 1, 2] = 24
  return K, C, img_hw, n, props, cls, box


def test_head_post_every_pair(backend, monkeypatch):
  """Softmax, decode and clip of every (RoI, class) pair: ODT_GRAPH_SINGLE with nms_thresh 1 (no IoU exceeds 1: nothing is
  suppressed), score_thresh -1 and per_im = K * (C - 1), so the output holds all pairs of the nprops real rows in
  probability order.  Reference: oracle/graph.head_decode evaluated in float64 (the oracle modules' float type swapped).
  Pairs are identified by their rank: the reference's probabilities are at least 1e-4 apart (20 x the tolerance).
  Tolerances of test_detections_single: probabilities 5e-6, boxes 1e-3 * max(img_hw) / 128 px; labels exact."""
  name, lib = backend
  K, C, img_hw, n, props, cls, box = _head_post_inputs(HEAD_POST_SEED)
  H, W = img_hw
  rw = np.array([10, 10, 5, 5], F)
  clip = float(np.log(1333 / 16.0))
  per_im = K * (C - 1)
  nprops = np.array([n], np.int32)
  gb, gp, gl, gv = ops.detections(ODT_GRAPH_SINGLE, cls, box, props, nprops, img_hw, rw, clip, -1.0, 1.0, per_im, lib=lib)

  monkeypatch.setattr(og, "F", np.float64)
  monkeypatch.setattr(tfops, "F", np.float64)
  dec, probs = og.head_decode(props[0].astype(np.float64), box[:, 1:].astype(np.float64), cls.astype(np.float64), img_hw,
                              rw.astype(np.float64))
  raw = og.decode_bbox_target(box[:, 1:] / rw.astype(np.float64), np.repeat(props[0][:, None], C - 1, 1), 1e9)  # no clips
  monkeypatch.undo()
  assert dec.dtype == np.float64 and probs.dtype == np.float64
  # conditions on the inputs: deltas above decode_clip that the frame does not hide, all four frame clips, both ways
  tw = box[:n, 1:, 2:] / rw[2:]
  assert (tw > clip).sum() >= 6
  assert (dec[5, :, 2] - dec[5, :, 0]).max() < 60 and (dec[5, :, 3] - dec[5, :, 1]).max() < 60
  raw = raw.reshape(K, C - 1, 4)[:n]
  assert (raw[..., 0] < 0).any() and (raw[..., 1] < 0).any() and (raw[..., 2] > W).any() and (raw[..., 3] > H).any()
  assert (raw[..., 2] < 0).any() and (raw[..., 0] > W).any()
  assert props[0, 4, 0] == props[0, 4, 2]
  fg = probs[:n, 1:]
  order = np.argsort(-fg.reshape(-1), kind="stable")
  sp = fg.reshape(-1)[order]
  assert np.diff(sp).max() <= -1e-4, np.diff(sp).max()              # condition on the seed
  roi, c = order // (C - 1), order % (C - 1)
  r = n * (C - 1)
  assert gv[0] == r
  assert np.array_equal(gl[0, :r], (c + 1).astype(np.int32))
  np.testing.assert_allclose(gp[0, :r], sp, rtol=0, atol=5e-6)
  np.testing.assert_allclose(gb[0, :r], dec[roi, c], rtol=0, atol=1e-3 * max(img_hw) / 128)
  assert not gb[0, r:].any() and not gp[0, r:].any() and not gl[0, r:].any()
