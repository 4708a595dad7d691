"""RPN proposal generation (csrc/proposals.hip over the primitives of csrc/select_device.hpp) on its own, through
ops.proposals and ops.nms.

The only inexact operation between the inputs and the proposals is expf in the decode, and exp(+-0) = 1, exp(-inf) = 0
are exact (IEEE 754; numpy's float32 exp, which oracle/graph.decode_bbox_target uses, and expf agree).  With every size
delta 0.0 or -inf -- the centre deltas stay arbitrary floats -- the rest is + - * (one rounding each: the build uses
-ffp-contract=off) and fminf / fmaxf, so sections 1-4 compare props, nprops and the zero tail with the oracle bit for bit.
Section 5 sees expf on general arguments with suppression off, against the same decode in float64.

Oracle results are computed once per case list and shared by the two backends.
"""
import functools

import numpy as np
import pytest

from object_detection_tracking_amd import ops
from object_detection_tracking_amd._lib import ODT_GRAPH_MULTI, ODT_GRAPH_SINGLE, OdtError
from oracle import graph as og
from oracle import tfops
from oracle.anchors import all_anchors
from test_ops import _oracle_proposals_multi, _oracle_proposals_single

F = np.float32
STRIDES, SIZES = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512)
RATIOS = (0.5, 1, 2)
CLIP = float(np.log(256 / 16.0))       # decode_clip of the exact sections: never reached by a size delta of 0 or -inf
GRAPHS = pytest.mark.parametrize("graph", [ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI], ids=["single", "multi"])


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _logits(rng, shape, shift, ninf=0.0, pinf=0.0):
  """Per element: half multiples of 0.25 in [-2, 2] (exact ties within and across levels), half N(0, 1.5^2); minus shift;
  half of the exact zeros become -0.0; fractions ninf / pinf of the elements become -inf / +inf."""
  q = rng.integers(-8, 9, shape) * 0.25
  g = rng.standard_normal(shape) * 1.5
  lg = (np.where(rng.random(shape) < 0.5, q, g) - shift).astype(F)
  lg[(lg == 0) & (rng.random(shape) < 0.5)] = F(-0.0)
  u = rng.random(shape)
  lg[u < ninf] = -np.inf
  lg[(u >= ninf) & (u < ninf + pinf)] = np.inf
  return lg


def _deltas(rng, shape):
  """[..., 3, 4]: centre deltas N(0, 0.5^2), 5 % of the x deltas times 8 (boxes that leave the image and clip to zero
  width); size deltas 0.0, 6 % of them -inf (zero-width / zero-height boxes)."""
  dl = np.zeros(shape + (4,), F)
  dl[..., :2] = rng.standard_normal(shape + (2,)) * 0.5
  dl[..., 0] *= np.where(rng.random(shape) < 0.05, 8.0, 1.0).astype(F)
  dl[..., 2:][rng.random(shape + (2,)) < 0.06] = -np.inf
  return dl


def _pack(lg, dl):
  """The device layout, its unused 16th channel NaN: the plans' fused RPN head leaves it unspecified."""
  r = ops.pack_rpn(lg, dl)
  r[..., 15] = np.nan
  return r


def _case(graph, B, levels, hw_levels, img_hw, K, thr, rng, shift=0.0, ninf=0.0, pinf=0.0):
  logits, deltas, anchors = [], [], []
  for li, (h, w) in zip(levels, hw_levels):
    logits.append(_logits(rng, (B, h, w, 3), shift, ninf, pinf))
    deltas.append(_deltas(rng, (B, h, w, 3)))
    anchors.append(all_anchors(STRIDES[li], [SIZES[li]], RATIOS, max(img_hw) + 64))
  return dict(graph=graph, B=B, levels=list(levels), img_hw=img_hw, K=K, thr=thr, logits=logits, deltas=deltas,
              anchors=anchors)


def _fuzz_case(seed, img_units=(1, 4), Ks=(1, 3, 8, 20, 50, 120), first_level=None, B=None, ninf=0.0, pinf=0.0):
  """Seed parity picks the graph; 1..5 consecutive levels from a random one (or first_level); image 16 * img_units px a
  side, levels of ceil(side / stride) cells."""
  rng = np.random.default_rng(seed)
  graph = ODT_GRAPH_MULTI if seed % 2 else ODT_GRAPH_SINGLE
  nb = int(rng.integers(1, 4))
  if B is None:
    B = nb if graph == ODT_GRAPH_MULTI else 1
  l0 = int(rng.integers(0, 5))
  if first_level is not None:
    l0 = first_level
  levels = range(l0, l0 + int(rng.integers(1, 6 - l0)))
  H, W = (16 * int(rng.integers(img_units[0], img_units[1] + 1)) for _ in range(2))
  hw_levels = [(-(-H // STRIDES[l]), -(-W // STRIDES[l])) for l in levels]
  K = int(rng.choice(Ks)); thr = float(rng.choice([0.3, 0.5, 0.7]))
  shift = float(rng.choice([0, 0, 1, 3]))
  return _case(graph, B, levels, hw_levels, (H, W), K, thr, rng, shift, ninf, pinf)


def _oracle(case):
  """The restatements of the two graphs in tests/test_ops.py -> list of [n_b, 4]."""
  args = (case["logits"], case["deltas"], case["anchors"], case["img_hw"], case["K"], case["thr"], CLIP)
  with np.errstate(invalid="ignore", over="ignore"):
    if case["graph"] == ODT_GRAPH_SINGLE:
      return [_oracle_proposals_single(*args)]
    return _oracle_proposals_multi(*args)


def _oracle_traced(case):
  """_oracle(case) and, for _events, what the oracle decided on the way: one dict per (level, image) with scores (all logits
  of the level), nms_in (NMS candidates), kept, kept_scores (NMS survivors), and valid (SINGLE: the size filter over the
  top-k) or picked_pad (MULTI: how many of the image's merged top-K rows are this level's zero padding).  Read from the
  oracle's own per-level calls, og.rpn_proposals_level_b1 and tfops.combined_non_max_suppression, in level order."""
  K, B, logits = case["K"], case["B"], case["logits"]
  calls = []
  real_level, real_cnms = og.rpn_proposals_level_b1, tfops.combined_non_max_suppression

  def level(*args, **kw):
    out = real_level(*args, **kw)
    calls.append(out)
    return out

  def cnms(boxes, scores, *args, **kw):
    out = real_cnms(boxes, scores, *args, **kw)
    calls.append((np.asarray(scores, F), out))
    return out
  og.rpn_proposals_level_b1, tfops.combined_non_max_suppression = level, cnms
  try:
    ref = _oracle(case)
  finally:
    og.rpn_proposals_level_b1, tfops.combined_non_max_suppression = real_level, real_cnms
  assert len(calls) == len(logits)
  trace = []
  if case["graph"] == ODT_GRAPH_SINGLE:
    for l, (_, s, info) in enumerate(calls):
      trace.append(dict(level=l, image=0, scores=logits[l][0].reshape(-1), valid=info["valid"],
                        nms_in=int((info["nms_in_scores"] > -np.inf).sum()), kept=int(s.size), kept_scores=s))
    return ref, trace
  cs = np.concatenate([ns for _, (_, ns, _, _) in calls], 1)                  # [B, L * K]: the merge's input
  for b in range(B):
    tk = tfops.top_k(cs[b], min(cs.shape[1], K))
    for l, (ss, (_, ns, _, nv)) in enumerate(calls):
      n = int(nv[b])
      trace.append(dict(level=l, image=b, scores=logits[l][b].reshape(-1), nms_in=int((ss[b] > -np.inf).sum()), kept=n,
                        kept_scores=ns[b, :n], picked_pad=int(((tk // K == l) & (tk % K >= n)).sum())))
  return ref, trace


def _check(lib, case, ref):
  """No tolerance anywhere: the count, the proposals and the zero tail."""
  rpn = [_pack(lg, dl) for lg, dl in zip(case["logits"], case["deltas"])]
  props, nprops = ops.proposals(case["graph"], rpn, case["anchors"], case["img_hw"], case["K"], case["thr"], CLIP, lib=lib)
  tag = {k: case[k] for k in ("graph", "B", "levels", "img_hw", "K", "thr")}
  for b in range(case["B"]):
    n = len(ref[b])
    assert nprops[b] == n, (tag, b, int(nprops[b]), n)
    assert np.array_equal(props[b, :n], ref[b]), (tag, b)
    assert not props[b, n:].any(), (tag, b)


def _events(case, trace):
  """What a case exercises, from the oracle's own intermediate results (any level, any image counts):
  cut      -- a level has more logits than K
  tie      -- the K-th and (K+1)-th logit of a level are equal
  supp     -- NMS suppresses something
  filt     -- SINGLE: the size filter drops a candidate
  mergecut -- the survivors of all levels exceed K
  pad      -- MULTI: the merged top-K holds padding
  zero     -- MULTI: a surviving score is exactly 0 in an image whose levels are padded"""
  K = case["K"]
  ev = dict(cut=False, tie=False, supp=False, filt=False, mergecut=False, pad=False, zero=False)
  for b in range(case["B"]):
    rows = [t for t in trace if t["image"] == b]
    for t in rows:
      s = np.sort(t["scores"])[::-1]
      ev["cut"] |= s.size > K
      ev["tie"] |= s.size > K and s[K - 1] == s[K]
      ev["supp"] |= t["kept"] < t["nms_in"]
      if case["graph"] == ODT_GRAPH_SINGLE:
        ev["filt"] |= not t["valid"].all()
    ev["mergecut"] |= sum(t["kept"] for t in rows) > K
    if case["graph"] == ODT_GRAPH_MULTI:
      ev["pad"] |= any(t["picked_pad"] > 0 for t in rows)
      ev["zero"] |= any(t["kept"] < K for t in rows) and any((t["kept_scores"] == 0).any() for t in rows)
  return ev


# ---- 1. fuzz of the whole stage ---------------------------------------------------------------------------------------------
FUZZ_CHUNKS, FUZZ_CHUNK = 3, 100       # graph = seed parity: 150 cases per graph


@functools.lru_cache(maxsize=None)
def _fuzz(chunk):
  """(cases, oracle results, events) of seeds chunk * 100 .. + 99."""
  cases, refs, evs = [], [], []
  for seed in range(chunk * FUZZ_CHUNK, (chunk + 1) * FUZZ_CHUNK):
    c = _fuzz_case(seed)
    ref, trace = _oracle_traced(c)
    cases.append(c); refs.append(ref); evs.append(_events(c, trace))
  return cases, refs, evs


def test_proposals_fuzz_is_not_vacuous():
  """Over the cases of each graph, each decision the fuzz is there for is taken in at least 5 % of them (_events)."""
  cases, evs = [], []
  for chunk in range(FUZZ_CHUNKS):
    c, _, e = _fuzz(chunk)
    cases += c; evs += e
  for graph, names in ((ODT_GRAPH_SINGLE, ("cut", "tie", "supp", "filt", "mergecut")),
                       (ODT_GRAPH_MULTI, ("cut", "tie", "supp", "mergecut", "pad", "zero"))):
    ge = [e for c, e in zip(cases, evs) if c["graph"] == graph]
    assert len(ge) >= 150
    for name in names:
      share = sum(bool(e[name]) for e in ge) / len(ge)
      print("graph %d %s: %.0f %%" % (graph, name, 100 * share))
      assert share >= 0.05, (graph, name, share)


@pytest.mark.parametrize("chunk", range(FUZZ_CHUNKS))
def test_proposals_fuzz_bit_exact(backend, chunk):
  """Coordinates, clip, operand order; exact-tie order at the per-level top-k, the NMS walk and the cross-level merge; the
  single graph's size filter and ordered compaction; zero-area rows and +-0 scores against the batched graph's padding."""
  name, lib = backend
  cases, refs, _ = _fuzz(chunk)
  for case, ref in zip(cases, refs):
    _check(lib, case, ref)


# ---- 2. K > 1024: rpn_select_kernel rounds, rpn_nms_big_kernel, rpn_merge_kernel<kMaxTopKBig> -------------------------------
BIG_KS = (1025, 1100, 1536, 1537, 2049)      # one past a round; inside the 3rd NMS panel; 3 panels; 3 panels + 1; 2 rounds + 1


def _big_case(seed, K, **kw):
  """P2 of 20 x 20 .. 32 x 32 cells (1 200 .. 3 072 anchors: up to three rounds of 1024, 3..6 NMS panels of 512) and up to
  four levels above it; B = 2 for the batched graph."""
  return _fuzz_case(seed, img_units=(5, 8), Ks=(K,), first_level=0, B=2 if seed % 2 else 1, **kw)


@functools.lru_cache(maxsize=None)
def _big(seed, K):
  case = _big_case(seed, K)
  return case, _oracle(case)


@pytest.mark.parametrize("seed", range(12))
def test_proposals_big_k_bit_exact(backend, seed):
  name, lib = backend
  case, ref = _big(seed, BIG_KS[(seed // 2) % len(BIG_KS)])
  assert 1200 <= case["logits"][0][0].size <= 3072 and case["K"] > 1024
  _check(lib, case, ref)


@GRAPHS
def test_proposals_k_4096(backend, graph):
  """The limit of K, on the same levels."""
  name, lib = backend
  case, ref = _big(100 + graph, 4096)
  assert case["graph"] == graph
  _check(lib, case, ref)


# ---- 3. a level of more than one top-k chunk --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_case(graph):
  """105 x 105 cells = 33 075 logits, just over kSelChunk = 32 768, and a 2 x 2 level; K = 20.  The flat logits
  32 760..32 775, the first four and the last three equal the level's maximum: the tie straddles the chunk border and both
  ends, and lower indices must win it."""
  rng = np.random.default_rng(33075 + graph)
  case = _case(graph, 1, (0, 4), [(105, 105), (2, 2)], (420, 420), 20, 0.7, rng)
  flat = case["logits"][0].reshape(-1)
  assert flat.size == 33075 and flat.base is not None
  top = flat.max()
  flat[32760:32776] = top; flat[:4] = top; flat[-3:] = top
  return case, _oracle(case)


@GRAPHS
def test_proposals_tie_across_the_chunk_border_bit_exact(backend, graph):
  name, lib = backend
  case, ref = _chunk_case(graph)
  _check(lib, case, ref)


# ---- 4. special scores: TF admits an NMS candidate only if score > score_threshold = -inf ------------------------------------
SPECIAL_SEEDS = range(1000, 1020)


@functools.lru_cache(maxsize=None)
def _special():
  """The section 1 generator with 10 % of the logits -inf and 7 % +inf, and two K > 1024 cases of the same."""
  cases = [_fuzz_case(seed, ninf=0.10, pinf=0.07) for seed in SPECIAL_SEEDS]
  cases += [_big_case(seed, 1100, ninf=0.10, pinf=0.07) for seed in (1020, 1021)]
  return cases, [_oracle(c) for c in cases]


def _neg_inf_reaches_nms(case):
  """Some level's top-k holds a -inf logit."""
  return any(np.isneginf(np.sort(lg[b].reshape(-1))[::-1][:case["K"]]).any()
             for lg in case["logits"] for b in range(case["B"]))


def test_proposals_special_scores_bit_exact(backend):
  name, lib = backend
  cases, refs = _special()
  for graph in (ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI):
    hit = [c for c in cases if c["graph"] == graph and _neg_inf_reaches_nms(c)]
    assert len(hit) >= 3 and any(c["K"] > 1024 for c in hit), graph
  for case, ref in zip(cases, refs):
    _check(lib, case, ref)


def _disjoint_boxes(n):
  i = np.arange(n, dtype=F)
  return np.stack([10 * i, 0 * i, 10 * i + 5, 0 * i + 5], 1)


def test_nms_drops_neg_inf_scores(backend):
  """nms_kernel: disjoint boxes, nothing suppressed; the -inf score is no candidate."""
  name, lib = backend
  b = _disjoint_boxes(3)
  s = np.array([1, -np.inf, 0.5], F)
  ref = tfops.non_max_suppression(b, s, 3, 0.5)
  assert ref.tolist() == [0, 2]
  assert ops.nms(b, s, 3, 0.5, lib=lib).tolist() == [0, 2]
  for s in (np.full(3, -np.inf, F), np.array([-np.inf, 2, np.inf], F), np.array([-np.inf], F)):
    ref = tfops.non_max_suppression(b[:s.size], s, 3, 0.5)
    assert np.array_equal(ops.nms(b[:s.size], s, 3, 0.5, lib=lib), ref.astype(np.int32)), s


def test_nms_big_drops_neg_inf_scores(backend):
  """nms_big_kernel (more than 1024 candidates): 30 % of the scores -inf, ties among the rest."""
  name, lib = backend
  rng = np.random.default_rng(1030)
  n = 1030
  ctr = rng.uniform(0, 200, (n // 8, 2))
  c = ctr[rng.integers(0, ctr.shape[0], n)] + rng.normal(0, 6, (n, 2))
  wh = rng.uniform(4, 60, (n, 2))
  b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F)
  s = (rng.integers(0, 40, n) / 8.0).astype(F)
  s[rng.random(n) < 0.3] = -np.inf
  ref = tfops.non_max_suppression(b, s, n, 0.7)
  assert 0 < ref.size < (s > -np.inf).sum()
  assert np.array_equal(ops.nms(b, s, n, 0.7, lib=lib), ref.astype(np.int32))


@GRAPHS
def test_proposals_drop_neg_inf_logits_hand_case(backend, graph):
  """One 2 x 2 x 3 level, K = 12 = every anchor, four logits -inf, nms_thresh 2 (nothing suppressed), zero deltas, all boxes
  of positive area: the eight finite logits are proposed, in score order."""
  name, lib = backend
  lg = np.arange(12, dtype=F).reshape(1, 2, 2, 3) - 6
  lg.reshape(-1)[[1, 4, 6, 11]] = -np.inf
  dl = np.zeros((1, 2, 2, 3, 4), F)
  an = all_anchors(16, [32], RATIOS, 96)
  case = dict(graph=graph, B=1, levels=[2], img_hw=(32, 32), K=12, thr=2.0, logits=[lg], deltas=[dl], anchors=[an])
  ref = _oracle(case)
  assert len(ref[0]) == 8
  _check(lib, case, ref)


# ---- 5. the decode with real expf, suppression off --------------------------------------------------------------------------
E_EXPF = 2        # ulp error tests/test_ops.py attributes to device expf


@functools.lru_cache(maxsize=None)
def _decode_case():
  """Three levels whose logits are one shuffled linspace over (0.1, 5): distinct and positive, so the per-level top-k and
  the merged top-K are unambiguous in both graphs and no padding outranks a proposal.  Centre deltas U(-0.3, 0.3), size
  deltas U(-0.5, clip + 1) with some exactly clip and some one float below / above it.  The image is far larger than the
  anchor field, so only the low clip acts on most boxes and every box keeps a positive width and height.
  Returns (case, clip, reference [K, 4] float64, bound [K, 4])."""
  rng = np.random.default_rng(5)
  levels, hw_levels, img_hw, K = (0, 1, 2), [(12, 16), (6, 8), (3, 4)], (3000, 4000), 150
  clip = F(np.log(224 / 16.0))
  n = [h * w * 3 for h, w in hw_levels]
  lin = rng.permutation(np.linspace(0.1, 5.0, sum(n))).astype(F)
  assert np.unique(lin).size == lin.size
  logits, deltas, anchors, o = [], [], [], 0
  for li, (h, w), m in zip(levels, hw_levels, n):
    logits.append(lin[o:o + m].reshape(1, h, w, 3)); o += m
    dl = np.zeros((1, h, w, 3, 4), F)
    dl[..., :2] = rng.uniform(-0.3, 0.3, dl[..., :2].shape)
    sz = rng.uniform(-0.5, float(clip) + 1, dl[..., 2:].shape).astype(F)
    u = rng.random(sz.shape)
    sz[u < 0.05] = clip
    sz[(u >= 0.05) & (u < 0.10)] = np.nextafter(clip, F(np.inf))
    sz[(u >= 0.10) & (u < 0.15)] = np.nextafter(clip, F(-np.inf))
    dl[..., 2:] = sz
    deltas.append(dl)
    anchors.append(all_anchors(STRIDES[li], [SIZES[li]], RATIOS, 256))
  case = dict(graph=None, B=1, levels=list(levels), img_hw=img_hw, K=K, thr=2.0, logits=logits, deltas=deltas,
              anchors=anchors)
  # the anchors the oracle's top_k picks: per level, then merged
  d, a, s = [], [], []
  for lg, dl, an in zip(logits, deltas, anchors):
    h, w = lg.shape[1:3]
    idx = tfops.top_k(lg.reshape(-1), min(K, lg.size))
    d.append(dl.reshape(-1, 4)[idx]); a.append(an[:h, :w].reshape(-1, 4)[idx]); s.append(lg.reshape(-1)[idx])
  d, a, s = np.concatenate(d), np.concatenate(a), np.concatenate(s)
  assert s.size > K and min(n) < K < max(n)
  tk = tfops.top_k(s, K)
  d, a = d[tk].astype(np.float64), a[tk].astype(np.float64)
  # decode_bbox_target + clip_boxes in float64
  waha = a[:, 2:] - a[:, :2]; xaya = (a[:, 2:] + a[:, :2]) * 0.5
  wbhb = np.exp(np.minimum(d[:, 2:], np.float64(clip))) * waha
  xbyb = d[:, :2] * waha + xaya
  raw = np.concatenate([xbyb - wbhb * 0.5, xbyb + wbhb * 0.5], 1)
  hi = np.array([img_hw[1], img_hw[0]] * 2, np.float64)
  ref = np.minimum(np.maximum(raw, 0), hi)
  assert (ref[:, 2] - ref[:, 0] > 0).all() and (ref[:, 3] - ref[:, 1] > 0).all()
  # conditions on the inputs: the special size deltas are among the picks, and most coordinates are unclipped
  for v in (clip, np.nextafter(clip, F(np.inf)), np.nextafter(clip, F(-np.inf))):
    assert (d[:, 2:] == np.float64(v)).sum() >= 3
  assert (d[:, 2:] > np.float64(clip) + 0.5).any() and (ref == raw).mean() > 0.5
  # |err| <= 2^-24 * (4 * (|d| * wa + |xa|) + (E + 4) * wb / 2), a term count with u = 2^-24.  Centre d * wa + xa: the
  # roundings of wa and of the product cost u * |d| * wa each, that of xa u * |xa|, that of the sum u * (|d| * wa + |xa|):
  # at most 3 of the 4; the 4th is the centre's share of the last rounding, xb -+ wb / 2.  Half size: E for expf, one each
  # for wa, the product and the last rounding's share: E + 3 of the E + 4.  The clip to the image increases no error.
  half = 2.0 ** -24 * (4 * (np.abs(d[:, :2]) * waha + np.abs(xaya)) + (E_EXPF + 4) * wbhb / 2)
  return case, float(clip), ref, np.concatenate([half, half], 1)


@GRAPHS
def test_decode_with_real_expf(backend, graph):
  """expf on general arguments and the decode_clip minimum, apart from any selection decision: nms_thresh = 2 (the
  comparison is a strict iou > thresh and the threshold is not range-checked, so nothing is suppressed), distinct
  positive logits.  Reference: the same decode and clip in float64 on the anchors the oracle's top_k picks; bound per
  coordinate as derived in _decode_case, E = 2."""
  name, lib = backend
  case, clip, ref, bound = _decode_case()
  rpn = [_pack(lg, dl) for lg, dl in zip(case["logits"], case["deltas"])]
  props, nprops = ops.proposals(graph, rpn, case["anchors"], case["img_hw"], case["K"], case["thr"], clip, lib=lib)
  assert nprops[0] == case["K"]
  ratio = np.abs(props[0].astype(np.float64) - ref) / bound
  print("decode %s graph %d: max(err / bound) = %.3f" % (name, graph, ratio.max()))
  assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


# ---- 6. argument limits -----------------------------------------------------------------------------------------------------
def _tiny_call(lib, K, nlevels=1):
  rpn = [np.zeros((1, 1, 1, 16), F)] * nlevels
  an = [all_anchors(64, [512], RATIOS, 64)] * nlevels
  return ops.proposals(ODT_GRAPH_SINGLE, rpn, an, (16, 16), K, 0.7, CLIP, lib=lib)


@pytest.mark.parametrize("K", [0, 4097])
def test_rejects_k_outside_1_4096(backend, K):
  name, lib = backend
  with pytest.raises(OdtError, match=r"rpn_test_post_nms_topk must be in \[1,4096\]"):
    _tiny_call(lib, K)


def test_rejects_six_levels(backend):
  name, lib = backend
  with pytest.raises(OdtError, match="odt_op_proposals: bad argument"):
    _tiny_call(lib, 8, nlevels=6)
