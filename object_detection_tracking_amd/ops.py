"""numpy-in / numpy-out wrappers of the stand-alone op entry points of the C ABI
(include/odt.h ``odt_op_*``).  Each runs exactly the HIP kernels ``odt_forward``
uses; the staged parity tests call the kernels through these.  ``lib`` defaults
to the product library (libodt_hip.so, GPU required).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RPN_CH, c_float_p, f32, fptr, i32, iptr


def _L(lib):
  return lib if lib is not None else _lib.get_lib()


def conv2d(x_nhwc, w_hwio, bias=None, stride=1, dil=1, pad_t=0, pad_l=0, out_hw=None,
           out_off=(0, 0), res=None, res_mode=0, relu=False, lib=None, device=0):
  """reference nn.py:337-381 (+ folded-BN bias, residual, ReLU epilogue)."""
  lib = _L(lib)
  x = f32(x_nhwc); w = f32(w_hwio)
  B, H, W, Cin = x.shape
  kh, kw, _, Cout = w.shape
  if out_hw is None:
    ke_h, ke_w = (kh - 1) * dil + 1, (kw - 1) * dil + 1
    out_hw = ((H + 2 * pad_t - ke_h) // stride + 1, (W + 2 * pad_l - ke_w) // stride + 1)
  Ho, Wo = out_hw
  oy, ox = out_off
  out = np.zeros((B, Ho + oy, Wo + ox, Cout), np.float32)
  b = f32(bias) if bias is not None else None
  r = f32(res) if res is not None else None
  lib.check(lib.dll.odt_op_conv2d(device, fptr(x), B, H, W, Cin, fptr(w),
                                  fptr(b) if b is not None else None, kh, kw, Cout, stride, dil,
                                  pad_t, pad_l, Ho, Wo, oy, ox,
                                  fptr(r) if r is not None else None, res_mode, int(relu),
                                  fptr(out)))
  return out


def conv2d_cat(a, b2, wa, wb, bias=None, stride_b=1, relu=False, lib=None, device=0):
  """1x1 conv over the K-concatenation [a | b2[:, ::stride_b, ::stride_b]] (fused conv3 +
  convshortcut, reference nn.py:503-521)."""
  lib = _L(lib)
  a = f32(a); b2 = f32(b2); wa = f32(wa); wb = f32(wb)
  B, Ho, Wo, Ca = a.shape
  _, Hb, Wb, Cb = b2.shape
  Cout = wa.shape[1]
  out = np.zeros((B, Ho, Wo, Cout), np.float32)
  bb = f32(bias) if bias is not None else None
  lib.check(lib.dll.odt_op_conv2d_cat(device, fptr(a), B, Ho, Wo, Ca, fptr(b2), Hb, Wb, Cb, stride_b,
                                      fptr(wa), fptr(wb), fptr(bb) if bb is not None else None, Cout,
                                      int(relu), fptr(out)))
  return out


def bottleneck_tail(x, w2, b2, w3, b3, res=None, dil=1, relu3=True, fuse=True, lib=None, device=0):
  """conv2 (3x3, 'SAME', ReLU) -> conv3 (1x1 (+ res), ReLU) of a bottleneck block (reference nn.py:503-521) on the fp16x2
  kernels; fuse=True: conv3 inside the 3x3 kernel (one launch), False: the two launches it replaces."""
  lib = _L(lib)
  x = f32(x); w2 = f32(w2); b2 = f32(b2); w3 = f32(w3); b3 = f32(b3)
  B, H, W, Cc = x.shape
  C3 = w3.shape[1]
  r = f32(res) if res is not None else None
  out = np.zeros((B, H, W, C3), np.float32)
  lib.check(lib.dll.odt_op_bottleneck_tail(device, fptr(x), B, H, W, Cc, fptr(w2), fptr(b2), dil, fptr(w3), fptr(b3), C3,
                                           fptr(r) if r is not None else None, int(relu3), int(fuse), fptr(out)))
  return out


def bottleneck_block(x, w1, b1, w2, b2, w3, b3, fuse=True, lib=None, device=0):
  """relu(conv3(relu(conv2(relu(conv1(x))))) + x): a stride-1 identity bottleneck (reference nn.py:503-521) on the fp16x2
  kernels, x [B,H,W,4C], w1 [4C,C], w2 [3,3,C,C], w3 [C,4C], C = 64; fuse=True: conv_block_kernel (one launch), False: the
  three convs as launches of their own."""
  lib = _L(lib)
  x = f32(x); w1 = f32(w1); b1 = f32(b1); w2 = f32(w2); b2 = f32(b2); w3 = f32(w3); b3 = f32(b3)
  B, H, W, C4 = x.shape
  Cc = w1.shape[1]
  assert C4 == 4 * Cc and w1.shape[0] == C4 and w3.shape == (Cc, C4), (x.shape, w1.shape, w3.shape)
  out = np.zeros((B, H, W, C4), np.float32)
  lib.check(lib.dll.odt_op_bottleneck_block(device, fptr(x), B, H, W, Cc, fptr(w1), fptr(b1), fptr(w2), fptr(b2), fptr(w3),
                                            fptr(b3), int(fuse), fptr(out)))
  return out


def stem(frame_pad, w_hwio, bias, fuse=True, grid=0, lib=None, device=0):
  """conv0 (7x7 stride 2 VALID + bias + ReLU) -> pool0 (3x3 stride 2 max over the top/left zero-padded map) on a padded frame
  tensor [B, Hp, Wp, 3] (reference nn.py:860-896, 784-792), fp16x2 arithmetic; fuse=True: conv_stem_kernel (one launch),
  False: the two launches it replaces.  Returns [B, Hq, Wq, 64]."""
  lib = _L(lib)
  x = f32(frame_pad); w = f32(w_hwio); b = f32(bias)
  B, Hp, Wp, _ = x.shape
  Ho0, Wo0 = (Hp - 7) // 2 + 1, (Wp - 7) // 2 + 1
  Hq, Wq = (Ho0 + 1 - 3) // 2 + 1, (Wo0 + 1 - 3) // 2 + 1
  out = np.zeros((B, Hq, Wq, 64), np.float32)
  lib.check(lib.dll.odt_op_stem(device, fptr(x), B, Hp, Wp, fptr(w), fptr(b), int(fuse), int(grid), fptr(out)))
  return out


CONV_CHOICE_SHAPE = ("B", "H", "W", "Cin", "Cout", "kh", "kw", "stride", "dil", "pad", "Ho", "Wo", "in_Wa", "Cin2", "res_mode", "ranges",
                     "in_ldc", "out_ldc")
CONV_CHOICE_OUT = ("status", "kind", "bm", "bn", "kwr", "splitk", "dstage", "f32_tile", "f32_stages", "f32_fine", "reduce_blocks")


def conv_choice(shape, conv_arith=0, conv_split_family=0, lib=None):
  """odt_op_conv_choice: the kernel the library would run this conv on (host only; the ODT_* knobs are read at the call).
  shape: the CONV_CHOICE_SHAPE values; returns the CONV_CHOICE_OUT fields and the row's name as a dict."""
  lib = lib if lib is not None else _lib.OdtLib(_lib.LIB_HIP_PATH)      # (no device needed: not get_lib())
  s = i32(list(shape)); out = np.zeros(len(CONV_CHOICE_OUT), np.int32)
  assert s.shape == (len(CONV_CHOICE_SHAPE),)
  name = C.create_string_buffer(64)
  lib.check(lib.dll.odt_op_conv_choice(iptr(s), int(conv_arith), int(conv_split_family), iptr(out), name, 64))
  d = dict(zip(CONV_CHOICE_OUT, (int(v) for v in out)))
  d["name"] = name.value.decode()
  return d


def last_conv(lib):
  """odt_op_last_conv: the kernel the calling thread's last stand-alone conv call (conv2d, conv2d_cat, bottleneck_tail,
  bottleneck_block, stem) launched on `lib` -- the CONV_CHOICE_OUT fields and the row's name, as conv_choice returns them."""
  out = np.zeros(len(CONV_CHOICE_OUT), np.int32)
  name = C.create_string_buffer(64)
  lib.check(lib.dll.odt_op_last_conv(iptr(out), name, 64))
  d = dict(zip(CONV_CHOICE_OUT, (int(v) for v in out)))
  d["name"] = name.value.decode()
  return d


def preprocess(frames, pad_t, pad_l, Hp, Wp, lib=None, device=0):
  """reference models.py:340-355 + zero pad; returns [B,Hp,Wp,4]."""
  lib = _L(lib)
  fr = np.ascontiguousarray(frames)
  assert fr.dtype in (np.uint8, np.float32)
  B, H, W, _ = fr.shape
  out = np.zeros((B, Hp, Wp, 4), np.float32)
  lib.check(lib.dll.odt_op_preprocess(device, fr.ctypes.data_as(C.c_void_p),
                                      0 if fr.dtype == np.uint8 else 1, B, H, W, pad_t, pad_l,
                                      Hp, Wp, fptr(out)))
  return out


def maxpool3x3s2(x_nhwc, lib=None, device=0):
  """reference nn.py:890-896."""
  lib = _L(lib)
  x = f32(x_nhwc)
  B, H, W, Cc = x.shape
  out = np.zeros((B, (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, Cc), np.float32)
  lib.check(lib.dll.odt_op_maxpool(device, fptr(x), B, H, W, Cc, fptr(out)))
  return out


def top_k(scores, k, lib=None, device=0):
  lib = _L(lib)
  s = f32(scores).reshape(-1)
  idx = np.zeros((k,), np.int32)
  lib.check(lib.dll.odt_op_topk(device, fptr(s), s.size, k, iptr(idx)))
  return idx


def nms(boxes, scores, max_out, iou_thresh, lib=None, device=0):
  lib = _L(lib)
  b = f32(boxes).reshape(-1, 4); s = f32(scores).reshape(-1)
  idx = np.zeros((max(1, s.size),), np.int32)
  n = C.c_int(0)
  lib.check(lib.dll.odt_op_nms(device, fptr(b), fptr(s), s.size, max_out, iou_thresh, iptr(idx),
                               C.byref(n)))
  return idx[:n.value].copy()


def pack_rpn(logits, deltas):
  """[B,h,w,3] + [B,h,w,3,4] -> the device layout [B,h,w,16]."""
  B, h, w, A = logits.shape
  out = np.zeros((B, h, w, RPN_CH), np.float32)
  out[..., :A] = logits
  out[..., A:A + 4 * A] = np.asarray(deltas, np.float32).reshape(B, h, w, 4 * A)
  return out


def proposals(graph, rpn_levels, anchors, img_hw, K, nms_thresh, decode_clip, lib=None, device=0):
  """generate_fpn_proposals (reference models.py:402-436 / :2458-2522).
  rpn_levels: list of [B,h,w,16]; anchors: list of [S,S,3,4].  -> (props [B,K,4], nprops [B])."""
  lib = _L(lib)
  L = len(rpn_levels)
  rp = [f32(r) for r in rpn_levels]; an = [f32(a) for a in anchors]
  B = rp[0].shape[0]
  hs = i32([r.shape[1] for r in rp]); ws = i32([r.shape[2] for r in rp])
  fs = i32([a.shape[0] for a in an])
  rpp = (c_float_p * L)(*[fptr(r) for r in rp]); anp = (c_float_p * L)(*[fptr(a) for a in an])
  props = np.zeros((B, K, 4), np.float32); nprops = np.zeros((B,), np.int32)
  lib.check(lib.dll.odt_op_proposals(device, graph, B, L, iptr(hs), iptr(ws), iptr(fs), rpp, anp,
                                     int(img_hw[0]), int(img_hw[1]), K, nms_thresh, decode_clip,
                                     fptr(props), iptr(nprops)))
  return props, nprops


def roi_align(feats_nhwc, strides, boxes, box_ind, lib=None, device=0):
  """multilevel_roi_align (reference models.py:465-485) -> ([R,C,7,7], [R,C])."""
  lib = _L(lib)
  ft = [f32(x) for x in feats_nhwc]
  B, _, _, Cc = ft[0].shape
  hs = i32([x.shape[1] for x in ft]); ws = i32([x.shape[2] for x in ft])
  fp = (c_float_p * 4)(*[fptr(x) for x in ft])
  st = f32(strides); bx = f32(boxes).reshape(-1, 4); bi = i32(box_ind)
  R = bx.shape[0]
  out = np.zeros((R, Cc, 7, 7), np.float32); pooled = np.zeros((R, Cc), np.float32)
  lib.check(lib.dll.odt_op_roi_align(device, B, Cc, iptr(hs), iptr(ws), fp, fptr(st), fptr(bx),
                                     iptr(bi), R, fptr(out), fptr(pooled)))
  return out, pooled


SENTINEL_BITS = 0x7F7F7F7F      # what an output element no kernel wrote reads back as (odt_op_roi_align_plan, EfficientDet ops)


def roi_align_plan(allocs, views, Cc, strides, boxes, per_image, count=None, levels=None, level0=2, out_size=7, pack_rows=0,
                   want_amax=False, nhwc=False, nchw=False, pooled=False, lib=None, device=0):
  """The ROIAlign kernel with the parameters the plans give it (one launch_roi_align).  allocs = list of 1..5 whole
  allocations [B,alloc_h,alloc_w,ldc]; views = [(h, w)] of each that the kernel may read, with the first Cc channels;
  boxes [B * per_image,4]; count [B] or None; levels [B * per_image] or None (FPN rule).  nhwc / nchw / pooled choose the
  outputs.  Returns dict(nhwc [R,o,o,C], nchw [R,C,o,o], pooled [R,C], amax uint32 float bits), None where not asked for;
  rows the kernel did not write hold SENTINEL_BITS."""
  lib = _L(lib)
  al = [f32(a) for a in allocs]
  L = len(al); B = al[0].shape[0]
  dims = i32([[h, w, a.shape[1], a.shape[2], a.shape[3]] for (h, w), a in zip(views, al)])
  fp = (c_float_p * L)(*[fptr(a) for a in al])
  st = f32(strides); bx = f32(boxes).reshape(-1, 4)
  R = B * per_image
  assert bx.shape[0] == R and st.size == L
  cnt = i32(count) if count is not None else None
  lv = i32(levels) if levels is not None else None
  assert cnt is None or cnt.size == B
  assert lv is None or lv.size == R
  o = out_size if out_size else 7
  out_nhwc = np.empty((R, o, o, Cc), np.float32) if nhwc else None
  out_nchw = np.empty((R, Cc, o, o), np.float32) if nchw else None
  out_pool = np.empty((R, Cc), np.float32) if pooled else None
  amax = np.zeros(1, np.uint32)
  lib.check(lib.dll.odt_op_roi_align_plan(device, B, Cc, L, iptr(dims), fp, fptr(st), fptr(bx), per_image,
                                          iptr(cnt) if cnt is not None else None, iptr(lv) if lv is not None else None,
                                          level0, out_size, int(pack_rows), int(want_amax), _p(out_nhwc), _p(out_nchw),
                                          _p(out_pool), amax.ctypes.data_as(C.POINTER(C.c_uint32))))
  return dict(nhwc=out_nhwc, nchw=out_nchw, pooled=out_pool, amax=amax[0] if want_amax else None)


def mask_select(logits, labels, valid, per_image, lib=None, device=0):
  """mask head tail (launch_mask_select): logits [B * per_image,14,14,4,ld], labels [B * per_image] 1-based, valid [B]
  -> masks [B * per_image,28,28]."""
  lib = _L(lib)
  lg = f32(logits); lb = i32(labels); vd = i32(valid)
  R, ld, B = lg.shape[0], lg.shape[4], vd.size
  assert lg.shape[1:4] == (14, 14, 4) and R == B * per_image and lb.size == R
  masks = np.empty((R, 28, 28), np.float32)
  lib.check(lib.dll.odt_op_mask_select(device, fptr(lg), ld, iptr(lb), iptr(vd), B, per_image, fptr(masks)))
  return masks


def detections(graph, cls_logits, box_logits, props, nprops, img_hw, reg_weights, decode_clip,
               score_thresh, nms_thresh, per_im, lib=None, device=0):
  """inference tail (reference models.py:828-843, :1258-1304 / :2924-2976).
  cls_logits [B*K,C], box_logits [B*K,C,4] (class 0 ignored), props [B,K,4]."""
  lib = _L(lib)
  pr = f32(props); B, K, _ = pr.shape
  cl = f32(cls_logits); Cn = cl.shape[1]
  bl = f32(box_logits).reshape(B * K, Cn * 4)
  npz = i32(nprops); rw = f32(reg_weights)
  boxes = np.zeros((B, per_im, 4), np.float32); probs = np.zeros((B, per_im), np.float32)
  labels = np.zeros((B, per_im), np.int32); valid = np.zeros((B,), np.int32)
  lib.check(lib.dll.odt_op_detections(device, graph, B, K, Cn, fptr(cl), fptr(bl), fptr(pr),
                                      iptr(npz), int(img_hw[0]), int(img_hw[1]), fptr(rw),
                                      decode_clip, score_thresh, nms_thresh, per_im, fptr(boxes),
                                      fptr(probs), iptr(labels), iptr(valid)))
  return boxes, probs, labels, valid


def class_nms(graph, boxes, scores, per_im, iou_thresh, score_thresh=0.0, ncand=None, lib=None, device=0):
  """The selection half of the tail on caller-supplied data: per-class NMS + merged top ``per_im``
  (tf.image.combined_non_max_suppression for graph ODT_GRAPH_MULTI, nms_return_masks + fastrcnn_predictions for
  ODT_GRAPH_SINGLE).  boxes [B,N,C,4] (or [B,N,1,4], shared by the classes), scores [B,N,C]; ncand [B]: rows of each
  image that are real (default N).  ODT_GRAPH_MULTI scores must be >= 0 (they come from a softmax): the kernels place
  the other images' zero-score padding slots among a class's candidates by that assumption.
  Returns (boxes [B,per_im,4], scores [B,per_im], classes [B,per_im] 0-based, valid [B])."""
  lib = _L(lib)
  sc = f32(scores); B, N, Cn = sc.shape
  bx = f32(boxes)
  if bx.shape[2] == 1 and Cn > 1:
    bx = f32(np.repeat(bx, Cn, axis=2))
  nc = i32(ncand if ncand is not None else np.full((B,), N))
  ob = np.zeros((B, per_im, 4), np.float32); os_ = np.zeros((B, per_im), np.float32)
  ol = np.zeros((B, per_im), np.int32); ov = np.zeros((B,), np.int32)
  lib.check(lib.dll.odt_op_class_nms(device, graph, B, N, Cn, fptr(bx), fptr(sc), iptr(nc), score_thresh, iou_thresh,
                                     per_im, fptr(ob), fptr(os_), iptr(ol), iptr(ov)))
  return ob, os_, ol - 1, ov


def nn_cosine(gallery, seg_offsets, dets, lib=None, device=0):
  """NearestNeighborDistanceMetric.distance, cosine (reference
  deep_sort/nn_matching.py:156-177) -> float64 [T,N]."""
  lib = _L(lib)
  g = f32(gallery); d = f32(dets); s = i32(seg_offsets)
  T = s.size - 1
  N = d.shape[0] if d.ndim == 2 else 0
  cost = np.zeros((T, N), np.float64)
  if T == 0 or N == 0:
    return cost
  lib.check(lib.dll.odt_nn_cosine(device, fptr(g), iptr(s), T, fptr(d), N, d.shape[1],
                                  cost.ctypes.data_as(_lib.c_double_p)))
  return cost


# ---- EfficientDet kernels alone.  Each call reports a write past the end of any buffer it allocated (guard regions).

def _se_args(se_w):
  """(se, mid, w1, b1, w2t, b2) for the fused squeeze, or zeros / Nones without it.  se_w = (w1 [se,ldc], b1 [se],
  w2t [se,ldc], b2 [mid])."""
  if se_w is None:
    return 0, 0, None, None, None, None
  w1, b1, w2t, b2 = (f32(a) for a in se_w)
  return w1.shape[0], b2.shape[0], w1, b1, w2t, b2


def _p(a):
  return fptr(a) if a is not None else None


def dwconv(x, wt, bias, k, stride, pad_t, pad_l, out_hw, act=0, se_w=None, lib=None, device=0):
  """depthwise k x k conv (dwconv_plan + launch_dwconv) of x [B,H,W,ldc] with wt [k*k,ldc], bias [ldc] -> out
  [B,Ho,Wo,ldc].  se_w: the fused squeeze and the gate from its partial sums (see _se_args).  Returns (out, info) or
  (out, mean, gate, info); info = dict(px, nsplit, xcd_bands, cqn) as the plan chose them."""
  lib = _L(lib)
  x = f32(x); wt = f32(wt); bias = f32(bias)
  B, H, W, ldc = x.shape
  Ho, Wo = out_hw
  se, mid, w1, b1, w2t, b2 = _se_args(se_w)
  out = np.empty((B, Ho, Wo, ldc), np.float32)
  mean = np.empty((B, ldc), np.float32) if se_w is not None else None
  gate = np.empty((B, ldc), np.float32) if se_w is not None else None
  info = np.zeros(4, np.int32)
  lib.check(lib.dll.odt_op_dwconv(device, fptr(x), B, H, W, ldc, fptr(wt), fptr(bias), k, stride, pad_t, pad_l, Ho, Wo,
                                  act, 0, None, se, mid, _p(w1), _p(b1), _p(w2t), _p(b2), fptr(out), _p(mean), _p(gate),
                                  iptr(info)))
  info = dict(px=int(info[0]), nsplit=int(info[1]), xcd_bands=int(info[2]), cqn=int(info[3]))
  return (out, info) if se_w is None else (out, mean, gate, info)


def dwconv_maps(maps, wt, bias, k, act=0, lib=None, device=0):
  """the multi-map depthwise launch (batch 1, stride 1, 'SAME' pads k // 2): maps = list of up to 5 [h,w,ldc] arrays.
  Returns ([out_i], info)."""
  lib = _L(lib)
  maps = [f32(m) for m in maps]
  ldc = maps[0].shape[2]
  hw = i32([m.shape[:2] for m in maps])
  x = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in maps]))
  out = np.empty_like(x)
  info = np.zeros(4, np.int32)
  p = k // 2
  lib.check(lib.dll.odt_op_dwconv(device, fptr(x), 1, 0, 0, ldc, fptr(f32(wt)), fptr(f32(bias)), k, 1, p, p, 0, 0, act,
                                  len(maps), iptr(hw), 0, 0, None, None, None, None, fptr(out), None, None, iptr(info)))
  outs, off = [], 0
  for m in maps:
    outs.append(out[off:off + m.size].reshape(m.shape)); off += m.size
  return outs, dict(px=int(info[0]), nsplit=int(info[1]), xcd_bands=int(info[2]), cqn=int(info[3]))


def se_gate(x, mid, se_w, scale=False, lib=None, device=0):
  """squeeze-excite gate from the activations (launch_se_gate) of x [B,H*W,ldc]: returns (mean [B,ldc], gate [B,ldc],
  x * gate [B,HW,ldc] or None, channel-sum pixel splits)."""
  lib = _L(lib)
  x = f32(x)
  B, HW, ldc = x.shape
  w1, b1, w2t, b2 = (f32(a) for a in se_w)
  assert b2.shape[0] == mid
  mean = np.empty((B, ldc), np.float32); gate = np.empty((B, ldc), np.float32)
  scaled = np.empty_like(x) if scale else None
  info = np.zeros(1, np.int32)
  lib.check(lib.dll.odt_op_se_gate(device, fptr(x), B, HW, ldc, mid, w1.shape[0], fptr(w1), fptr(b1), fptr(w2t), fptr(b2),
                                   fptr(mean), fptr(gate), _p(scaled), iptr(info)))
  return mean, gate, scaled, int(info[0])


def bifpn_fuse(inputs, modes, out_hw, pads=None, wsm=None, act=0, lib=None, device=0):
  """BiFPN node input fusion (launch_bifpn_fuse): inputs = list of 1..3 [B,h,w,ldc] arrays, modes[k] 0 same size /
  1 nearest resize / 2 3x3 s2 'SAME' max pool (pads[k] = (top, left)), wsm = raw 'fastattn' scalars or None (sum)."""
  lib = _L(lib)
  ins = [f32(a) for a in inputs]
  n = len(ins)
  B, _, _, ldc = ins[0].shape
  h, w = out_hw
  arr = (c_float_p * 3)(*[fptr(a) for a in ins])
  hw = i32([a.shape[1:3] for a in ins])
  md = i32(modes)
  pd = i32(pads if pads is not None else [(0, 0)] * n)
  ws = f32(wsm) if wsm is not None else None
  out = np.empty((B, h, w, ldc), np.float32)
  lib.check(lib.dll.odt_op_bifpn_fuse(device, n, arr, iptr(hw), iptr(md), iptr(pd), _p(ws), act, B, h, w, ldc, fptr(out)))
  return out


def mbconv_expand_dw(x, e_wt, e_bias, dw_wt, dw_bias, k, stride, pad_t, pad_l, out_hw, se_w=None, lib=None, device=0):
  """the fused MBConv front half (launch_mbconv_expand_dw) of x [B,H,W,in_ldc]: e_wt [mid,in_ldc], e_bias [mid],
  dw_wt [k*k,lmid], dw_bias [lmid] -> out [B,Ho,Wo,lmid] (+ mean, gate with se_w).  Returns (out, [mean, gate,] nsplit)."""
  lib = _L(lib)
  x = f32(x); e_wt = f32(e_wt); e_bias = f32(e_bias); dw_wt = f32(dw_wt); dw_bias = f32(dw_bias)
  B, H, W, in_ldc = x.shape
  mid, lmid = e_wt.shape[0], dw_wt.shape[1]
  Ho, Wo = out_hw
  se, _, w1, b1, w2t, b2 = _se_args(se_w)
  out = np.empty((B, Ho, Wo, lmid), np.float32)
  mean = np.empty((B, lmid), np.float32) if se_w is not None else None
  gate = np.empty((B, lmid), np.float32) if se_w is not None else None
  info = np.zeros(1, np.int32)
  lib.check(lib.dll.odt_op_mbconv_expand_dw(device, fptr(x), B, H, W, in_ldc, fptr(e_wt), fptr(e_bias), mid, lmid,
                                            fptr(dw_wt), fptr(dw_bias), k, stride, pad_t, pad_l, Ho, Wo, se, _p(w1), _p(b1),
                                            _p(w2t), _p(b2), fptr(out), _p(mean), _p(gate), iptr(info)))
  return (out, int(info[0])) if se_w is None else (out, mean, gate, int(info[0]))


def effdet_post(cls, box, anchors, ncls, k, max_out, score_thresh=0.0, iou_thresh=0.5, image_scale=1.0, lib=None,
                device=0):
  """the EfficientDet detection tail (launch_effdet_post): cls / box = 5 per-level [B,npix,ldc_cls] / [B,npix,ldc_box]
  arrays (9 * ncls / 36 valid channels), anchors [N,4].  Returns a dict: cand_idx, cand_boxes, cand_scores, cand_cls,
  cand_lvl ([B,k(,4)]) and boxes, scores, labels, levels ([B,max_out(,4)]), valid [B]."""
  lib = _L(lib)
  cls = [f32(a) for a in cls]; box = [f32(a) for a in box]
  B, _, ldc_cls = cls[0].shape
  ldc_box = box[0].shape[2]
  npix = i32([a.shape[1] for a in cls])
  an = f32(anchors)
  r = dict(cand_idx=np.empty((B, k), np.int32), cand_boxes=np.empty((B, k, 4), np.float32),
           cand_scores=np.empty((B, k), np.float32), cand_cls=np.empty((B, k), np.int32),
           cand_lvl=np.empty((B, k), np.int32), boxes=np.empty((B, max_out, 4), np.float32),
           scores=np.empty((B, max_out), np.float32), labels=np.empty((B, max_out), np.int32),
           levels=np.empty((B, max_out), np.int32), valid=np.empty(B, np.int32))
  lib.check(lib.dll.odt_op_effdet_post(device, B, ncls, iptr(npix), ldc_cls, ldc_box, (c_float_p * 5)(*[fptr(a) for a in cls]),
                                       (c_float_p * 5)(*[fptr(a) for a in box]), fptr(an), k, max_out, score_thresh,
                                       iou_thresh, image_scale, iptr(r["cand_idx"]), fptr(r["cand_boxes"]),
                                       fptr(r["cand_scores"]), iptr(r["cand_cls"]), iptr(r["cand_lvl"]), fptr(r["boxes"]),
                                       fptr(r["scores"]), iptr(r["labels"]), iptr(r["levels"]), iptr(r["valid"])))
  return r


def preprocess_rgb(frames, pad_t, pad_l, Hp, Wp, resize_hw=None, lib=None, device=0):
  """the EfficientDet preprocess of BGR frames [B,Hs,Ws,3] (uint8 or float32) -> normalised RGB [B,Hp,Wp,4], zero
  padded; resize_hw = (Hr, Wr): the on-device bilinear resize first."""
  lib = _L(lib)
  dtype = _lib.ODT_DTYPE_U8 if frames.dtype == np.uint8 else _lib.ODT_DTYPE_F32
  fr = np.ascontiguousarray(frames if dtype == _lib.ODT_DTYPE_U8 else frames.astype(np.float32))
  B, Hs, Ws, _ = fr.shape
  Hr, Wr = resize_hw if resize_hw is not None else (0, 0)
  out = np.empty((B, Hp, Wp, 4), np.float32)
  lib.check(lib.dll.odt_op_preprocess_rgb(device, fr.ctypes.data_as(C.c_void_p), dtype, B, Hs, Ws, Hr, Wr, pad_t, pad_l,
                                          Hp, Wp, int(resize_hw is not None), fptr(out)))
  return out


def mask_rle(masks, boxes, frame_hw, scale=1.0, want_counts=False, device_ptrs=None, lib=None, device=0):
  """odt_op_mask_rle: masks [n,28,28] (final_masks) and boxes [n,4] (network coordinates) -> the COCO RLE of each mask
  pasted into a frame_hw = (H0, W0) frame at boxes / scale, as [{"size": [H0, W0], "counts": str}] (fill_full_mask +
  pycocotools mask.encode, include/odt.h); want_counts: (rles, [uint32 counts per detection]).  device_ptrs = (masks_ptr,
  boxes_ptr, n): inputs already on the device (masks / boxes are then ignored)."""
  lib = _L(lib)
  res = _lib.OdtRleResult()
  if device_ptrs is not None:
    pm, pb, n = device_ptrs
    keep = None
    lib.check(lib.dll.odt_op_mask_rle(device, C.c_void_p(pm), C.c_void_p(pb), int(n), 1, int(frame_hw[0]), int(frame_hw[1]),
                                      float(scale), int(bool(want_counts)), C.byref(res)))
  else:
    m = f32(masks).reshape(-1, 28, 28)
    b = f32(boxes).reshape(-1, 4)
    assert m.shape[0] == b.shape[0], (m.shape, b.shape)
    keep = (m, b)
    lib.check(lib.dll.odt_op_mask_rle(device, m.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), m.shape[0], 0,
                                      int(frame_hw[0]), int(frame_hw[1]), float(scale), int(bool(want_counts)),
                                      C.byref(res)))
  del keep
  rles = res.rles()
  return (rles, res.count_lists()) if want_counts else rles


def se_fold(w3, b3, fc1_w, fc1_b):
  """conv3 + BN folded into the SE gate's first layer (mean_HW commutes with a 1x1 conv and an affine BN): w3 [ch, 4 ch] with
  the BN scale folded in, b3 [4 ch] the BN shift -> (w1 [r][ch], b1 [r]) in float64, rounded to float32 once -- what the plan
  does at build time (csrc/plan_common.hip upload_se_gate)."""
  w3 = np.asarray(w3, np.float64); f1 = np.asarray(fc1_w, np.float64)
  w1 = (w3 @ f1).T
  b1 = np.asarray(b3, np.float64) @ f1 + np.asarray(fc1_b, np.float64)
  return f32(w1), f32(b1)


def rse_gate(t2, w1, b1, w2t, b2, lib=None, device=0):
  """SE-ResNet gate as the plan runs it: t2 [B,H,W,ch] -> spatial mean -> relu(. w1 + b1) (w1 [r][ch]) -> sigmoid(. w2t + b2)
  (w2t [r][cout]).  Returns (mean [B,ch], gate [B,cout])."""
  lib = _L(lib)
  t2 = f32(t2); w1 = f32(w1); b1 = f32(b1); w2t = f32(w2t); b2 = f32(b2)
  B, ch = t2.shape[0], t2.shape[-1]
  HW = t2.size // (B * ch)
  r, cout = w2t.shape
  assert w1.shape == (r, ch) and b1.shape == (r,) and b2.shape == (cout,)
  mean = np.empty((B, ch), np.float32); gate = np.empty((B, cout), np.float32)
  lib.check(lib.dll.odt_op_rse_gate(device, fptr(t2), B, HW, ch, r, cout, fptr(w1), fptr(b1), fptr(w2t), fptr(b2), fptr(mean),
                                    fptr(gate)))
  return mean, gate


def rse_apply(y, gate, shortcut, C=None, in_place=False, out_init=None, lib=None, device=0):
  """out = max(y * gate[b, c] + shortcut, 0) over the first C channels of [B,...,ldc] tensors (gate [B,ldc]); channels [C, ldc)
  of the result keep what out_init holds (default zeros).  Returns (out, recorded |max| of out)."""
  lib = _L(lib)
  y = f32(y); s = f32(shortcut); g = f32(gate)
  B, ldc = y.shape[0], y.shape[-1]
  HW = y.size // (B * ldc)
  C = ldc if C is None else int(C)
  assert s.shape == y.shape and g.shape == (B, ldc)
  out = np.zeros(y.shape, np.float32) if out_init is None else f32(out_init).copy()
  amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_rse_apply(device, fptr(y), fptr(g), fptr(s), B, HW, C, ldc, int(bool(in_place)), fptr(out), fptr(amax)))
  return out, float(amax[0])


def group_conv(x, w, bias, stride=1, dil=1, pad=None, out_hw=None, relu=True, lib=None, device=0):
  """3x3 convolution in 32 groups (ResNeXt-32x4d conv2; csrc/conv_group.hip): x [B,H,W,C], C in {128, 256, 512, 1024}, w
  grouped HWIO [3,3,C/32,C], bias [C].  pad = (top, left) zeros in front and out_hw = (Ho, Wo) default to TensorFlow's
  'SAME' (out = ceil(in / stride), the smaller half of the padding in front); taps past H x W read zero.  Returns
  (out [B,Ho,Wo,C], recorded |max| of out)."""
  lib = _L(lib)
  x = f32(x); w = f32(w); bias = f32(bias)
  B, H, W, C = x.shape
  assert w.shape == (3, 3, C // 32, C) and bias.shape == (C,)
  keff = 2 * dil + 1
  same = [((n + stride - 1) // stride, max(((n + stride - 1) // stride - 1) * stride + keff - n, 0) // 2) for n in (H, W)]
  Ho, Wo = out_hw if out_hw is not None else (same[0][0], same[1][0])
  pt, pl = pad if pad is not None else (same[0][1], same[1][1])
  out = np.empty((B, Ho, Wo, C), np.float32); amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_group_conv(device, fptr(x), B, H, W, C, fptr(w), fptr(bias), int(stride), int(dil), int(pt), int(pl),
                                      int(Ho), int(Wo), int(bool(relu)), fptr(out), fptr(amax)))
  return out, float(amax[0])


def deform_conv(x, w_off, b_off, w, lib=None, device=0, view=None):
  """The deformable conv2 of a --use_deformable stage entry (csrc/conv_deform.hip; reference nn.py:469-485, 1642-1712): x
  [B,H,W,C], C in {128, 256, 512}; w_off [3,3,C,18] + b_off [18] give the offsets at the even positions (a 3x3 stride-2 conv
  with one zero row / column in front; channel 2 n the row offset, 2 n + 1 the column offset of tap n = 3 ky + kx); w
  [3,3,C,C] multiplies the nine bilinear samples at the clamped coordinates.  Returns (out [B,ceil(H/2),ceil(W/2),C], recorded
  |max| of out, offsets [B,ceil(H/2),ceil(W/2),18]).  With view = (H, W, C), x is an allocation [B,Ha,Wa,ldc] of which the op reads
  rows < H, columns < W and channels < C, as the plan reads a pitched tensor."""
  lib = _L(lib)
  x = f32(x); w_off = f32(w_off); b_off = f32(b_off); w = f32(w)
  B, Ha, Wa, ldc = x.shape
  H, W, C = (Ha, Wa, ldc) if view is None else view
  assert w_off.shape == (3, 3, C, 18) and b_off.shape == (18,) and w.shape == (3, 3, C, C)
  Ho, Wo = (H + 1) // 2, (W + 1) // 2
  out = np.empty((B, Ho, Wo, C), np.float32); off = np.empty((B, Ho, Wo, 18), np.float32); amax = np.zeros(1, np.float32)
  if view is None:
    lib.check(lib.dll.odt_op_deform_conv(device, fptr(x), B, H, W, C, fptr(w_off), fptr(b_off), fptr(w), fptr(out), fptr(amax), fptr(off)))
  else:
    lib.check(lib.dll.odt_op_deform_conv_view(device, fptr(x), B, Ha, Wa, ldc, H, W, C, fptr(w_off), fptr(b_off), fptr(w), fptr(out),
                                              fptr(amax), fptr(off)))
  return out, float(amax[0]), off


def group_norm(x, gamma, beta, eps=1e-5, relu=False, res=None, upsample=False, view=None, offset=(0, 0), chunks=0, out_init=None,
               lib=None, device=0):
  """GroupNorm as a --use_gn plan runs it (csrc/group_norm.hip; reference nn.py:81-108): x [B,H,W,C], C % 32 == 0, 32 groups of
  adjacent channels; per image and group mean and biased variance over all positions, a = rsqrt(var + eps) * gamma[c],
  out = x * a + (beta[c] - mean * a), + res ([B,H,W,C], or [B,ceil(H/2),ceil(W/2),C] nearest-2x upsampled with upsample=True),
  ReLU if relu.  With view = (h, w, C), x is an allocation [B,Ha,Wa,ldc] of which the op normalises h rows, w columns and C
  channels starting at offset = (oy, ox), as the plan reads a pitched tensor or writes the interior of a zero-bordered one; out
  has x's shape and keeps what out_init holds (default zeros) outside the view.  chunks: row ranges of the statistics pass (0:
  the launcher's choice).  Returns (out, recorded |max| of out, mean [B,32], var [B,32])."""
  lib = _L(lib)
  x = f32(x); gamma = f32(gamma); beta = f32(beta)
  B, Ha, Wa, ldc = x.shape
  h, w, C = (Ha, Wa, ldc) if view is None else view
  oy, ox = offset
  assert gamma.shape == (C,) and beta.shape == (C,)
  mode, rH, rW, rp = 0, 0, 0, None
  if res is not None:
    res = f32(res)
    mode = 2 if upsample else 1
    rH, rW = res.shape[1:3]
    assert res.shape == (B, rH, rW, C)
    rp = fptr(res)
  out = np.zeros(x.shape, np.float32) if out_init is None else f32(out_init).copy()
  assert out.shape == x.shape
  amax = np.zeros(1, np.float32); mean = np.empty((B, 32), np.float32); var = np.empty((B, 32), np.float32)
  lib.check(lib.dll.odt_op_group_norm(device, fptr(x), B, Ha, Wa, ldc, int(h), int(w), int(C), int(oy), int(ox), fptr(gamma), fptr(beta),
                                      float(eps), int(bool(relu)), mode, rp, int(rH), int(rW), int(chunks), fptr(out), fptr(amax),
                                      fptr(mean), fptr(var)))
  return out, float(amax[0]), mean, var


def group_norm_roi(x, gamma, beta, eps=1e-5, view=None, out_init=None, lib=None, device=0):
  """GroupNorm of a RoI tensor as the 4-conv box head runs it under --use_gn (csrc/group_norm_roi.hip): x [R,h,w,C], h * w <= 64,
  C % 32 == 0 in [32, 512]; per RoI and group of C / 32 adjacent channels the arithmetic of group_norm, in one launch and one
  pass, with no residual and no activation.  With view = C, x is an allocation [R,h,w,ldc] of which the first C channels are
  normalised; out has x's shape and keeps what out_init holds (default zeros) past them.  Returns (out, recorded |max| of out,
  mean [R,32], var [R,32])."""
  lib = _L(lib)
  x = f32(x); gamma = f32(gamma); beta = f32(beta)
  R, h, w, ldc = x.shape
  C = ldc if view is None else int(view)
  assert gamma.shape == (C,) and beta.shape == (C,)
  out = np.zeros(x.shape, np.float32) if out_init is None else f32(out_init).copy()
  assert out.shape == x.shape
  amax = np.zeros(1, np.float32); mean = np.empty((R, 32), np.float32); var = np.empty((R, 32), np.float32)
  lib.check(lib.dll.odt_op_group_norm_roi(device, fptr(x), R, h, w, ldc, C, fptr(gamma), fptr(beta), float(eps), fptr(out), fptr(amax),
                                          fptr(mean), fptr(var)))
  return out, float(amax[0]), mean, var


def relation_geo(boxes, n, geo_emb, geo_conv, bias_init=None, lib=None, device=0):
  """The geometric bias of a relation module as the box head runs it under --add_relation_nn (csrc/relation.hip; reference
  nn.py:115-143, 273-298): boxes [K,4] (x1, y1, x2, y2), of which the first n are real; geo_emb = (W [4,64], b [64]), geo_conv =
  (W [1,1,64,16] or [64,16], b [16]).  Returns bias [16, K, Kp] with Kp = K rounded up to 4: bias[h, i, j] =
  log(max(relu(a[i, j, h]), 1e-6)) for i, j < n; every other entry keeps what bias_init holds (default zeros)."""
  lib = _L(lib)
  boxes = f32(boxes)
  K = boxes.shape[0]
  assert boxes.shape == (K, 4)
  wts = np.concatenate([f32(geo_emb[0]).reshape(-1), f32(geo_emb[1]).reshape(-1), f32(geo_conv[0]).reshape(-1),
                        f32(geo_conv[1]).reshape(-1)])
  assert wts.size == 1360, wts.size
  Kp = (K + 3) // 4 * 4
  bias = np.zeros((16, K, Kp), np.float32) if bias_init is None else f32(bias_init).copy()
  assert bias.shape == (16, K, Kp)
  lib.check(lib.dll.odt_op_relation_geo(device, fptr(boxes), K, int(n), fptr(wts), fptr(bias)))
  return bias


def relation_attention(q, k, v, bias, n, out_init=None, lib=None, device=0):
  """The attention of a relation module (csrc/relation.hip; reference nn.py:146-183): q, k, v [K, D] with 16 heads of D / 16
  columns in q and k, bias [16, K, Kp], of all of which the first n rows / columns are real and the rest is never read.  Returns
  (out, recorded |max| of out): out[i, h, :] = sum_j softmax_j(q_h[i] . k_h[j] / sqrt(D / 16) + bias[h, i, j]) v[j, :] for i < n
  and zeros for n <= i < K.  out_init (flat, at least K * 16 * D floats; default zeros of exactly that size) is the buffer the
  kernel writes into: the flat result comes back whole, so that a caller can see that nothing past [K,16,D] changed."""
  lib = _L(lib)
  q = f32(q); k = f32(k); v = f32(v); bias = f32(bias)
  K, D = q.shape
  assert k.shape == (K, D) and v.shape == (K, D) and bias.shape == (16, K, (K + 3) // 4 * 4)
  out = np.zeros(K * 16 * D, np.float32) if out_init is None else f32(out_init).reshape(-1).copy()
  amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_relation_attention(device, fptr(q), fptr(k), fptr(v), fptr(bias), K, D, int(n), fptr(out), out.size,
                                              fptr(amax)))
  return (out.reshape(K, 16, D) if out_init is None else out), float(amax[0])


def att_pool(x, lib=None, device=0):
  """The sum over a RoI's positions as the box head's attention branch runs it under --use_att_frcnn_head (csrc/att_head.hip;
  reference models.py:1064-1081, whose one-channel softmax map is 1): x [R,49,C] (or [R,7,7,C]), C % 4 == 0.  Returns (out [R,C],
  recorded |max| of out); out[r, c] is the 49 values added to +0 one after another in row-major order, in float32."""
  lib = _L(lib)
  x = f32(x)
  R, C = x.shape[0], x.shape[-1]
  assert x.size == R * 49 * C, x.shape
  out = np.empty((R, C), np.float32); amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_att_pool(device, fptr(x), R, C, fptr(out), fptr(amax)))
  return out, float(amax[0])


def att_add(h, a, view=None, lib=None, device=0):
  """hidden + attended_feat of the same branch (reference models.py:1089): h [R,ldh], of which the first D = view (default ldh)
  columns are the hidden vector, a [R,D], D % 4 == 0.  Returns (out [R,D], recorded |max| of out)."""
  lib = _L(lib)
  h = f32(h); a = f32(a)
  R, ldh = h.shape
  D = ldh if view is None else int(view)
  assert a.shape == (R, D), (a.shape, R, D)
  out = np.empty((R, D), np.float32); amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_att_add(device, fptr(h), ldh, fptr(a), R, D, fptr(out), fptr(amax)))
  return out, float(amax[0])


def se_tail(t2, w3, b3, fc1, fc2, shortcut, lib=None, device=0):
  """The tail of an SE bottleneck (reference nn.py:502-521) as the plan runs it: pool of t2 [B,H,W,ch] -> gate (conv3 + BN
  folded into fc1 = (W [4 ch, ch / 4], b), fc2 = (W [ch / 4, 4 ch], b)) -> conv3 (w3 [ch, 4 ch] with BN folded, + b3) ->
  max(conv3 * gate + shortcut, 0).  Returns (out [B,H,W,4 ch], gate [B,4 ch], recorded |max| of out)."""
  lib = _L(lib)
  t2 = f32(t2); w3 = f32(w3); b3 = f32(b3); s = f32(shortcut)
  B, H, W, ch = t2.shape
  C3 = w3.shape[1]
  assert C3 == 4 * ch and s.shape == (B, H, W, C3)
  w1, b1 = se_fold(w3, b3, fc1[0], fc1[1])
  w2t = f32(fc2[0]); b2 = f32(fc2[1])
  assert w2t.shape == (ch // 4, C3)
  out = np.empty((B, H, W, C3), np.float32); gate = np.empty((B, C3), np.float32); amax = np.zeros(1, np.float32)
  lib.check(lib.dll.odt_op_se_tail(device, fptr(t2), B, H, W, ch, fptr(w3), fptr(b3), fptr(w1), fptr(b1), fptr(w2t), fptr(b2),
                                   fptr(s), fptr(out), fptr(gate), fptr(amax)))
  return out, gate, float(amax[0])
