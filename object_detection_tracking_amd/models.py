"""Host-side mirror of the reference's model surface for the hot path.

The reference builds a TF1 graph once and exposes tensor *handles*
(``model.final_boxes`` ...) that callers fetch with ``sess.run(handles,
feed_dict)`` (reference models.py:97-119 ``get_model``, :965-973 output
identities, :1629-1636 ``get_feed_dict_forward``, :3301
``get_feed_dict_forward_multi``; call sites obj_detect_tracking.py:505-517,
:610-635 and obj_detect_tracking_multi.py:460-467).  This module keeps exactly
that surface -- same factory, same attribute names, same feed-dict methods,
same output dtypes/shapes -- over the C ABI of libodt_hip.so, and adds the
plain ``predict()`` / ``predict_batch()`` calls BASELINE.json asks for.

There is no CPU path: constructing a model without the HIP library or without a
GPU raises.
"""
from __future__ import annotations

import collections
import copy
import ctypes as C
import functools
import itertools
import os

import numpy as np

from . import _lib
from ._lib import (ODT_DTYPE_F32, ODT_DTYPE_U8, ODT_GRAPH_MULTI, ODT_GRAPH_SINGLE, OdtConfig, OdtOutputs, _Handle, as_frames,
                   fptr, iptr)
from .anchors import fpn_anchor_fields
from .config import HEAD_DECODE_CLIP, finalize_config
from .nn import get_new_hw
from .range_guard import RangeGuard
from .frozen_pb import load_frozen_pb
from .tf_checkpoint import load_checkpoint
from .weights import (att_head_variables, backbone_block_kind, conv_head_variables, deformable_groups, expand_class_agnostic_box, group_norm_variables, load_npz,
                      relation_variables, select_partial_classes)


class TensorHandle(object):
  """Opaque stand-in for a TF tensor handle (fetch key for Session.run)."""

  def __init__(self, model, name):
    self.model = model
    self.name = name

  def __repr__(self):
    return "<odt tensor %s:0>" % self.name


class _Graph(object):
  """The part of ``tf.Graph`` the frozen-model route uses: tensors by name (reference
  models.py:219-238 ``self.graph.get_tensor_by_name("%s/final_boxes:0" % var_prefix)``)."""

  def __init__(self):
    self._tensors = {}

  def _register(self, prefix, handle):
    self._tensors["%s/%s:0" % (prefix, handle.name)] = handle

  def _unregister(self, prefix):
    for k in [k for k in self._tensors if k.startswith(prefix + "/")]:
      del self._tensors[k]

  def get_tensor_by_name(self, name):
    if name in self._tensors:
      return self._tensors[name]
    # un-prefixed "final_boxes:0" resolves when exactly one imported model carries it
    hits = [h for k, h in self._tensors.items() if k.split("/", 1)[-1] == name]
    if len(hits) == 1:
      return hits[0]
    raise KeyError("The name %r refers to a Tensor which does not exist%s" %
                   (name, " (ambiguous: %d imported models)" % len(hits) if hits else ""))


_DEFAULT_GRAPH = _Graph()


def get_default_graph():
  return _DEFAULT_GRAPH


class _Engine(object):
  """One static plan (fixed batch, H, W) on one GPU."""

  def __init__(self, lib, config, graph, batch, height, width, weights, device,
               num_class=None):
    self.lib = lib
    self.batch, self.height, self.width = batch, height, width
    self.src_height, self.src_width = height, width
    self.per_im = int(config.result_per_im)
    self.channels = int(config.fpn_num_channel)
    c = OdtConfig()
    c.graph = graph; c.batch = batch; c.height = height; c.width = width
    c.num_class = int(num_class if num_class is not None else config.num_class)
    for i, n in enumerate(config.resnet_num_block):
      c.num_blocks[i] = int(n)
    c.use_dilations = int(bool(config.use_dilations))
    c.fpn_channels = self.channels
    c.head_dim = int(config.fpn_frcnn_fc_head_dim)
    c.rpn_topk = int(config.rpn_test_post_nms_topk)
    c.result_per_im = self.per_im
    c.anchor_field = int(np.ceil(config.max_size / config.anchor_strides[0]))
    c.rpn_nms_thresh = float(config.rpn_proposal_nms_thres)
    c.rpn_decode_clip = float(config.bbox_decode_clip)
    c.head_decode_clip = HEAD_DECODE_CLIP
    for i in range(4):
      c.bbox_reg_weights[i] = float(config.fastrcnn_bbox_reg_weights[i])
    c.result_score_thresh = float(config.result_score_thres)
    c.head_nms_thresh = float(config.fastrcnn_nms_iou_thres)
    self.add_mask = bool(getattr(config, "add_mask", False))
    c.add_mask = int(self.add_mask)
    c.mask_dim = int(getattr(config, "mrcnn_head_dim", 256))
    # arithmetic of the conv / FC products (include/odt.h ODT_ARITH_*): None / "default" | "f32" | "bf16x3"
    arith = getattr(config, "conv_arith", None)
    c.conv_arith = {None: 0, "default": 0, "f32": _lib.ODT_ARITH_F32, "bf16x3": _lib.ODT_ARITH_BF16X3}[arith]
    # conv_split_family: "auto" (the DEFAULT, also for an args object that does not carry the field): start on the fp16x2
    # kernels under a RangeGuard (range_guard.py).  Explicit: 0 / 2 the fp16x2 kernels where eligible, unguarded | 3 bf16x3
    # only | 1 one-stage bf16x3.
    fam = getattr(config, "conv_split_family", "auto")
    fam = "auto" if fam is None else fam
    self._family_requested = fam
    self._guard = None
    if fam == "auto" and c.conv_arith == 0:
      cfg3 = copy.copy(config)
      cfg3.conv_split_family = 3
      self._guard = RangeGuard(config, functools.partial(_Engine, lib, cfg3, graph, batch, height, width, weights, device, num_class))
    if fam == "auto":
      fam = 2
    c.conv_split_family = int(fam)
    # debug / parity runs: every stage tensor keeps its own buffer and tap() can read it after a forward; the production
    # default plans the activations into an arena (a stage's memory is reused once its consumers have run)
    c.keep_taps = int(bool(getattr(config, "keep_taps", False)))
    c.tail_overlap = -1 if getattr(config, "tail_overlap", True) in (False, -1) else 0      # (False: everything on the compute stream)
    c.use_se = int(bool(getattr(config, "use_se", False)))      # model version 6: squeeze-excitation in every bottleneck
    c.block_kind = backbone_block_kind(config)                  # include/odt.h: 0 bottleneck | 1 basic | 2 ResNeXt-32x4d
    c.use_deformable = int(bool(getattr(config, "use_deformable", False)))      # deformable conv2 in the stage-entry bottlenecks
    c.use_gn = int(bool(getattr(config, "use_gn", False)))      # GroupNorm in the backbone and the FPN
    c.use_conv_frcnn_head = int(bool(getattr(config, "use_conv_frcnn_head", False)))      # 4 convs + one FC in place of fc6 / fc7
    c.conv_head_dim = int(getattr(config, "conv_frcnn_head_dim", 256))
    c.add_relation_nn = int(bool(getattr(config, "add_relation_nn", False)))      # RM_r1 / RM_r2 behind fc6 / fc7
    c.use_att_frcnn_head = int(bool(getattr(config, "use_att_frcnn_head", False)))      # hidden + relu(att_trans(pooled RoI)) in front of the outputs
    B, P, Cn = batch, self.per_im, self.channels
    self._boxes = np.zeros((B, P, 4), np.float32)
    self._probs = np.zeros((B, P), np.float32)
    self._labels = np.zeros((B, P), np.int32)
    self._valid = np.zeros((B,), np.int32)
    self._feats = np.zeros((B * P, Cn, 7, 7), np.float32)
    self._pooled = np.zeros((B * P, Cn), np.float32)
    self._masks = np.zeros((B * P, 28, 28), np.float32) if self.add_mask else None
    self._ticket_want = {}           # ticket -> (want_feats, want_pooled) as submitted
    self._ingest_dtype = ODT_DTYPE_U8
    self._ingest_view = None         # numpy view of the pinned buffer armed by ingest_buffer() (until the next submit)
    self._ingest_views_out = False   # a view into this handle's pinned memory was ever handed out
    self._retired = []               # handles replaced by the guard whose pinned memory a caller may still hold
    anchors = (("anchors/lvl%d" % i, a) for i, a in enumerate(fpn_anchor_fields(config)))
    self._handle = _Handle(lib, c, device, itertools.chain(weights.items(), anchors))

  # what needs nothing but the handle (_lib._Handle), on the one the engine runs now
  h = property(lambda self: self._handle.h)      # (None once closed; callers of lib.dll.odt_* read it)
  tap = property(lambda self: self._handle.tap)
  forward_serial = property(lambda self: self._handle.forward_serial)
  profile = property(lambda self: self._handle.profile)
  profile_read = property(lambda self: self._handle.profile_read)
  profile_layers = property(lambda self: self._handle.profile_layers)

  def set_source_size(self, src_height, src_width):
    """Frames of [B, src_height, src_width, 3] from now on; the bilinear resize to the plan's
    [height, width] (reference resizeImage, nn.py:1540-1560) runs on the device."""
    if (src_height, src_width) != (self.src_height, self.src_width):
      self._handle.set_source_size(src_height, src_width)
      self.src_height, self.src_width = int(src_height), int(src_width)
      if self._guard is not None and self._guard.twin is not None:
        self._guard.twin.set_source_size(src_height, src_width)

  def close(self):
    if self._guard is not None:
      self._guard.close()
    for old in self._retired:
      old.close()
    self._retired = []
    self._ingest_view = None
    self._handle.close()

  def _outputs(self, want_feats, want_pooled):
    out = OdtOutputs()
    out.boxes = fptr(self._boxes); out.probs = fptr(self._probs)
    out.labels = iptr(self._labels); out.valid = iptr(self._valid)
    out.feats = fptr(self._feats) if want_feats else None
    out.pooled = fptr(self._pooled) if want_pooled else None
    out.masks = fptr(self._masks) if self.add_mask else None
    return out

  def _result(self, want_feats, want_pooled):
    total = int(self._valid.sum())
    return (self._boxes.copy(), self._labels.copy(), self._probs.copy(), self._valid.copy(),
            self._feats[:total].copy() if want_feats else None,
            self._pooled[:total].copy() if want_pooled else None)

  def _frames(self, frames):
    fr, dt = as_frames(frames)
    assert fr.shape == (self.batch, self.src_height, self.src_width, 3), fr.shape
    return fr, fr.ctypes.data_as(C.c_void_p), dt

  def _calibrate(self, run):
    """Ahead of a forward: the guard's comparison of ``run(e)`` on this engine and its twin, when one is due.  Returns
    True when the engine changed handles."""
    self._handle.live()              # (a closed engine builds no twin)
    return self._guard is not None and self._guard.calibrate(self, run)

  def _forward_blocking(self, src, dt, want_feats=False, want_pooled=False):
    """odt_forward of host frames at ``src``; the guard's comparisons need the detections only."""
    out = self._outputs(want_feats, want_pooled)
    self.lib.check(self.lib.dll.odt_forward(self._handle.live(), src, dt, 0, None, C.byref(out)))

  def take_handle(self, twin):
    """Continue on ``twin``'s handle, which ``twin`` gives up (the guard's change to bf16x3).  State bound to the old
    handle: no tickets (the guard never compares with one outstanding); pinned ingest memory a caller may still hold a
    view of keeps the old handle alive until close(); the profiling switch follows."""
    old, self._handle = self._handle, twin._handle.move()
    if self._ingest_views_out:
      self._retired.append(old)
    else:
      old.close()
    self._ingest_views_out = False
    if old.profiling:
      self._handle.profile(True)

  def _watch(self):
    if self._guard is not None:
      self._guard.after_forward(self)

  def range_health(self, rebase=False):
    return self._handle.range_health(rebase)

  def forward(self, frames, want_feats=True, want_pooled=False):
    """frames: [B,H,W,3] uint8/float32 BGR host array.  Returns fresh arrays."""
    fr, src, dt = self._frames(frames)
    self._calibrate(lambda e: e._forward_blocking(src, dt))
    self._forward_blocking(src, dt, want_feats, want_pooled)
    self._watch()
    return self._result(want_feats, want_pooled)

  def mask_rle(self, frame_hw, scale, serial=None, want_counts=False):
    """odt_mask_rle: the masks of forward ``serial`` (default: the most recent one) as COCO RLE of a frame_hw frame with the
    boxes divided by ``scale`` -- [{"size": [H0, W0], "counts": str}] per valid detection (reference
    obj_detect_tracking.py:715-739).  Raises once another forward has been enqueued since ``serial``."""
    res = _lib.OdtRleResult()
    s = self.forward_serial() if serial is None else int(serial)
    self.lib.check(self.lib.dll.odt_mask_rle(self._handle.live(), s, int(frame_hw[0]), int(frame_hw[1]), float(scale),
                                             int(bool(want_counts)), C.byref(res)))
    rles = res.rles()
    return (rles, res.count_lists()) if want_counts else rles

  def read_outputs(self, want_feats=True, want_pooled=False):
    """The outputs of the most recently enqueued forward (odt_read_outputs): what :meth:`forward` would have
    returned for the frames of the last :meth:`forward_device_async`."""
    out = self._outputs(want_feats, want_pooled)
    self.lib.check(self.lib.dll.odt_read_outputs(self._handle.live(), C.byref(out)))
    return self._result(want_feats, want_pooled)

  def submit(self, frames, want_feats=True, want_pooled=True):
    """Pipelined ingest (odt_submit_ex): enqueue H2D + forward + D2H for one batch of host
    frames and return a ticket at once; at most two tickets may be outstanding.  Only what is
    asked for crosses PCIe on the way back (the [M,C,7,7] features are 40 MB per 8-frame batch,
    their 7x7 mean 0.8 MB)."""
    if frames is None:                # the frames were written into ingest_buffer(): no staging copy
      src, dt = None, self._ingest_dtype
      view = self._ingest_view        # (None: nothing armed for this ticket -- odt_submit_ex refuses below)
      # the zero-copy path is guarded like the others: both handles read the armed pinned buffer (a blocking forward
      # does not touch the ingest slots); if the engine moves to the twin's handle, the frames move to ITS buffer
      if view is not None and self._calibrate(lambda e: e._forward_blocking(view.ctypes.data_as(C.c_void_p), dt)):
        self.ingest_buffer(np.uint8 if dt == ODT_DTYPE_U8 else np.float32)[...] = view
      self._ingest_view = None
    else:
      fr, src, dt = self._frames(frames)
      self._calibrate(lambda e: e._forward_blocking(src, dt))
    t = C.c_int()
    want = (1 if want_feats else 0) | (2 if want_pooled else 0) | (4 if self.add_mask else 0)
    self.lib.check(self.lib.dll.odt_submit_ex(self._handle.live(), src, dt, want, C.byref(t)))
    self._ticket_want[t.value] = (bool(want_feats), bool(want_pooled))
    return t.value

  def ingest_buffer(self, dtype=np.uint8):
    """The NEXT ticket's pinned host input buffer as a numpy array [B,Hs,Ws,3] (odt_ingest_buffer): a decoder writes
    its frames straight into it and calls ``submit(None)`` -- the pageable -> pinned staging copy of
    ``submit(frames)`` disappears (what 8 co-hosted ranks contend on first is host memory bandwidth)."""
    dt = ODT_DTYPE_U8 if np.dtype(dtype) == np.uint8 else ODT_DTYPE_F32
    buf = C.c_void_p(); nbytes = C.c_size_t()
    self.lib.check(self.lib.dll.odt_ingest_buffer(self._handle.live(), dt, C.byref(buf), C.byref(nbytes)))
    self._ingest_dtype = dt
    ctype = C.c_uint8 if dt == ODT_DTYPE_U8 else C.c_float
    n = nbytes.value // C.sizeof(ctype)
    arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ctype)), shape=(n,))
    self._ingest_view = arr.reshape(self.batch, self.src_height, self.src_width, 3)
    self._ingest_views_out = True
    return self._ingest_view

  def collect(self, ticket, want_feats=None, want_pooled=None):
    """Wait for a ticket of :meth:`submit`; same return value as :meth:`forward`.  By default what comes back is what
    the ticket was submitted with (features and / or their 7x7 mean); asking for more than that is an error."""
    sub = self._ticket_want.get(ticket, (True, False))
    want_feats = sub[0] if want_feats is None else want_feats
    want_pooled = sub[1] if want_pooled is None else want_pooled
    out = self._outputs(want_feats, want_pooled)
    self.lib.check(self.lib.dll.odt_collect(self._handle.live(), ticket, C.byref(out)))
    self._ticket_want.pop(ticket, None)
    self._watch()
    return self._result(want_feats, want_pooled)

  def forward_stream(self, batches, want_feats=False, want_pooled=True):
    """Generator over an iterable of frame batches with two batches in flight: the H2D of
    batch i+1 and the D2H of batch i-1 overlap the forward of batch i.  By default the appearance
    features come back pooled ([M,C]: what create_obj_infos makes of fpn_box_feat anyway,
    reference deep_sort/utils.py:27-28); want_feats=True returns the [M,C,7,7] tensor."""
    pending = []
    for fr in batches:
      pending.append(self.submit(fr, want_feats, want_pooled))
      if len(pending) == 2:
        yield self.collect(pending.pop(0), want_feats, want_pooled)
    while pending:
      yield self.collect(pending.pop(0), want_feats, want_pooled)

  def forward_device_async(self, dev_ptr, dtype, stream=None):
    """Enqueue one forward on frames already resident in HBM (bench path)."""
    def run(e):
      e.lib.check(e.lib.dll.odt_forward_async(e._handle.live(), C.c_void_p(dev_ptr), dtype, 1, None))
      e._handle.synchronize()
    self._calibrate(run)
    self.lib.check(self.lib.dll.odt_forward_async(self._handle.live(), C.c_void_p(dev_ptr), dtype, 1,
                                                  C.c_void_p(stream) if stream else None))

  def synchronize(self):
    self._handle.synchronize()
    self._watch()

  def describe(self):
    """What the handle runs (odt_describe), and what its range guard has done."""
    d = self._handle.describe()
    if self._guard is not None:
      d["conv_split_family_auto"], d["range_guard"] = self._guard.report()
    else:
      d["range_guard"] = "off (explicit conv_split_family = %r / conv_arith)" % (self._family_requested,)
    return d

  def range_report(self, names=None):
    """Debug handles (keep_taps): per stage tensor the |max| of the last forward and the share of its non-zero elements
    more than 2^17 below it -- what the fp16x2 kernels' per-tensor power of two leaves in the f16 subnormal grid (absolute
    instead of relative precision there).  {name: {"amax", "frac_nonzero_below_2^-17_amax", "elements"}}."""
    out = {}
    for name in (names or ("conv0", "pool0", "c2", "c3", "c4", "c5", "p2", "p3", "p4", "p5", "p6")):
      t = np.abs(self.tap(name))
      amax = float(t.max())
      nz = t > 0
      out[name] = {"amax": amax, "elements": int(t.size),
                   "frac_nonzero_below_2^-17_amax": float(((t < amax * 2.0 ** -17) & nz).sum() / max(1, int(nz.sum())))}
    return out


def _missing_se_variables(weights, num_blocks):
  """Names of the squeeze-excitation variables (groupG/blockI/fc1/{W,b}, fc2/{W,b}; W as [in, out]) that ``weights`` lacks
  or holds in another shape."""
  bad = []
  for g, (ch, cnt) in enumerate(zip((64, 128, 256, 512), num_blocks)):
    for i in range(int(cnt)):
      pre = "group%d/block%d/" % (g, i)
      for name, shape in (("fc1/W", (4 * ch, ch // 4)), ("fc1/b", (ch // 4,)), ("fc2/W", (ch // 4, 4 * ch)), ("fc2/b", (4 * ch,))):
        if pre + name not in weights or tuple(np.shape(weights[pre + name])) != shape:
          bad.append(pre + name)
  return bad


class _DetectorBase(object):
  graph = ODT_GRAPH_SINGLE

  def __init__(self, config, gpuid=0, weights=None, lib=None):
    self.config = finalize_config(config)
    self.gpuid = gpuid
    self.lib = lib if lib is not None else _lib.get_lib()
    if weights is None:
      path = getattr(config, "load_from", None) if getattr(config, "is_load_from_pb", False) \
          else getattr(config, "model_path", None)
      path = path or getattr(config, "model_path", None)
      if path and str(path).endswith(".pb"):
        # frozen graph (reference --is_load_from_pb, models.py:198-263): Const payloads by name
        weights = load_frozen_pb(path)
      elif path and str(path).endswith(".npz"):
        weights = load_npz(path)
      elif path and (os.path.isdir(str(path)) or os.path.exists(str(path) + ".index") or
                     str(path).endswith(".index")):
        # TF checkpoint directory / prefix (reference obj_detect_tracking.py:404-416), read
        # without TensorFlow
        weights = load_checkpoint(str(path))
      else:
        raise ValueError("weights: pass a {name: array} dict or set config.model_path to a "
                         "Tensorpack-style .npz (reference obj_detect_tracking.py:417-435), a "
                         "TF checkpoint directory / prefix, or a frozen .pb (--is_load_from_pb)")
    unsupported = [f for f in ("use_small_object_head", "use_cascade_rcnn")
                   if getattr(self.config, f, False)]
    if unsupported:
      raise NotImplementedError("graph variants not built on this path (SURVEY.md 8, out of scope): "
                                + ", ".join(unsupported))
    if getattr(self.config, "use_gn", False):
      # --use_gn (nn.py:81-108): GroupNorm in the plain bottleneck backbone and the FPN (and, with use_conv_frcnn_head, the box head)
      for f in ("use_se", "use_resnext", "use_basic_block", "use_deformable"):
        if getattr(self.config, f, False):
          raise NotImplementedError("graph variants not built on this path: use_gn together with %s" % f)
      missing = [n for n in group_norm_variables(self.config) if n not in weights]
      if missing:
        raise NotImplementedError("a GroupNorm graph cannot be built from weights without gn/{gamma,beta} variables: missing "
                                  + ", ".join(missing[:4]) + (" ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
    if getattr(self.config, "add_relation_nn", False):
      # --add_relation_nn (nn.py:115-190 from models.py:1044-1054): RM_r1 behind fc6 and RM_r2 behind fc7 of the 2-FC box head;
      # independent of the backbone, the output layers and the mask head
      if getattr(self.config, "use_conv_frcnn_head", False):
        raise NotImplementedError("graph variants not built on this path: add_relation_nn together with use_conv_frcnn_head (the "
                                  "reference takes the flag for that head, ignores it and says nothing)")
      if self.graph != ODT_GRAPH_SINGLE:
        raise NotImplementedError("add_relation_nn is built for the single-image graph (Mask_RCNN_FPN): the reference's batched "
                                  "graph calls the box head without boxes and cannot build it")
      topk = int(self.config.rpn_test_post_nms_topk)
      if topk > 1024:
        raise NotImplementedError("graph variants not built on this path: add_relation_nn with rpn_test_post_nms_topk = %d (at most "
                                  "1024: the attention kernel keeps one score row per query in LDS)" % topk)
      dim = int(self.config.fpn_frcnn_fc_head_dim)
      if dim < 64 or dim > 1024 or dim % 64 != 0:
        raise NotImplementedError("graph variants not built on this path: add_relation_nn with fpn_frcnn_fc_head_dim = %d (a "
                                  "multiple of 64 in [64, 1024]: 16 heads of whole MFMA k-steps, 64-column output chunks)" % dim)
      missing = [n for n in relation_variables(self.config) if n not in weights]
      if missing:
        raise NotImplementedError("a relation-network box head (add_relation_nn) cannot be built from weights without its variables: "
                                  "missing " + ", ".join(missing[:4]) + (" ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
    if getattr(self.config, "use_conv_frcnn_head", False):
      # --use_conv_frcnn_head (models.py:1110-1124): fastrcnn/conv0..3 (+ fastrcnn/gn0..3 under use_gn) and fastrcnn/fc in place
      # of fc6 / fc7; independent of the backbone, the output layers and the mask head
      dc = int(getattr(self.config, "conv_frcnn_head_dim", 256))
      if dc < 32 or dc > 512 or dc % 32 != 0:
        raise NotImplementedError("graph variants not built on this path: use_conv_frcnn_head with conv_frcnn_head_dim = %d (a "
                                  "multiple of 32 in [32, 512]: the conv kernels' channel step and GroupNorm's 32 groups)" % dc)
      missing = [n for n in conv_head_variables(self.config) if n not in weights]
      if missing:
        raise NotImplementedError("a 4-conv box head (use_conv_frcnn_head) cannot be built from weights without its variables: "
                                  "missing " + ", ".join(missing[:4]) + (" ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
    if getattr(self.config, "use_att_frcnn_head", False):
      # --use_att_frcnn_head (models.py:1064-1089, :2682-2707): hidden + relu(att_trans(sum of the RoI's 49 positions)) behind
      # whichever box head is configured; independent of the backbone, the graph and the mask head.  Checked here, not at the
      # first frame: a model that cannot run should not construct
      if getattr(self.config, "use_frcnn_class_agnostic", False):
        raise NotImplementedError("graph variants not built on this path: use_att_frcnn_head together with use_frcnn_class_agnostic "
                                  "(set by hand or by version 4 .. 6): the reference's class-agnostic head has no attention branch -- "
                                  "it takes the flag, ignores it and says nothing")
      missing = [n for n in att_head_variables(self.config) if n not in weights]
      if missing:
        raise NotImplementedError("an attention box head (use_att_frcnn_head) cannot be built from weights without its variables: "
                                  "missing " + ", ".join(missing))
      ch, dim = int(self.config.fpn_num_channel), int(self.config.fpn_frcnn_fc_head_dim)
      for n, shape in zip(att_head_variables(self.config), ((3, 3, ch, 1), (1,), (ch, dim), (dim,))):
        got = tuple(np.asarray(weights[n]).shape)
        if int(np.prod(got)) != int(np.prod(shape)):
          raise ValueError("use_att_frcnn_head: bad shape for %s: %s, the graph has %s" % (n, list(got), list(shape)))
      for n in ("fastrcnn/attention/W", "fastrcnn/attention/b"):
        # the map is softmax over ONE channel: exp(l - l) / exp(l - l) = 1 for a finite logit, NaN otherwise
        if not np.isfinite(np.asarray(weights[n], np.float32)).all():
          raise ValueError("use_att_frcnn_head: %s holds a non-finite value: the reference's softmax over the attention map's one "
                           "channel returns NaN there, not the 1.0 this path rests on" % n)
    for f in ("use_resnext", "use_basic_block"):
      # the reference's basic and ResNeXt blocks take use_se and ignore it (nn.py:439-456, 524-549): a graph that silently
      # differs from what a --version 6 checkpoint was trained as is worse than an error
      if getattr(self.config, f, False) and getattr(self.config, "use_se", False):
        raise NotImplementedError("graph variants not built on this path: %s together with use_se (the reference builds "
                                  "these blocks without squeeze-excitation and says nothing)" % f)
    if getattr(self.config, "use_deformable", False):
      # --use_deformable (nn.py:469-485, 574-585): a deformable conv2 in the stride-2 bottleneck that opens a stage
      for f in ("use_resnext", "use_basic_block"):
        if getattr(self.config, f, False):
          raise NotImplementedError("graph variants not built on this path: use_deformable together with %s (the reference "
                                    "takes the flag for these blocks, ignores it and says nothing)" % f)
      if getattr(self.config, "use_se", False):
        raise NotImplementedError("graph variants not built on this path: use_deformable together with use_se")
      groups = deformable_groups(self.config)
      if 3 in groups and getattr(self.config, "use_dilations", False):
        raise ValueError("use_deformable with use_dilations: the reference pads the deformable, dilated group3/block0 once more "
                         "(nn.py:493-497) and its graph does not build (ceil(h / 2) + 1 rows against the shortcut's h / 2); "
                         "pass use_dilations=False (or version=2) with use_deformable=True")
      missing = [n for g in groups for n in ("group%d/block0/conv2_offset/W" % g, "group%d/block0/conv2_offset/b" % g)
                 if n not in weights]
      if missing:
        raise NotImplementedError("a deformable graph cannot be built from weights without conv2_offset variables: missing "
                                  + ", ".join(missing[:4]) + (" ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
    if getattr(self.config, "use_se", False):
      # version 6 (nn.py:506-517): every bottleneck carries fc1 / fc2.  Checked here, not at the first frame: a plan cannot be
      # built without them, and a model that cannot run should not construct
      missing = _missing_se_variables(weights, self.config.resnet_num_block)
      if missing:
        raise NotImplementedError("an SE graph cannot be built from weights without squeeze-excitation variables: missing "
                                  + ", ".join(missing[:4]) + (" ... (%d in all)" % len(missing) if len(missing) > 4 else ""))
    # --use_partial_classes (reference models.py:807-829): class-subset head
    self.head_num_class = int(self.config.num_class)
    if getattr(self.config, "use_frcnn_class_agnostic", False):
      weights = expand_class_agnostic_box(weights, self.head_num_class)
    if getattr(self.config, "use_partial_classes", False):
      ids = [self.config.classname2id[name] for name in self.config.partial_classes]
      weights = select_partial_classes(weights, ids, self.head_num_class)
      self.head_num_class = len(ids) + 1
    self.weights = weights
    self._engines = {}
    # the reference's tensor handles / placeholders (models.py:282-283, 965-973)
    self.image = TensorHandle(self, "image")
    self.is_train = TensorHandle(self, "is_train")
    self.final_boxes = TensorHandle(self, "final_boxes")
    self.final_labels = TensorHandle(self, "final_labels")
    self.final_probs = TensorHandle(self, "final_probs")
    self.fpn_box_feat = TensorHandle(self, "fpn_box_feat")
    self.final_valid_indices = TensorHandle(self, "final_valid_indices")
    if getattr(self.config, "add_mask", False):       # reference models.py:959-962
      if self.graph != ODT_GRAPH_SINGLE:
        raise NotImplementedError("--add_mask is built for the single-image graph (Mask_RCNN_FPN)")
      self.final_masks = TensorHandle(self, "final_masks")

  # static plans kept per model: a plan owns its activations, a device copy of the weights and pinned staging
  # (tens of GB at 8 x 1080p), so frames of ever-changing sizes (the reference's image-list drivers) must not
  # accumulate them: least-recently-used plans beyond this many are closed
  max_engines = 8

  def engine(self, batch, height, width, src_hw=None, replica=0, stream_set=False):
    """The static plan for frames of this size.  ``replica`` > 0: a further handle of the same plan (own weights copy, arena and
    streams) -- ``predict_stream`` keeps consecutive frames in flight on them."""
    key = (batch, height, width) if src_hw is None else (batch, height, width) + tuple(src_hw)
    if replica:
      key = key + ("replica", int(replica))
    cfg_e = self.config
    if stream_set:
      # handles of predict_stream: side by side, no side streams of their own (include/odt.h: tail_overlap)
      key = key + ("stream",)
      cfg_e = copy.copy(self.config); cfg_e.tail_overlap = False
    e = self._engines.pop(key, None)
    if e is None:
      # evict least-recently-used plans beyond the cap -- but never one with tickets in flight (its pinned results
      # would be destroyed under the caller): those stay until collected, even if that exceeds the cap.  An engine
      # object a caller kept from an earlier engine() call is closed by its eviction; its next use raises OdtError
      # ("engine closed") -- hold at most `max_engines` plan sizes at a time, or raise the cap.
      while len(self._engines) >= max(1, int(self.max_engines)):
        old = next((k for k, v in self._engines.items() if not v._ticket_want), None)
        if old is None:
          break
        self._engines.pop(old).close()
      e = _Engine(self.lib, cfg_e, self.graph, batch, height, width,
                  self.weights, self.gpuid, num_class=self.head_num_class)
      if src_hw is not None:
        e.set_source_size(*src_hw)
    self._engines[key] = e           # (re)insert: dict order = recency
    return e

  def engine_for_raw(self, batch, src_height, src_width):
    """Engine for frames as they come off the decoder: (engine, scale) with the plan sized by
    the reference's rule (get_new_hw, nn.py:1548-1560, short_edge_size / max_size of the config)
    and the resize done on the device; ``scale`` is what the drivers divide boxes by
    (obj_detect_tracking.py:607-608)."""
    neww, newh = get_new_hw(src_height, src_width, self.config.short_edge_size, self.config.max_size)
    scale = (newh * 1.0 / src_height + neww * 1.0 / src_width) / 2.0
    if (newh, neww) == (src_height, src_width):
      return self.engine(batch, newh, neww), scale
    return self.engine(batch, newh, neww, src_hw=(src_height, src_width)), scale

  # reference models.py:1629-1636
  def get_feed_dict_forward(self, imgdata):
    return {self.image: imgdata, self.is_train: False}

  def _fetch(self, fetches, feed_dict):
    raise NotImplementedError

  def close(self):
    for e in self._engines.values():
      e.close()
    self._engines = {}


def _first_image(result, pooled):
  """A b = 1 engine result as the single-image graph returns it: the valid rows, labels as int64."""
  boxes, labels, probs, valid, feats, pl = result
  r = int(valid[0])
  return boxes[0, :r].copy(), labels[0, :r].astype(np.int64), probs[0, :r].copy(), pl if pooled else feats


class Mask_RCNN_FPN(_DetectorBase):
  """b=1 graph (reference models.py:267-973)."""
  graph = ODT_GRAPH_SINGLE

  def predict(self, img, pooled=False):
    """One frame [H,W,3] BGR -> (final_boxes [R,4] f32, final_labels [R] i64,
    final_probs [R] f32, fpn_box_feat [R,256,7,7] f32 (or [R,256] if pooled))."""
    img = np.asarray(img)
    e = self.engine(1, img.shape[0], img.shape[1])
    ret = _first_image(e.forward(img[None], want_feats=not pooled, want_pooled=pooled), pooled)
    self.last_masks = e._masks[:len(ret[0])].copy() if e.add_mask else None    # final_masks [R,28,28]
    self._last_forward = (e, e.forward_serial())
    return ret

  def masks_rle(self, frame_hw, scale, want_counts=False):
    """The masks of the last ``predict`` / ``predict_raw`` as the reference's JSON holds them: per detection
    ``{"size": [H0, W0], "counts": str}`` of ``fill_full_mask(final_boxes[j] / scale, final_masks[j], frame_hw)`` encoded
    with pycocotools (obj_detect_tracking.py:715-739), computed on the device from that forward's outputs.  A rectangle
    that reaches past the frame is clipped to it (the reference raises).  Raises if the engine has run another forward
    since, and for a model without add_mask."""
    last = getattr(self, "_last_forward", None)
    if last is None:
      raise _lib.OdtError("masks_rle: no forward yet (predict / predict_raw)")
    e, serial = last
    return e.mask_rle(frame_hw, scale, serial=serial, want_counts=want_counts)

  def predict_stream(self, frames, in_flight=2, pooled=False):
    """Frame-by-frame detection of a video with ``in_flight`` consecutive frames on the GPU at once (round 6): frame t runs on
    handle t mod in_flight, each handle on its own streams, results come back in frame order.  A single 1080p frame leaves most of
    the chip idle most of the time (each of its ~130 launches is latency-bound): 181 -> 220 frames/s with two frames in flight on
    `Mask_RCNN_FPN`.  Two is the robust default; from three on the handles are built without side streams of their own
    (odt_config.tail_overlap = -1) -- 223 / 236 frames/s with three / four in a process that holds no other handles, but 192 / 210
    next to an idle one (streams share hardware queues in creation order: profiles/r06_b1_stream_set.txt); the reference's loop (obj_detect_tracking.py:597-635) sees the same
    per-frame results, one frame later.  Yields what ``predict`` returns."""
    n = max(1, int(in_flight))
    pending = collections.deque()

    def finish(e, ticket):
      return _first_image(e.collect(ticket), pooled)

    for k, img in enumerate(frames):
      img = np.asarray(img)
      if len(pending) == n:
        yield finish(*pending.popleft())
      e = self.engine(1, img.shape[0], img.shape[1], replica=k % n, stream_set=n > 2)
      pending.append((e, e.submit(img[None], want_feats=not pooled, want_pooled=pooled)))
    while pending:
      yield finish(*pending.popleft())

  def predict_raw(self, frame, pooled=False, mask_rle=False):
    """Decoder-sized frame [H0,W0,3] (uint8 or float32 BGR): the reference's
    ``resizeImage(frame.astype("float32"), short_edge_size, max_size)`` step
    (obj_detect_tracking.py:597-608) runs on the device.  Returns (boxes, labels, probs, feats,
    scale) with boxes in resized-image coordinates, exactly what ``sess.run`` returns after the
    host-side resize.  mask_rle=True (add_mask models): one more element, ``masks_rle((H0, W0), scale)``."""
    frame = np.asarray(frame)
    e, scale = self.engine_for_raw(1, frame.shape[0], frame.shape[1])
    ret = _first_image(e.forward(frame[None], want_feats=not pooled, want_pooled=pooled), pooled) + (scale,)
    self._last_forward = (e, e.forward_serial())
    if mask_rle:
      ret = ret + (self.masks_rle(frame.shape[:2], scale),)
    return ret

  def _fetch(self, fetches, feed_dict):
    boxes, labels, probs, feats = self.predict(feed_dict[self.image])
    table = {"final_boxes": boxes, "final_labels": labels, "final_probs": probs,
             "fpn_box_feat": feats,
             "final_valid_indices": np.asarray([boxes.shape[0]], np.int32),
             "final_masks": self.last_masks}
    return [table[f.name] for f in fetches]


class Mask_RCNN_FPN_multi(_DetectorBase):
  """b=B graph (reference models.py:1969-2408)."""
  graph = ODT_GRAPH_MULTI

  # reference models.py:3301
  def get_feed_dict_forward_multi(self, imgdata_list):
    return {self.image: np.stack(imgdata_list, axis=0), self.is_train: False}

  def predict_batch(self, imgs, pooled=False):
    """[B,H,W,3] -> (final_boxes [B,100,4], final_labels [B,100] f32, final_probs [B,100],
    final_valid_indices [B] i32, fpn_box_feat [M,256,7,7]), M = sum(valid)."""
    imgs = np.asarray(imgs)
    e = self.engine(imgs.shape[0], imgs.shape[1], imgs.shape[2])
    boxes, labels, probs, valid, feats, pl = e.forward(imgs, want_feats=not pooled,
                                                       want_pooled=pooled)
    return boxes, labels.astype(np.float32), probs, valid, (pl if pooled else feats)

  def predict_batch_raw(self, frames, pooled=False):
    """[B,H0,W0,3] decoder-sized frames; device-side resize (see Mask_RCNN_FPN.predict_raw).
    Returns predict_batch's tuple + scale."""
    frames = np.asarray(frames)
    e, scale = self.engine_for_raw(frames.shape[0], frames.shape[1], frames.shape[2])
    boxes, labels, probs, valid, feats, pl = e.forward(frames, want_feats=not pooled,
                                                       want_pooled=pooled)
    return boxes, labels.astype(np.float32), probs, valid, (pl if pooled else feats), scale

  def _fetch(self, fetches, feed_dict):
    boxes, labels, probs, valid, feats = self.predict_batch(feed_dict[self.image])
    table = {"final_boxes": boxes, "final_labels": labels, "final_probs": probs,
             "final_valid_indices": valid, "fpn_box_feat": feats}
    return [table[f.name] for f in fetches]


class Session(object):
  """Shim for the ``tf.Session`` the reference drivers use: ``run(fetches,
  feed_dict)`` triggers ONE forward and returns numpy arrays in fetch order
  (reference obj_detect_tracking.py:632-635)."""

  def __init__(self, config=None):
    pass

  def __enter__(self):
    return self

  def __exit__(self, *a):
    return False

  def run(self, fetches, feed_dict=None):
    """Fetches / feed keys are tensor handles or TF tensor names ("model_0/final_boxes:0", or "final_boxes:0"
    when one frozen model is imported): the reference's frozen route addresses everything by name."""
    single = isinstance(fetches, (TensorHandle, str))
    fl = [fetches] if single else list(fetches)
    fl = [_DEFAULT_GRAPH.get_tensor_by_name(f) if isinstance(f, str) else f for f in fl]
    feed = {(_DEFAULT_GRAPH.get_tensor_by_name(k) if isinstance(k, str) else k): v
            for k, v in (feed_dict or {}).items()}
    model = fl[0].model
    out = model._fetch(fl, feed)
    return out[0] if single else out


def config_from_weights(weights, add_mask=False, is_multi=False, **overrides):
  """Architecture of a frozen model from its tensors (the reference's Mask_RCNN_FPN_frozen needs no config: the
  graph is in the file; here the file is a weight container, so what the graph would say is read off the shapes):
  bottlenecks per stage, classes, FPN / head widths, class-agnostic box head.  Everything that is a graph constant
  rather than a tensor (rpn_test_post_nms_topk, thresholds, frame size) keeps the reference's defaults unless
  overridden.  ``group0/block0/fc1/W`` present means a squeeze-excitation backbone (use_se); unless overridden,
  use_dilations=False follows from it: the only published SE model (version 6) is undilated.  A
  ``groupG/block0/conv2_offset/W`` means deformable stage entries (use_deformable, and no dilations); ``conv0/gn/gamma`` means
  GroupNorm in the backbone and the FPN (use_gn); ``fastrcnn/conv0/W`` means the 4-conv + FC box head (use_conv_frcnn_head, its
  last axis conv_frcnn_head_dim); ``fastrcnn/RM_r1/query_linear/W`` means relation modules in the 2-FC head (add_relation_nn);
  ``fastrcnn/att_trans/W`` behind per-class box outputs means the attention branch (use_att_frcnn_head).  No ``group0/block0/conv3/W``
  means basic blocks (use_basic_block); a ``conv2/W`` of [3,3,C/32,C] means ResNeXt-32x4d (use_resnext)."""
  from .config import make_config
  blocks = [0, 0, 0, 0]
  for k in weights:
    parts = k.split("/")
    if len(parts) >= 3 and parts[0].startswith("group") and parts[1].startswith("block") and parts[2] == "conv1":
      g, b = int(parts[0][5:]), int(parts[1][5:])
      blocks[g] = max(blocks[g], b + 1)
  num_class = int(np.asarray(weights["fastrcnn/outputs/class/W"]).shape[-1])
  nbox = int(np.asarray(weights["fastrcnn/outputs/box/W"]).shape[-1])
  kw = dict(resnet_num_block=blocks, num_class=num_class, add_mask=bool(add_mask),
            use_frcnn_class_agnostic=(nbox == 4 or nbox == 8) and num_class > 2,
            im_batch_size=2 if is_multi else 1)
  if "group0/block0/fc1/W" in weights:
    kw.update(use_se=True, use_dilations=False)
  if any(k.endswith("/block0/conv2_offset/W") for k in weights):
    kw.update(use_deformable=True, use_dilations=False)      # (the reference graph does not build with both)
  if "conv0/gn/gamma" in weights:
    kw.update(use_gn=True)                     # GroupNorm variables in place of conv0/bn
  if "fastrcnn/conv0/W" in weights:            # the 4-conv + FC box head; its width is the conv's Cout
    kw.update(use_conv_frcnn_head=True, conv_frcnn_head_dim=int(np.asarray(weights["fastrcnn/conv0/W"]).shape[-1]))
  if "fastrcnn/RM_r1/query_linear/W" in weights:      # relation modules behind fc6 / fc7
    kw.update(add_relation_nn=True)
  if "fastrcnn/att_trans/W" in weights and not kw["use_frcnn_class_agnostic"]:
    kw.update(use_att_frcnn_head=True)         # the attention branch (the class-agnostic head has none and never creates the variable)
  if "group0/block0/conv3/W" not in weights:
    kw.update(use_basic_block=True)            # resnet_basicblock: two 3x3 convs, no conv3
  else:
    w2 = np.asarray(weights["group0/block0/conv2/W"]).shape
    if w2[2] * 32 == w2[3]:
      kw.update(use_resnext=True)              # conv2/W [3,3,C/32,C]: the 32-group conv of resnext_32x4d_bottleneck
  kw.update(overrides)
  cfg = make_config(**kw)
  cfg.fpn_num_channel = int(np.asarray(weights["fpn/lateral_1x1_c2/W"]).shape[-1])
  cfg.fpn_frcnn_fc_head_dim = int(np.asarray(weights["fastrcnn/fc/W" if cfg.use_conv_frcnn_head else "fastrcnn/fc6/W"]).shape[-1])
  return cfg


class Mask_RCNN_FPN_frozen(object):
  """``Mask_RCNN_FPN_frozen(modelpath, gpuid, add_mask, is_multi)`` (reference models.py:198-263): a frozen ``.pb``
  imported under the name scope ``model_<gpuid>`` whose placeholders and outputs are looked up BY NAME --
  ``model_0/image:0`` in, ``model_0/final_boxes:0``, ``final_labels:0``, ``final_probs:0``, ``fpn_box_feat:0``
  (``final_valid_indices:0`` with is_multi, ``final_masks:0`` with add_mask) out -- and run with
  ``sess.run([...], feed_dict=model.get_feed_dict_forward(img))``.  Same attributes, same feed-dict methods; the
  tensors are also reachable through ``get_default_graph().get_tensor_by_name`` and as plain strings in
  ``Session.run``.  The file is read without TensorFlow (frozen_pb.py); pass the driver's ``config`` for what is
  a graph constant in the file (rpn_test_post_nms_topk ...), else config_from_weights() fills in the reference's
  defaults."""

  def __init__(self, modelpath, gpuid, add_mask=False, is_multi=False, config=None, lib=None):
    self.graph = get_default_graph()
    self.is_multi = is_multi
    self.var_prefix = "model_%s" % gpuid
    weights = load_frozen_pb(modelpath)
    if config is None:
      config = config_from_weights(weights, add_mask=add_mask, is_multi=is_multi)
    cls = Mask_RCNN_FPN_multi if is_multi else Mask_RCNN_FPN
    self._model = cls(config, gpuid=gpuid, weights=weights, lib=lib)
    self.config = self._model.config
    names = ["image", "final_boxes", "final_labels", "final_probs", "fpn_box_feat"]
    if is_multi:
      names.append("final_valid_indices")
    if add_mask:
      names.append("final_masks")
    self.graph._unregister(self.var_prefix)             # re-import under the same scope replaces it
    for n in names:
      h = getattr(self._model, n)
      self.graph._register(self.var_prefix, h)
      setattr(self, n, self.graph.get_tensor_by_name("%s/%s:0" % (self.var_prefix, n)))

  def get_feed_dict_forward(self, imgdata):              # reference models.py:241-255
    if self.is_multi:
      return {self.image: np.stack(imgdata, axis=0)}
    return {self.image: imgdata}

  def get_feed_dict_forward_multi(self, imgs):           # reference models.py:257-264
    return {self.image: np.stack(imgs, axis=0)}

  def predict(self, *a, **k):
    return self._model.predict(*a, **k)

  def predict_batch(self, *a, **k):
    return self._model.predict_batch(*a, **k)

  def engine(self, *a, **k):
    return self._model.engine(*a, **k)

  def close(self):
    self.graph._unregister(self.var_prefix)
    self._model.close()


def get_model(config, gpuid=0, task=0, controller="/cpu:0", is_multi=False, weights=None,
              lib=None):
  """reference models.py:97-119.  Dispatch is the reference's; frozen ``.pb`` files are read
  without TensorFlow; the EfficientDet branch is a "next" row."""
  # is_load_from_pb (reference models.py:102-108 -> Mask_RCNN_FPN_frozen): the frozen file is read
  # as a weight container (frozen_pb.load_frozen_pb), the architecture comes from the config
  if getattr(config, "is_efficientdet", False):        # reference models.py:103-104,112-113
    from .efficientdet import EfficientDet
    return EfficientDet(config, gpuid=gpuid, weights=weights, lib=lib)
  if weights is None and getattr(config, "is_load_from_pb", False):   # reference models.py:102-108
    path = getattr(config, "load_from", None) or getattr(config, "model_path", None)
    return Mask_RCNN_FPN_frozen(path, gpuid, add_mask=getattr(config, "add_mask", False), is_multi=is_multi,
                                config=config, lib=lib)
  cls = Mask_RCNN_FPN_multi if is_multi else Mask_RCNN_FPN
  return cls(config, gpuid=gpuid, weights=weights, lib=lib)


def initialize(config, sess):
  """reference obj_detect_tracking.py:392-448: weights are loaded when the model is
  built, so this is a no-op kept for drop-in compatibility."""
  return None
