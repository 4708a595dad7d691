"""ctypes binding of the C ABI declared in include/odt.h.

The product path is libodt_hip.so (hand-written HIP for gfx950) and nothing
else: :func:`get_lib` raises if the library is missing or no GPU is visible --
there is no CPU fallback.  (Tests may bind another build of the *same* sources,
e.g. the HIP-on-CPU simulator under tests/emu/, by constructing
:class:`OdtLib` with an explicit path; the package itself never does.)
"""
from __future__ import annotations

import copy
import ctypes as C
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_HIP_PATH = os.path.join(HERE, "libodt_hip.so")

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int32)
c_i64_p = C.POINTER(C.c_int64)
c_double_p = C.POINTER(C.c_double)

ODT_DTYPE_U8, ODT_DTYPE_F32 = 0, 1
ODT_ARITH_DEFAULT, ODT_ARITH_F32, ODT_ARITH_BF16X3 = 0, 1, 2
ODT_GRAPH_SINGLE, ODT_GRAPH_MULTI, ODT_GRAPH_EFFNET = 0, 1, 2
RPN_CH = 16


class OdtConfig(C.Structure):
  _fields_ = [
      ("graph", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32),
      ("width", C.c_int32), ("num_class", C.c_int32),
      ("num_blocks", C.c_int32 * 4), ("use_dilations", C.c_int32),
      ("fpn_channels", C.c_int32), ("head_dim", C.c_int32),
      ("rpn_topk", C.c_int32), ("result_per_im", C.c_int32),
      ("anchor_field", C.c_int32), ("rpn_nms_thresh", C.c_float),
      ("rpn_decode_clip", C.c_float), ("head_decode_clip", C.c_float),
      ("bbox_reg_weights", C.c_float * 4), ("result_score_thresh", C.c_float),
      ("head_nms_thresh", C.c_float), ("add_mask", C.c_int32), ("mask_dim", C.c_int32),
      ("eff_backbone", C.c_int32), ("eff_det", C.c_int32), ("eff_topk", C.c_int32),
      ("eff_image_scale", C.c_float), ("conv_arith", C.c_int32), ("conv_split_family", C.c_int32),
      ("keep_taps", C.c_int32),
      ("tail_overlap", C.c_int32),
      ("use_se", C.c_int32),
      ("block_kind", C.c_int32),
      ("use_deformable", C.c_int32),
      ("use_gn", C.c_int32),
      ("use_conv_frcnn_head", C.c_int32),      # the 4-conv + FC box head (fastrcnn/conv0..3, fastrcnn/fc)
      ("conv_head_dim", C.c_int32),            # conv_frcnn_head_dim (256)
      ("add_relation_nn", C.c_int32),          # relation modules RM_r1 / RM_r2 in the 2-FC box head
      ("use_att_frcnn_head", C.c_int32),       # hidden + relu(att_trans(sum of the RoI's 49 positions)) in front of the output layers
  ]


class OdtOutputs(C.Structure):
  _fields_ = [("boxes", c_float_p), ("probs", c_float_p), ("labels", c_int_p),
              ("valid", c_int_p), ("feats", c_float_p), ("pooled", c_float_p),
              ("masks", c_float_p)]


class OdtRleResult(C.Structure):
  _fields_ = [("n", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("strings", C.c_void_p),
              ("offsets", c_i64_p), ("lengths", c_int_p), ("counts", C.POINTER(C.c_uint32)), ("count_offsets", c_i64_p)]

  def rles(self):
    """[{"size": [H, W], "counts": str}] -- what the reference puts into its JSON (counts.decode("ascii"))."""
    size = [int(self.height), int(self.width)]
    out = []
    for j in range(int(self.n)):
      s = C.string_at(self.strings + int(self.offsets[j]), int(self.lengths[j])) if self.lengths[j] else b""
      out.append({"size": list(size), "counts": s.decode("ascii")})
    return out

  def count_lists(self):
    """The uncompressed counts per detection (want_counts) as numpy uint32 arrays."""
    if not self.counts:
      return None
    total = int(self.count_offsets[int(self.n)])
    flat = np.ctypeslib.as_array(self.counts, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
    return [flat[int(self.count_offsets[j]):int(self.count_offsets[j + 1])] for j in range(int(self.n))]


def fptr(a):
  return a.ctypes.data_as(c_float_p)


def iptr(a):
  return a.ctypes.data_as(c_int_p)


def f32(a):
  return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
  return np.ascontiguousarray(a, dtype=np.int32)


class OdtError(RuntimeError):
  pass


class OdtLib(object):
  """Typed view of one build of the C ABI."""

  SYMBOLS = [
      "odt_last_error", "odt_device_count", "odt_create", "odt_destroy",
      "odt_load_tensor", "odt_finalize_weights", "odt_forward",
      "odt_forward_async", "odt_synchronize", "odt_read_outputs", "odt_describe", "odt_range_health", "odt_submit", "odt_submit_ex", "odt_collect",
      "odt_ingest_buffer", "odt_set_source_size", "odt_tap", "odt_profile_enable",
      "odt_profile_read", "odt_profile_layer", "odt_probe_mfma_bf16", "odt_nn_cosine", "odt_op_conv2d", "odt_op_conv2d_cat",
      "odt_op_bottleneck_tail", "odt_op_bottleneck_block", "odt_op_stem", "odt_op_conv_choice", "odt_op_last_conv", "odt_op_preprocess",
      "odt_op_maxpool", "odt_op_topk", "odt_op_nms", "odt_op_proposals",
      "odt_op_roi_align", "odt_op_roi_align_plan", "odt_op_mask_select", "odt_op_detections", "odt_op_class_nms",
      "odt_op_dwconv", "odt_op_se_gate", "odt_op_rse_gate", "odt_op_rse_apply", "odt_op_se_tail", "odt_op_group_conv", "odt_op_deform_conv", "odt_op_deform_conv_view", "odt_op_group_norm", "odt_op_group_norm_roi", "odt_op_relation_geo", "odt_op_relation_attention", "odt_op_att_pool", "odt_op_att_add", "odt_op_bifpn_fuse", "odt_op_mbconv_expand_dw", "odt_op_effdet_post",
      "odt_op_preprocess_rgb", "odt_forward_serial", "odt_mask_rle", "odt_op_mask_rle", "odt_tracker_create", "odt_tracker_destroy",
      "odt_tracker_predict", "odt_tracker_update", "odt_tracker_tracks", "odt_lsap", "odt_tracker_nms",
      "odt_tmot_create", "odt_tmot_destroy", "odt_tmot_reset", "odt_tmot_update", "odt_tmot_tracks",
  ]

  def __init__(self, path):
    if not os.path.exists(path):
      raise OdtError("native library not found: %s (build it with "
                     "`python -m object_detection_tracking_amd.build`)" % path)
    self.path = path
    self.dll = C.CDLL(path)
    d = self.dll
    for s in self.SYMBOLS:
      if not hasattr(d, s):
        raise OdtError("%s does not export %s" % (path, s))
    d.odt_last_error.restype = C.c_char_p
    d.odt_create.argtypes = [C.POINTER(OdtConfig), C.c_int, C.POINTER(C.c_void_p)]
    d.odt_destroy.argtypes = [C.c_void_p]
    d.odt_load_tensor.argtypes = [C.c_void_p, C.c_char_p, c_float_p, c_i64_p, C.c_int]
    d.odt_finalize_weights.argtypes = [C.c_void_p]
    d.odt_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                              C.POINTER(OdtOutputs)]
    d.odt_forward_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d.odt_synchronize.argtypes = [C.c_void_p]
    d.odt_read_outputs.argtypes = [C.c_void_p, C.POINTER(OdtOutputs)]
    d.odt_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    d.odt_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    d.odt_range_health.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    d.odt_submit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    d.odt_collect.argtypes = [C.c_void_p, C.c_int, C.POINTER(OdtOutputs)]
    d.odt_set_source_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
    d.odt_ingest_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_size_t)]
    d.odt_tap.argtypes = [C.c_void_p, C.c_char_p, c_float_p, C.c_size_t, c_i64_p,
                          C.POINTER(C.c_int)]
    d.odt_profile_enable.argtypes = [C.c_void_p, C.c_int]
    d.odt_profile_read.argtypes = [C.c_void_p, c_double_p, c_double_p,
                                   C.POINTER(C.c_int), c_double_p]
    d.odt_profile_layer.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, c_double_p,
                                    c_double_p, c_i64_p, C.POINTER(C.c_int)]
    d.odt_probe_mfma_bf16.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, c_double_p, c_double_p, c_double_p,
                                      C.POINTER(C.c_int)]
    d.odt_nn_cosine.argtypes = [C.c_int, c_float_p, c_int_p, C.c_int, c_float_p, C.c_int,
                                C.c_int, c_double_p]
    d.odt_op_conv2d.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p, c_float_p] + \
        [C.c_int] * 11 + [c_float_p, C.c_int, C.c_int, c_float_p]
    d.odt_op_conv2d_cat.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p] + [C.c_int] * 4 + \
        [c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, c_float_p]
    d.odt_op_bottleneck_tail.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p, c_float_p, C.c_int, c_float_p, c_float_p,
                                         C.c_int, c_float_p, C.c_int, C.c_int, c_float_p]
    d.odt_op_bottleneck_block.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p] * 6 + [C.c_int, c_float_p]
    d.odt_op_stem.argtypes = [C.c_int, c_float_p] + [C.c_int] * 3 + [c_float_p, c_float_p, C.c_int, C.c_int, c_float_p]
    d.odt_op_conv_choice.argtypes = [c_int_p, C.c_int, C.c_int, c_int_p, C.c_char_p, C.c_int]
    d.odt_op_last_conv.argtypes = [c_int_p, C.c_char_p, C.c_int]
    d.odt_op_preprocess.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 8 + [c_float_p]
    d.odt_op_maxpool.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p]
    d.odt_op_topk.argtypes = [C.c_int, c_float_p, C.c_int, C.c_int, c_int_p]
    d.odt_op_nms.argtypes = [C.c_int, c_float_p, c_float_p, C.c_int, C.c_int, C.c_float,
                             c_int_p, C.POINTER(C.c_int)]
    d.odt_op_proposals.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p,
                                   C.POINTER(c_float_p), C.POINTER(c_float_p), C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_float, c_float_p, c_int_p]
    d.odt_op_roi_align.argtypes = [C.c_int, C.c_int, C.c_int, c_int_p, c_int_p,
                                   C.POINTER(c_float_p), c_float_p, c_float_p, c_int_p, C.c_int,
                                   c_float_p, c_float_p]
    d.odt_op_roi_align_plan.argtypes = [C.c_int] * 4 + [c_int_p, C.POINTER(c_float_p), c_float_p, c_float_p, C.c_int, c_int_p,
                                        c_int_p] + [C.c_int] * 4 + [c_float_p] * 3 + [C.POINTER(C.c_uint32)]
    d.odt_op_mask_select.argtypes = [C.c_int, c_float_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, c_float_p]
    d.odt_tracker_create.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p)]
    d.odt_tracker_destroy.argtypes = [C.c_void_p]
    d.odt_tracker_predict.argtypes = [C.c_void_p]
    d.odt_tracker_update.argtypes = [C.c_void_p, c_double_p, c_double_p, c_float_p, C.c_int, C.c_int]
    d.odt_tracker_tracks.argtypes = [C.c_void_p, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p,
                                     c_double_p, c_double_p, C.POINTER(C.c_int)]
    d.odt_lsap.argtypes = [c_double_p, C.c_int, C.c_int, c_int_p, c_int_p, C.POINTER(C.c_int)]
    d.odt_tracker_nms.argtypes = [c_double_p, c_double_p, c_int_p, C.c_int, C.c_double, c_int_p, C.POINTER(C.c_int)]
    d.odt_tmot_create.argtypes = [C.c_double] * 8 + [C.POINTER(C.c_void_p)]
    d.odt_tmot_destroy.argtypes = [C.c_void_p]
    d.odt_tmot_reset.argtypes = [C.c_void_p]
    d.odt_tmot_update.argtypes = [C.c_void_p, c_double_p, c_double_p, c_float_p, C.c_int, C.c_int,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    d.odt_tmot_tracks.argtypes = [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_double_p,
                                  c_double_p, c_double_p, c_double_p, c_int_p, c_int_p, c_int_p,
                                  C.POINTER(C.c_int)]
    d.odt_op_detections.argtypes = [C.c_int] * 5 + [c_float_p, c_float_p, c_float_p, c_int_p,
                                                    C.c_int, C.c_int, c_float_p, C.c_float,
                                                    C.c_float, C.c_float, C.c_int, c_float_p,
                                                    c_float_p, c_int_p, c_int_p]
    d.odt_op_class_nms.argtypes = [C.c_int] * 5 + [c_float_p, c_float_p, c_int_p, C.c_float, C.c_float, C.c_int,
                                                   c_float_p, c_float_p, c_int_p, c_int_p]

    d.odt_op_dwconv.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p, c_float_p] + [C.c_int] * 8 + \
        [c_int_p, C.c_int, C.c_int] + [c_float_p] * 7 + [c_int_p]
    d.odt_op_se_gate.argtypes = [C.c_int, c_float_p] + [C.c_int] * 5 + [c_float_p] * 7 + [c_int_p]
    d.odt_op_rse_gate.argtypes = [C.c_int, c_float_p] + [C.c_int] * 5 + [c_float_p] * 6
    d.odt_op_rse_apply.argtypes = [C.c_int, c_float_p, c_float_p, c_float_p] + [C.c_int] * 5 + [c_float_p, c_float_p]
    d.odt_op_se_tail.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p] * 10
    d.odt_op_group_conv.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p, c_float_p] + [C.c_int] * 7 + [c_float_p, c_float_p]
    d.odt_op_deform_conv.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p] * 6
    d.odt_op_deform_conv_view.argtypes = [C.c_int, c_float_p] + [C.c_int] * 7 + [c_float_p] * 6
    d.odt_op_group_norm.argtypes = ([C.c_int, c_float_p] + [C.c_int] * 9 + [c_float_p, c_float_p, C.c_float, C.c_int, C.c_int, c_float_p] +
                                    [C.c_int] * 3 + [c_float_p] * 4)
    d.odt_op_group_norm_roi.argtypes = [C.c_int, c_float_p] + [C.c_int] * 5 + [c_float_p, c_float_p, C.c_float] + [c_float_p] * 4
    d.odt_op_relation_geo.argtypes = [C.c_int, c_float_p, C.c_int, C.c_int, c_float_p, c_float_p]
    d.odt_op_relation_attention.argtypes = [C.c_int] + [c_float_p] * 4 + [C.c_int] * 3 + [c_float_p, C.c_size_t, c_float_p]
    d.odt_op_att_pool.argtypes = [C.c_int, c_float_p, C.c_int, C.c_int, c_float_p, c_float_p]
    d.odt_op_att_add.argtypes = [C.c_int, c_float_p, C.c_int, c_float_p, C.c_int, C.c_int, c_float_p, c_float_p]
    d.odt_op_bifpn_fuse.argtypes = [C.c_int, C.c_int, C.POINTER(c_float_p), c_int_p, c_int_p, c_int_p, c_float_p] + \
        [C.c_int] * 5 + [c_float_p]
    d.odt_op_mbconv_expand_dw.argtypes = [C.c_int, c_float_p] + [C.c_int] * 4 + [c_float_p] * 2 + [C.c_int] * 2 + \
        [c_float_p] * 2 + [C.c_int] * 7 + [c_float_p] * 7 + [c_int_p]
    d.odt_op_effdet_post.argtypes = [C.c_int] * 3 + [c_int_p, C.c_int, C.c_int, C.POINTER(c_float_p), C.POINTER(c_float_p),
                                     c_float_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, c_int_p, c_float_p,
                                     c_float_p, c_int_p, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p, c_int_p]
    d.odt_op_preprocess_rgb.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 11 + [c_float_p]
    d.odt_forward_serial.argtypes = [C.c_void_p, c_i64_p]
    d.odt_mask_rle.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(OdtRleResult)]
    d.odt_op_mask_rle.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.POINTER(OdtRleResult)]

  def check(self, rc):
    if rc != 0:
      msg = self.dll.odt_last_error()
      raise OdtError(msg.decode("utf-8", "replace") if msg else "odt error %d" % rc)

  def device_count(self):
    n = C.c_int(0)
    self.check(self.dll.odt_device_count(C.byref(n)))
    return n.value


_LIB = None


def get_lib():
  """The product library (HIP, gfx950).  Fails loudly; never falls back."""
  global _LIB
  if _LIB is None:
    lib = OdtLib(LIB_HIP_PATH)
    if lib.device_count() < 1:
      raise OdtError("libodt_hip.so loaded but no HIP device is visible")
    _LIB = lib
  return _LIB


def as_frames(frames):
  """Host frames as the library reads them -- contiguous, uint8 as it is, anything else as float32 -- and their ODT_DTYPE_*."""
  fr = np.ascontiguousarray(frames)
  if fr.dtype == np.uint8:
    return fr, ODT_DTYPE_U8
  return np.ascontiguousarray(fr, dtype=np.float32), ODT_DTYPE_F32


class _Handle(object):
  """What the Mask R-CNN engine (models.py) and the EfficientNet / EfficientDet engine (efficientdet/backbone.py) share.
  Owns ``h``, one handle of ``lib``: odt_create(config: OdtConfig, device), odt_load_tensor for every (name, array) of
  ``tensors``, odt_finalize_weights.  Every call goes through :meth:`live`: a closed handle raises instead of reaching
  the library as a null pointer."""

  def __init__(self, lib, config, device, tensors):
    self.lib = lib
    self.profiling = False
    self.h = C.c_void_p()
    lib.check(lib.dll.odt_create(C.byref(config), device, C.byref(self.h)))
    try:
      for name, arr in tensors:
        a = f32(arr)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        lib.check(lib.dll.odt_load_tensor(self.h, name.encode(), fptr(a), C.cast(shape, c_i64_p), a.ndim))
      lib.check(lib.dll.odt_finalize_weights(self.h))
    except Exception:
      self.close()
      raise

  def close(self):
    if self.h is not None:
      self.lib.dll.odt_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def live(self):
    """``h``, or OdtError for a closed handle (model.close(), or evicted from the model's plan cache)."""
    if self.h is None:
      raise OdtError("engine closed (model.close(), or evicted from the model's plan cache: _DetectorBase.max_engines)")
    return self.h

  def move(self):
    """A new wrapper that owns this handle; this one is left closed."""
    new = copy.copy(self)
    self.h = None
    return new

  def set_source_size(self, src_height, src_width):
    self.lib.check(self.lib.dll.odt_set_source_size(self.live(), int(src_height), int(src_width)))

  def synchronize(self):
    self.lib.check(self.lib.dll.odt_synchronize(self.live()))

  def describe(self):
    """What the handle runs (odt_describe): conv arithmetic mode, launches per kernel family, policy thresholds, memory."""
    buf = C.create_string_buffer(16384)
    self.lib.check(self.lib.dll.odt_describe(self.live(), buf, 16384))
    return json.loads(buf.value.decode())

  def tap(self, name):
    """Stage tensor in the device layout (NHWC; EfficientNet: channel stride padded to 32), as numpy."""
    h = self.live()
    shape = (C.c_int64 * 4)(); rank = C.c_int()
    self.lib.check(self.lib.dll.odt_tap(h, name.encode(), None, 0, C.cast(shape, c_i64_p), C.byref(rank)))
    out = np.zeros([int(shape[i]) for i in range(rank.value)], np.float32)
    self.lib.check(self.lib.dll.odt_tap(h, name.encode(), fptr(out), out.size, C.cast(shape, c_i64_p), C.byref(rank)))
    return out

  def range_health(self, rebase=False):
    """odt_range_health: the largest growth, over the plan's tensors, of the recorded |max| against the level last accepted
    (rebase=True accepts the current one), with the producing layer's name -- one or two forwards old, free to read."""
    f = C.c_double(); amax = C.c_double(); seen = C.c_longlong(); name = C.create_string_buffer(128)
    self.lib.check(self.lib.dll.odt_range_health(self.live(), int(bool(rebase)), C.byref(f), name, 128, C.byref(amax),
                                                 C.byref(seen)))
    return {"worst_growth": f.value, "tensor": name.value.decode(), "tensor_amax": amax.value, "tensors_seen": int(seen.value)}

  def forward_serial(self):
    """odt_forward_serial: the number of forwards enqueued on this handle (the serial of the most recent one)."""
    v = C.c_int64()
    self.lib.check(self.lib.dll.odt_forward_serial(self.live(), C.byref(v)))
    return int(v.value)

  def profile(self, enable):
    self.lib.check(self.lib.dll.odt_profile_enable(self.live(), int(enable)))
    self.profiling = bool(enable)

  def profile_read(self):
    ms = C.c_double(); fl = C.c_double(); n = C.c_int(); tot = C.c_double()
    self.lib.check(self.lib.dll.odt_profile_read(self.live(), C.byref(ms), C.byref(fl), C.byref(n), C.byref(tot)))
    return dict(conv_ms=ms.value, conv_flops=fl.value, conv_launches=n.value, total_ms=tot.value)

  def profile_layers(self):
    """[(name, flops, ms, (M, N, K))] for every conv launch of the plan."""
    h = self.live()
    cnt = C.c_int()
    self.lib.check(self.lib.dll.odt_profile_layer(h, -1, None, 0, None, None, None, C.byref(cnt)))
    out = []
    for i in range(cnt.value):
      name = C.create_string_buffer(128); fl = C.c_double(); ms = C.c_double()
      mnk = (C.c_int64 * 3)()
      self.lib.check(self.lib.dll.odt_profile_layer(h, i, name, 128, C.byref(fl), C.byref(ms), C.cast(mnk, c_i64_p),
                                                    C.byref(cnt)))
      out.append((name.value.decode(), fl.value, ms.value, (mnk[0], mnk[1], mnk[2])))
    return out
