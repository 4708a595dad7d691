"""EfficientNet backbone on the HIP kernels (the part of the EfficientDet path that is built):
``EfficientNetBackbone(name, weights).features(frames)`` -> {level: [B,h,w,C] float32} for the
reduction_1..5 endpoints (reference efficientdet/efficientdet_arch.py:396-437 ``build_backbone``:
levels 3, 4, 5 feed the BiFPN)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import ODT_GRAPH_EFFNET, OdtConfig, _Handle, as_frames
from .arch import backbone_spec


class EfficientNetBackbone(_Handle):

  def __init__(self, name, weights, batch, height, width, device=0, lib=None, det=None, num_classes=90,
               topk=5000, score_thresh=0.0, per_im=100, image_scale=1.0, keep_taps=True):
    self.name, self.batch, self.height, self.width = name, batch, height, width
    self.src_height, self.src_width = height, width
    self.spec = backbone_spec(name)
    c = OdtConfig()
    c.graph = ODT_GRAPH_EFFNET; c.batch = batch; c.height = height; c.width = width
    c.eff_backbone = int(name[-1])
    c.eff_det = -1 if det is None else int(det[-1])      # "efficientdet-dN"
    c.num_class = num_classes; c.eff_topk = topk; c.result_score_thresh = score_thresh
    c.result_per_im = per_im; c.eff_image_scale = image_scale; c.head_nms_thresh = 0.5
    c.keep_taps = int(bool(keep_taps))     # (features() / tap() read stage tensors: the stand-alone backbone keeps them by default)
    _Handle.__init__(self, lib if lib is not None else _lib.get_lib(), c, device, weights.items())

  def set_source_size(self, src_height, src_width):
    """Frames of [B, src_height, src_width, 3]; the reference's input scaling (dataloader.py:100-123)
    runs on the device and the output boxes are multiplied by image_scale_to_original."""
    _Handle.set_source_size(self, src_height, src_width)
    self.src_height, self.src_width = int(src_height), int(src_width)

  def forward_async(self, frames):
    fr, dt = as_frames(frames)
    assert fr.shape == (self.batch, self.src_height, self.src_width, 3), fr.shape
    self._keep = fr
    self.lib.check(self.lib.dll.odt_forward_async(self.live(), fr.ctypes.data_as(C.c_void_p), dt, 0, None))

  def features(self, frames):
    """{level: NHWC float32 [B,h,w,C]} of reduction_1..5 (pad channels stripped)."""
    self.forward_async(frames); self.synchronize()
    out = {}
    for b in self.spec["blocks"]:
      if b["reduction"]:
        out[b["reduction"]] = np.ascontiguousarray(self.tap("reduction_%d" % b["reduction"])[..., :b["cout"]])
    return out
