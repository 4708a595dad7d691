"""Build-time guard for csrc/group_norm_roi.hip (test_kernel_resources.py's compile-time report): the ROI GroupNorm kernel
keeps a ROI's share in registers between its one load and its one store and is bound by HBM -- no scratch memory, and at least
four waves per SIMD, so that a CU keeps enough 16-byte loads in flight."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_group_norm_roi_kernel_uses_no_scratch_and_keeps_four_waves():
  res = _resources("group_norm_roi.hip")
  roi = {k: v for k, v in res.items() if "group_norm_roi_kernel" in k}
  assert len(roi) == 1 and len(res) == 1, sorted(res)
  for k, v in roi.items():
    assert v.get("scratch", 0) == 0, (k, v)
    assert v.get("occupancy", 0) >= 4, (k, v)
