"""Build-time guard for csrc/conv_group.hip (on the pattern of test_se_kernel_resources.py): no scratch memory in any
instantiation of the grouped conv, and the streaming instantiations (G = 4 and 8) -- kernels that need loads in flight, not
registers -- keep at least 4 waves per SIMD."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_group_conv_kernels_use_no_scratch_and_streaming_keeps_occupancy():
  res = _resources("conv_group.hip")
  stream = {k: v for k, v in res.items() if "group_conv_stream_kernel" in k}
  mfma = {k: v for k, v in res.items() if "group_conv_mfma_kernel" in k}
  assert len(stream) == 8 and len(mfma) == 2, sorted(res)      # G in {4, 8} x stride x dilation; G in {16, 32}
  for k, v in list(stream.items()) + list(mfma.items()):
    assert v.get("scratch", -1) == 0, (k, v)
  for k, v in stream.items():
    assert v.get("occupancy", 0) >= 4, (k, v)
