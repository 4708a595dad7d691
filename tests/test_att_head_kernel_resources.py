"""Build-time guard for csrc/att_head.hip (test_kernel_resources.py's compile-time report): the file holds exactly the pooling
kernel and the add kernel of the box head's attention branch; both are bound by HBM -- no scratch memory, and at least four
waves per SIMD, so that a CU keeps enough 16-byte loads in flight."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_att_head_kernels_use_no_scratch_and_keep_four_waves():
  res = _resources("att_head.hip")
  pool = [k for k in res if "att_pool_kernel" in k]
  add = [k for k in res if "att_add_kernel" in k]
  assert len(pool) == 1 and len(add) == 1 and len(res) == 2, sorted(res)
  print("att_head.hip:", res)
  for k, v in res.items():
    assert v.get("scratch", 0) == 0, (k, v)
    assert v.get("occupancy", 0) >= 4, (k, v)
