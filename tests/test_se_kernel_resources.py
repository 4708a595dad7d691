"""Build-time guard for csrc/resnet_se.hip (on the pattern of test_kernel_resources.py): no scratch memory in the SE kernels,
and the apply kernel -- a streaming kernel that needs loads in flight, not registers -- keeps at least 4 waves per SIMD."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_se_kernels_use_no_scratch_and_apply_keeps_occupancy():
  res = _resources("resnet_se.hip")
  apply = {k: v for k, v in res.items() if "resnet_se_apply_kernel" in k}
  gates = {k: v for k, v in res.items() if "resnet_se_reduce_kernel" in k or "resnet_se_expand_kernel" in k}
  assert len(apply) == 1 and len(gates) == 2, sorted(res)
  for k, v in list(apply.items()) + list(gates.items()):
    assert v.get("scratch", -1) == 0, (k, v)
  for k, v in apply.items():
    assert v.get("occupancy", 0) >= 4, (k, v)
