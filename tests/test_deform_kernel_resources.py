"""Build-time guard for csrc/conv_deform.hip (on the pattern of test_group_conv_kernel_resources.py): no scratch memory in the
offset kernel or in any instantiation of the deformable conv, and the gather / GEMM kernel -- whose gathers of one slice run
under the MFMAs of another wave -- keeps at least 2 waves per SIMD (two 4-wave workgroups per CU)."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_deform_kernels_use_no_scratch_and_keep_two_waves_per_simd():
  res = _resources("conv_deform.hip")
  off = {k: v for k, v in res.items() if "deform_offset_kernel" in k}
  conv = {k: v for k, v in res.items() if "deform_conv_kernel" in k}
  assert len(off) == 1 and len(conv) == 3 and len(res) == 4, sorted(res)      # C in {128, 256, 512}
  for k, v in res.items():
    assert v.get("scratch", -1) == 0, (k, v)
  for k, v in conv.items():
    assert v.get("occupancy", 0) >= 2, (k, v)
