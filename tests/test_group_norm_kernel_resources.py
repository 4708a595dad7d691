"""Build-time guard for csrc/group_norm.hip (test_kernel_resources.py's compile-time report): the statistics and apply
kernels are streaming kernels bound by HBM -- no scratch memory in any kernel of the file, and at least four waves per SIMD for
the two that pass over the tensor, so that a CU keeps enough 16-byte loads in flight."""
import os

import pytest

from test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_group_norm_kernels_use_no_scratch_and_keep_four_waves():
  res = _resources("group_norm.hip")
  stats = {k: v for k, v in res.items() if "group_norm_stats_kernel" in k}
  apply = {k: v for k, v in res.items() if "group_norm_apply_kernel" in k}
  final = {k: v for k, v in res.items() if "group_norm_finalize_kernel" in k}
  assert len(stats) == 1 and len(apply) == 3 and len(final) == 1, sorted(res)
  for k, v in res.items():
    assert v.get("scratch", 0) == 0, (k, v)
  for k, v in list(stats.items()) + list(apply.items()):
    assert v.get("occupancy", 0) >= 4, (k, v)
