"""Build-time guard for csrc/relation.hip (test_kernel_resources.py's compile-time report): the file holds exactly the geometric
bias kernel and the attention kernel, neither uses scratch memory -- the 16 accumulators of a pair and the four 16 x 16 output
tiles of a wave stay in registers -- and the attention kernel's LDS (16 score rows of up to 1024 columns) fits the 160 KB of a
CU.  Occupancy is reported in DESIGN.md, not fixed here beyond one wave."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, _resources


def _lds(src):
  """{kernel: LDS bytes per workgroup} from the same compile-time report (_resources does not read that line)."""
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-c",
                      "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                      os.path.join(CSRC, src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
  assert r.returncode == 0, r.stderr[-2000:]
  out, cur = {}, None
  for line in r.stderr.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
      cur = m.group(1)
    m = re.search(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", line)
    if m and cur:
      out[cur] = int(m.group(1))
  return out


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ, reason="hipcc not installed")
def test_relation_kernels_use_no_scratch_and_fit_lds():
  res = _resources("relation.hip")
  geo = [k for k in res if "relation_geo_kernel" in k]
  att = [k for k in res if "relation_attention_kernel" in k]
  assert len(geo) == 1 and len(att) == 1 and len(res) == 2, sorted(res)
  for k, v in res.items():
    assert v.get("scratch", 0) == 0, (k, v)
    assert v.get("occupancy", 0) >= 1, (k, v)
  lds = _lds("relation.hip")
  print("relation.hip:", res, lds)
  assert 16 * 1024 * 4 <= lds[att[0]] <= 160 * 1024, lds
  assert lds[geo[0]] >= 1360 * 4, lds
