"""hipcc's kernel-resource-usage remarks for one .hip file of llmrec_amd/csrc, compiled for gfx950 (device code only, nothing written):
{mangled kernel name: {remark: value}}. One compile per file and test process - the CPU tests that read the remarks share it."""
import functools
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llmrec_amd", "csrc")
KEYS = ("VGPRs", "AGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]")

needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")


@functools.lru_cache(maxsize=None)
def resource_usage(source_path):
    """source_path: absolute, or a file name under llmrec_amd/csrc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, os.path.join(CSRC, source_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
        for key in KEYS:
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur].setdefault(key, int(m.group(1)))
    return res
