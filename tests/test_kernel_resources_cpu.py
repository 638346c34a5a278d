"""Every hand-written kernel compiles for gfx950 without scratch (no register spills, no private arrays): hipcc's own
kernel-resource-usage remarks for the six .hip files. A spill in one of the sweeps or GEMMs costs tens of per cent and is silent otherwise
(the register allocator of this toolchain is sensitive to small source changes - profiles/experiments/r05_topk.md)."""
import os
from concurrent.futures import ThreadPoolExecutor

from tests._hipcc import needs_hipcc, resource_usage


@needs_hipcc
def test_no_hand_written_kernel_uses_scratch():
    from llmrec_amd.build import SOURCES
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as ex:
        res = dict(zip(SOURCES, ex.map(resource_usage, SOURCES)))
    n = 0
    for src, kernels in res.items():
        assert kernels, src
        for name, u in kernels.items():
            if "rocprim" in name or "hipcub" in name:          # (the vendor radix sort of the CSR build keeps private arrays)
                continue
            n += 1
            assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (src, name, u)
    assert n > 100, n
    # the bench's two sweeps keep four blocks per CU (the bf16 sweep lives on its resident wavefronts: a second tile in flight at three blocks
    # per CU measured 0.57 ms against 0.31)
    tk = res["topk.hip"]
    pre = [u for k, u in tk.items() if "score_topk_pre_kernelILi2" in k]
    exact = [u for k, u in tk.items() if "score_topk_kernelILi4ELb1ELb1" in k]
    assert pre and exact
    assert pre[0]["Occupancy [waves/SIMD]"] == 4 and exact[0]["Occupancy [waves/SIMD]"] == 4, (pre, exact)
