"""CPU: the grouped SpMM launch (llmrec_spmm_multi_f32) - the grouped kernels keep the registers and occupancy of the single-problem
kernels they group (hipcc's resource remarks). (The layout of llmrec_spmm_problem_t: tests/test_abi_layout_cpu.py.)"""
import re

from tests._hipcc import needs_hipcc, resource_usage


@needs_hipcc
def test_grouped_kernels_keep_the_single_kernels_occupancy():
    res = resource_usage("spmm.hip")
    # _ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb0ELb0EEEvNS_8SpmmArgsE <-> _ZN6llmrec17spmm_multi_kernelILi16ELi1ELi4ELb0ELb0EEEvNS_9SpmmMultiE
    pairs = 0
    for name, u in res.items():
        m = re.match(r"_ZN6llmrec17spmm_multi_kernel(I.*E)EvNS_9SpmmMultiE$", name)
        if not m:
            continue
        single = res.get("_ZN6llmrec11spmm_kernel%sEvNS_8SpmmArgsE" % m.group(1))
        assert single is not None, name
        assert u["Occupancy [waves/SIMD]"] == single["Occupancy [waves/SIMD]"], (name, u, single)
        assert u["LDS Size [bytes/block]"] == single["LDS Size [bytes/block]"] and u.get("ScratchSize [bytes/lane]", 0) == 0, (name, u)
        pairs += 1
    assert pairs == 14, pairs                      # 7 vector-load families x {unweighted, weighted}
    # the bench's two instances (d = 64): registers as before the grouped launch existed
    k = lambda w: "_ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb%dELb0EEEvNS_8SpmmArgsE" % w
    assert res[k(0)]["VGPRs"] == 71 and res[k(0)]["Occupancy [waves/SIMD]"] == 7
    assert res[k(1)]["VGPRs"] == 90 and res[k(1)]["Occupancy [waves/SIMD]"] == 5
