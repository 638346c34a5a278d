"""The kernel that hosts an SpMM behind the grouped projection's work units (csrc/dense.hip: linear_fwd_grouped_bf16x3_host_kernel) must
not pay for its guest with the projection's residency: hipcc's kernel-resource-usage remarks for dense.hip.

test_hosting_kernel_within_128_vgprs: the bound the hosting kernel was specified with - at most 128 VGPRs, no scratch, LDS for two blocks
per CU. The kernel is compiled with __launch_bounds__(256, 4) for it: 108 VGPRs (the projection's own kernel, under (256, 2), takes 140).

test_hosting_kernel_keeps_its_hosts_residency: against the kernel it hosts in, linear_fwd_grouped_bf16x3_kernel<4, 2, 3> - the same waves
per SIMD, no scratch, as many blocks per CU by LDS as the host, and registers that allow that residency: a SIMD's unified file holds 512
registers per lane, architectural and accumulation registers together, so w resident waves may have 512 // w each (the capped build keeps
some values in accumulation registers: 108 + 44)."""
import pytest

from tests._hipcc import needs_hipcc, resource_usage

HOSTING = "_ZN6llmrec37linear_fwd_grouped_bf16x3_host_kernelENS_11LinearGroupEiiNS_8SpmmArgsE"
HOST = "_ZN6llmrec32linear_fwd_grouped_bf16x3_kernelILi4ELi2ELi3EEEvNS_11LinearGroupEi"
LDS_PER_CU = 160 * 1024

pytestmark = needs_hipcc


@pytest.fixture(scope="module")
def usage():
    res = resource_usage("dense.hip")
    assert HOSTING in res and HOST in res, sorted(k for k in res if "grouped_bf16x3" in k)
    print("[host chain resources] hosting %s\n[host chain resources] host    %s" % (res[HOSTING], res[HOST]))
    return res


def test_hosting_kernel_keeps_its_hosts_residency(usage):
    hosting, host = usage[HOSTING], usage[HOST]
    assert hosting["ScratchSize [bytes/lane]"] == 0 and hosting["VGPRs Spill"] == 0, hosting
    assert hosting["Occupancy [waves/SIMD]"] == host["Occupancy [waves/SIMD]"], (hosting, host)
    assert hosting["VGPRs"] + hosting["AGPRs"] <= 512 // host["Occupancy [waves/SIMD]"], (hosting, host)
    # a block is 4 wavefronts, one per SIMD: waves per SIMD = blocks per CU, if the LDS has room for as many
    assert LDS_PER_CU // hosting["LDS Size [bytes/block]"] >= hosting["Occupancy [waves/SIMD]"], hosting
    assert LDS_PER_CU // hosting["LDS Size [bytes/block]"] == LDS_PER_CU // host["LDS Size [bytes/block]"], (hosting, host)


def test_hosting_kernel_within_128_vgprs(usage):
    hosting = usage[HOSTING]
    assert hosting["ScratchSize [bytes/lane]"] == 0 and hosting["VGPRs Spill"] == 0, hosting
    assert LDS_PER_CU // hosting["LDS Size [bytes/block]"] >= 2, hosting
    assert hosting["VGPRs"] <= 128, hosting
