"""The kernel that hosts an SpMM in the CUs the multi-target weight gradient leaves free (csrc/wgrad_host.hip:
linear_wgrad_bf16x3_v2_multi_host_kernel) must keep its host's footprint, and the host's own kernel (csrc/dense.hip:
linear_wgrad_bf16x3_v2_multi_kernel) must keep the one it had: hipcc's kernel-resource-usage remarks for both files.

The weight gradient's kernel holds exactly one block per CU - 132 096 B of the CU's 160 KB of LDS, one wavefront per SIMD, 390 registers
per lane of the SIMD's unified file of 512 (the remarks report them as 256 architectural + 134 accumulation registers) and no scratch.
The hosting kernel runs the same body in its first blocks and must not pay for the guest there: no scratch, no spilled VGPR, the same
LDS size (the guest's partial sums live in the host's reduction array) and one wavefront per SIMD - so a guest block owns a CU exactly
like a host block, which is what places the guests on the CUs the 224-block layout leaves free."""
import pytest

from tests._hipcc import needs_hipcc, resource_usage

HOSTING = "_ZN6llmrec40linear_wgrad_bf16x3_v2_multi_host_kernelENS_10WgradMultiEiiNS_8SpmmArgsE"
HOST = "_ZN6llmrec35linear_wgrad_bf16x3_v2_multi_kernelENS_10WgradMultiEi"
LDS_PER_CU = 160 * 1024
LDS_BYTES = 132096
UNIFIED_REGISTERS = 512

pytestmark = needs_hipcc


@pytest.fixture(scope="module")
def usage():
    hosting, host = resource_usage("wgrad_host.hip"), resource_usage("dense.hip")
    assert HOSTING in hosting and HOST in host, (sorted(hosting), sorted(k for k in host if "wgrad_bf16x3_v2" in k))
    assert HOSTING not in host                                  # (its own translation unit: dense.hip's device code is the parent's)
    print("[wgrad host resources] hosting %s\n[wgrad host resources] host    %s" % (hosting[HOSTING], host[HOST]))
    return hosting[HOSTING], host[HOST]


def test_hosting_kernel_keeps_its_hosts_footprint(usage):
    hosting, host = usage
    assert hosting["ScratchSize [bytes/lane]"] == 0 and hosting["VGPRs Spill"] == 0, hosting
    assert hosting["LDS Size [bytes/block]"] == LDS_BYTES == host["LDS Size [bytes/block]"], (hosting, host)
    assert LDS_PER_CU // hosting["LDS Size [bytes/block]"] == 1                      # one block per CU, guest or host
    assert hosting["Occupancy [waves/SIMD]"] == 1 == host["Occupancy [waves/SIMD]"], (hosting, host)
    assert hosting["VGPRs"] + hosting["AGPRs"] <= UNIFIED_REGISTERS, hosting


def test_weight_gradient_kernel_is_unchanged(usage):
    _, host = usage
    assert host["VGPRs"] + host["AGPRs"] == 390, host                               # (256 architectural + 134 accumulation)
    assert host["ScratchSize [bytes/lane]"] == 0 and host["VGPRs Spill"] == 0, host
    assert host["LDS Size [bytes/block]"] == LDS_BYTES, host
