"""CPU: the guest launch (llmrec_spmm_multi_guest_f32) - every guest instance keeps the waves per SIMD of its host spmm_kernel instance
without scratch, and its LDS leaves room for the blocks that occupancy allows (hipcc's resource remarks); the entry point checks a guest
like the guest's own entry point, before any launch. (The call sequence of a guest-path step needs a device:
tests/test_gpu_spmm_guests.py; the layout of llmrec_spmm_guest_t and its members: tests/test_abi_layout_cpu.py.)"""
import ctypes as C
import re

from llmrec_amd import _lib, ops
from tests._hipcc import needs_hipcc, resource_usage

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers


@needs_hipcc
def test_guest_kernels_keep_their_hosts_occupancy():
    res = resource_usage("spmm.hip")
    host = lambda w: res["_ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb%dELb0EEEvNS_8SpmmArgsE" % w]
    assert host(0)["Occupancy [waves/SIMD]"] == 7 and host(1)["Occupancy [waves/SIMD]"] == 5
    # _ZN6llmrec23spmm_multi_guest_kernelILb0ENS_11SamplerArgsEEEvNS_14SpmmMultiGuestIT0_EE
    seen = set()
    for name, u in res.items():
        m = re.match(r"_ZN6llmrec23spmm_multi_guest_kernelILb([01])ENS_\d+(\w+?Args)EEEvNS_14SpmmMultiGuestIT0_EE$", name)
        if not m:
            continue
        w, guest = int(m.group(1)), m.group(2)
        assert u["Occupancy [waves/SIMD]"] == host(w)["Occupancy [waves/SIMD]"], (name, u, host(w))
        assert u.get("ScratchSize [bytes/lane]", 0) == 0, (name, u)
        # LDS: static + the launch's dynamic request (the plan's 2 B_max keys at the bench's B_max = 1126, and at the largest accepted
        # capacity); a CU has 160 KB and 4 SIMDs, a block is 8 wavefronts
        blocks_by_occupancy = u["Occupancy [waves/SIMD]"] * 4 // 8
        for b_max in (1126, _lib.CONST["LLMREC_SPMM_GUEST_MAX_PLAN_B"]):
            dynamic = 16 * b_max if guest == "PlanReachArgs" else 0
            assert (160 * 1024) // (u["LDS Size [bytes/block]"] + dynamic) >= blocks_by_occupancy, (name, u, b_max)
            assert u["LDS Size [bytes/block]"] + dynamic <= 64 * 1024
        seen.add((w, guest))
    assert seen == {(w, g) for w in (0, 1) for g in ("SamplerArgs", "PlanReachArgs", "LossesArgs")}, seen
    # the grouped and the single kernels are the ones tests/test_spmm_multi_cpu.py counts: no further spmm_multi_kernel instance
    assert sum(1 for n in res if re.match(r"_ZN6llmrec17spmm_multi_kernelI", n)) == 14


def _sampler_guest(**over):
    a = dict(seed=1, step_dev=FAKE, n_exist_users=10, exist_users=FAKE, n_items=5, train_rowptr=FAKE, train_colidx=FAKE, B_global=16,
             slice_begin=0, B=16, n_aug=4, aug_pos=FAKE, aug_neg=FAKE, users=FAKE, pos=FAKE, neg=FAKE, n_valid_dev=FAKE, ticket=FAKE)
    a.update(over)
    g = ops.SpmmGuestC(kind=ops.GUEST_SAMPLER)
    g.u.sampler = ops.GuestSamplerC(**a)
    return g


def test_guest_entry_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_spmm_multi_guest_f32
    assert call(0, None, None, None) == -1 and b"spmm_multi_guest" in lib.llmrec_last_error()          # no guest
    g = ops.SpmmGuestC(kind=9)
    assert call(0, None, C.byref(g), None) == -1 and b"unknown guest kind" in lib.llmrec_last_error()
    # the guest's own checks, with the guest's own status codes
    for over in (dict(B=0), dict(n_aug=17), dict(slice_begin=1), dict(ticket=None), dict(users=None), dict(aug_pos=None)):
        assert call(0, None, C.byref(_sampler_guest(**over)), None) == -1, over
        assert b"spmm_multi_guest (sampler)" in lib.llmrec_last_error()
    g = ops.SpmmGuestC(kind=ops.GUEST_PLAN_REACH)
    ok = dict(users=FAKE, pos=FAKE, neg=FAKE, B_max=64, n_valid_dev=None, plan=FAKE, n_users=100, n_items=50, item_rowptr=FAKE,
              item_colidx=FAKE, flags=FAKE)
    for over in (dict(B_max=-1), dict(n_users=0), dict(flags=None), dict(plan=None)):
        g.u.plan_reach = ops.GuestPlanReachC(**dict(ok, **over))
        assert call(0, None, C.byref(g), None) == -1, over
        assert b"spmm_multi_guest (plan + reach marks)" in lib.llmrec_last_error()
    for b_max in (_lib.CONST["LLMREC_BPR_MAX_B"] + 1, 0):                                              # too large; empty: nothing to host
        g.u.plan_reach = ops.GuestPlanReachC(**dict(ok, B_max=b_max))
        assert call(0, None, C.byref(g), None) == _lib.EUNSUPPORTED
    w = (C.c_float * 8)(*[1.0] * 8)
    g = ops.SpmmGuestC(kind=ops.GUEST_LOSSES)
    ok = dict(n_problems=8, B_max=64, n_valid_dev=None, remember_rate=0.5, decay=1e-5, batch_size_flag=64.0, out=FAKE, saved=FAKE,
              w_mf_host=C.cast(w, C.c_void_p), sumsq_partial=None, n_partial=0, feat_reg_coef=0.0, scal4=FAKE, running_sums3=None)
    for over in (dict(n_problems=0), dict(n_problems=9), dict(out=None), dict(w_mf_host=None), dict(n_partial=5)):
        g.u.losses = ops.GuestLossesC(**dict(ok, **over))
        assert call(0, None, C.byref(g), None) == -1, over
        assert b"spmm_multi_guest (loss values)" in lib.llmrec_last_error()
    # a valid guest without a non-empty problem to host it: refused, the caller issues the guest's own entry point
    g.u.losses = ops.GuestLossesC(**ok)
    assert call(0, None, C.byref(g), None) == _lib.EUNSUPPORTED
    assert call(0, None, C.byref(_sampler_guest()), None) == _lib.EUNSUPPORTED
