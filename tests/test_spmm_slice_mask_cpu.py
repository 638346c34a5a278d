"""CPU: the slice-masked SpMM instances (llmrec_spmm_epilogue_t.x_mask_stamp) - the single, the grouped and the loss-values guest kernel
each keep the 5 waves per SIMD of their host (the weighted float4 16-lane spmm_kernel) without scratch, and the guest instance leaves
the LDS room a guest instance must (hipcc's resource remarks); no other instance of them is compiled; the entry points check the new
fields and refuse what is not compiled before any launch."""
import ctypes as C
import re

from llmrec_amd import _lib, ops
from tests._hipcc import needs_hipcc, resource_usage

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers


@needs_hipcc
def test_slice_masked_kernels_keep_their_hosts_occupancy():
    res = resource_usage("spmm.hip")
    host = res["_ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb1ELb0EEEvNS_8SpmmArgsE"]
    assert host["Occupancy [waves/SIMD]"] == 5
    masked = {n: u for n, u in res.items() if re.match(r"_ZN6llmrec\d+spmm_smask_", n)}
    assert sorted(masked) == ["_ZN6llmrec17spmm_smask_kernelILi16ELi1ELi4EEEvNS_8SpmmArgsE",
                              "_ZN6llmrec23spmm_smask_multi_kernelILi16ELi1ELi4EEEvNS_9SpmmMultiE",
                              "_ZN6llmrec29spmm_smask_multi_guest_kernelINS_10LossesArgsEEEvNS_14SpmmMultiGuestIT_EE"], sorted(masked)
    for name, u in masked.items():
        assert u["Occupancy [waves/SIMD]"] == host["Occupancy [waves/SIMD]"], (name, u, host)
        assert u.get("ScratchSize [bytes/lane]", 0) == 0, (name, u)
        # LDS (the loss values request no dynamic LDS): a CU has 160 KB and 4 SIMDs, a block is 8 wavefronts
        blocks_by_occupancy = u["Occupancy [waves/SIMD]"] * 4 // 8
        assert (160 * 1024) // u["LDS Size [bytes/block]"] >= blocks_by_occupancy and u["LDS Size [bytes/block]"] <= 64 * 1024, (name, u)
    single, multi = (masked[n] for n in sorted(masked)[:2])
    assert single["LDS Size [bytes/block]"] == multi["LDS Size [bytes/block]"] == host["LDS Size [bytes/block]"]


def _call(lib, d, sw, epi, col_scale=FAKE, val=None, n=1, guest=None):
    plan = ops.SpmmPlanC(128, 2048, 2048, 0, None, 0, None, 0, None, None, 0, None, 0, None)
    prs = (ops.SpmmProblemC * n)(*[ops.SpmmProblemC(300, 200, FAKE, FAKE, val, None, col_scale, FAKE, d, FAKE + 0x100000 * (q + 1), d, d, sw,
                                                     C.addressof(plan), None, C.addressof(epi) if epi is not None else None) for q in range(n)])
    if guest is not None:
        return lib.llmrec_spmm_multi_guest_f32(n, prs, C.byref(guest), None)
    return lib.llmrec_spmm_multi_f32(n, prs, None)


def test_entry_points_check_the_mask_and_refuse_before_any_launch():
    lib = _lib.load()
    E = ops.SpmmEpilogueC
    # the fields' own checks: a stamp without mask bytes, a slice out of range, company the mask excludes
    assert _call(lib, 448, 64, E(x_mask_stamp=FAKE, mask_from_slice=2)) == -1 and b"x_mask_stamp" in lib.llmrec_last_error()
    assert _call(lib, 448, 64, E(x_row_mask=FAKE, x_mask_stamp=FAKE, mask_from_slice=8)) == -1
    assert _call(lib, 448, 64, E(x_row_mask=FAKE, x_mask_stamp=FAKE, mask_from_slice=-1)) == -1
    for extra in (dict(y_row_flag=FAKE), dict(y_row_gate=FAKE), dict(y_row_needed=FAKE, x_mask_active=1), dict(rows_listed_only=1)):
        assert _call(lib, 448, 64, E(x_row_mask=FAKE, x_mask_stamp=FAKE, mask_from_slice=2, **extra)) == -1, extra
        assert b"x_mask_stamp excludes" in lib.llmrec_last_error()
    assert _call(lib, 64, 0, E(op=ops.EPI_SOFTMAX_BWD, S=FAKE, lds=64, x_row_mask=FAKE, x_mask_stamp=FAKE)) == -1
    # shapes and variants that are not compiled: refused, nothing launched (no device here to launch on)
    ok = dict(x_row_mask=FAKE, x_mask_stamp=FAKE)
    for d, sw in ((16, 0), (32, 0), (128, 0), (448, 0), (62, 0)):
        assert _call(lib, d, sw, E(mask_from_slice=0, **ok)) == _lib.EUNSUPPORTED, (d, sw)
        assert b"slice-masked" in lib.llmrec_last_error()
    assert _call(lib, 448, 64, E(mask_from_slice=2, **ok), col_scale=None) == _lib.EUNSUPPORTED            # unweighted
    assert b"no col_scale" in lib.llmrec_last_error()
    assert _call(lib, 448, 64, E(mask_from_slice=2, **ok), val=FAKE) == _lib.EUNSUPPORTED                  # weighted by val
    assert b"has val" in lib.llmrec_last_error()
    g = ops.SpmmGuestC(kind=ops.GUEST_PLAN_REACH)
    g.u.plan_reach = ops.GuestPlanReachC(users=FAKE, pos=FAKE, neg=FAKE, B_max=64, n_valid_dev=None, plan=FAKE, n_users=100, n_items=50,
                                         item_rowptr=FAKE, item_colidx=FAKE, flags=FAKE)
    assert _call(lib, 448, 64, E(mask_from_slice=2, **ok), guest=g) == _lib.EUNSUPPORTED
    assert b"loss values only" in lib.llmrec_last_error()
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8


def test_companions_the_masked_instance_cannot_run_are_refused():
    """A grouped launch takes along only companions weighted by col_scale alone and without y_row_needed: the masked pipeline reads no
    val and computes every row. Anything else keeps its variant and the group is refused like any mixed one, before a launch."""
    lib = _lib.load()
    E = ops.SpmmEpilogueC
    plan = ops.SpmmPlanC(128, 2048, 2048, 0, None, 0, None, 0, None, None, 0, None, 0, None)
    masked = E(x_row_mask=FAKE, x_mask_stamp=FAKE, mask_from_slice=2)
    needed = E(y_row_needed=FAKE, x_mask_active=1)

    def problem(q, d, sw, epi, val, col_scale):
        return ops.SpmmProblemC(300, 200, FAKE, FAKE, val, None, col_scale, FAKE, d, FAKE + 0x100000 * (q + 1), d, d, sw, C.addressof(plan),
                                None, C.addressof(epi) if epi is not None else None)
    side = problem(0, 448, 64, masked, None, FAKE)
    w = (C.c_float * 8)(*[1.0] * 8)
    g = ops.SpmmGuestC(kind=ops.GUEST_LOSSES)
    g.u.losses = ops.GuestLossesC(n_problems=8, B_max=64, n_valid_dev=None, remember_rate=0.5, decay=1e-5, batch_size_flag=64.0, out=FAKE,
                                  saved=FAKE, w_mf_host=C.cast(w, C.c_void_p), sumsq_partial=None, n_partial=0, feat_reg_coef=0.0, scal4=FAKE,
                                  running_sums3=None)
    for what, comp in (("val alone", problem(1, 64, 0, None, FAKE, None)), ("val and col_scale", problem(1, 64, 0, None, FAKE, FAKE)),
                       ("y_row_needed", problem(1, 64, 0, needed, None, FAKE)), ("unweighted", problem(1, 64, 0, None, None, None))):
        for order in ((side, comp), (comp, side)):
            prs = (ops.SpmmProblemC * 2)(*order)
            assert lib.llmrec_spmm_multi_f32(2, prs, None) == _lib.EUNSUPPORTED, what
            assert b"another kernel instance" in lib.llmrec_last_error(), what
            assert lib.llmrec_spmm_multi_guest_f32(2, prs, C.byref(g), None) == _lib.EUNSUPPORTED, what
