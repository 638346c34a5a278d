"""CPU: llmrec_bpr_scatter_plan_reach_mark and llmrec_fuse_fwd_multi_sumsq_compact_f32 check their arguments and refuse what they do not
compile before they touch the device - status code + llmrec_last_error, no launch."""
import ctypes as C

from llmrec_amd import _lib, ops

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers


def test_the_rider_entry_points_are_declared():
    protos = _lib.parse_header()
    assert len(protos["llmrec_bpr_scatter_plan_reach_mark"][1]) == 12
    assert len(protos["llmrec_fuse_fwd_multi_sumsq_compact_f32"][1]) == 12
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8


def test_plan_reach_mark_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_bpr_scatter_plan_reach_mark
    ok = [FAKE, FAKE, FAKE, 64, None, FAKE, 100, 50, FAKE, FAKE, FAKE]
    bad = []
    for pos, value in ((3, -1), (6, 0), (6, 1 << 31), (7, 0), (8, None), (9, None), (10, None), (0, None), (5, None)):
        a = list(ok); a[pos] = value
        bad.append(a)
    for a in bad:
        assert call(*a, None) == -1, a
        assert b"bpr_scatter_plan_reach_mark" in lib.llmrec_last_error()
    big = list(ok); big[3] = _lib.CONST["LLMREC_BPR_MAX_B"] + 1
    assert call(*big, None) == _lib.EUNSUPPORTED
    empty = list(ok); empty[3] = 0
    assert call(*empty, None) == 0                                       # an empty capacity: nothing to do


def test_fusion_compact_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_fuse_fwd_multi_sumsq_compact_f32
    d = 64
    keep = [(C.c_void_p * 1)(FAKE), (C.c_int64 * 1)(d), (C.c_void_p * 2)(FAKE, FAKE), (C.c_int64 * 2)(d, d), (C.c_float * 2)(0.1, 0.1)]
    arr = (ops.FuseFwdProblem * 1)()
    pr = arr[0]
    pr.rows, pr.mean_scale, pr.n_mean, pr.n_norm = 32, 1.0, 1, 2
    pr.mean_terms, pr.mean_ld = C.cast(keep[0], C.c_void_p), C.cast(keep[1], C.c_void_p)
    pr.norm_terms, pr.norm_ld, pr.rates = C.cast(keep[2], C.c_void_p), C.cast(keep[3], C.c_void_p), C.cast(keep[4], C.c_void_p)
    pr.out, pr.ldo = FAKE, d
    n_part = C.c_int32(0)
    head = (1, arr, d, 2, FAKE, 4096, C.byref(n_part))
    for tail in ((0, FAKE, FAKE, FAKE), (1 << 31, FAKE, FAKE, FAKE), (100, None, FAKE, FAKE), (100, FAKE, None, FAKE), (100, FAKE, FAKE, None),
                 (100, FAKE + 4, FAKE, FAKE)):                           # flags that are not 16-byte aligned
        assert call(*head, *tail, None) == -1, tail
        assert b"fuse_fwd_multi_sumsq_compact" in lib.llmrec_last_error()
    assert call(3, arr, d, 2, FAKE, 4096, C.byref(n_part), 100, FAKE, FAKE, FAKE, None) == -1        # the fusion's own checks still hold
    assert call(1, arr, d, 2, FAKE, 0, C.byref(n_part), 100, FAKE, FAKE, FAKE, None) != 0            # no room for the partial sums
    # valid arguments outside the compiled float4 family: refused on the host, nothing launched
    pr.out = FAKE + 4
    assert call(*head, 100, FAKE, FAKE, FAKE, None) == _lib.EUNSUPPORTED
    assert b"fuse_fwd_multi_sumsq_compact" in lib.llmrec_last_error()
    pr.out = FAKE
    keep[1][0] = keep[3][0] = keep[3][1] = 66
    pr.ldo = 66
    assert call(1, arr, 66, 2, FAKE, 4096, C.byref(n_part), 100, FAKE, FAKE, FAKE, None) == _lib.EUNSUPPORTED
    del keep


def test_wide_sampler_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_sample_batch_wide
    assert len(_lib.parse_header()["llmrec_sample_batch_wide"][1]) == 19
    ok = [1, FAKE, 10, FAKE, 5, FAKE, FAKE, 16, 0, 16, 4, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE]
    for pos, value in ((9, 0), (7, 8), (8, 1), (10, 17), (10, -1), (2, 0), (4, 0), (1, None), (3, None), (13, None), (16, None), (17, None),
                       (11, None), (12, None)):                          # sizes, null pointers (the ticket among them), missing pairs
        a = list(ok); a[pos] = value
        assert call(*a, None) == -1, (pos, value)
        assert b"sample_batch_wide" in lib.llmrec_last_error()
