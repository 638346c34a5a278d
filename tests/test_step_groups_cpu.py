"""CPU: llmrec_step_rows_group_f32 (fusion backward + multi-tensor AdamW + softmax backward as one launch) checks its arguments and
refuses what it does not compile before it touches the device - status code + llmrec_last_error, no launch."""
import ctypes as C

from llmrec_amd import _lib, ops

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers
NO_SOFTMAX = (0, 0, 1.0, None, 0, None, 0, None, 0)
OPT = (1e-3, 0.9, 0.999, 1e-8, 0.01)


def _fuse_problem(d, rows=32, n_norm=2):
    keep = [(C.c_void_p * n_norm)(*[FAKE] * n_norm), (C.c_int64 * n_norm)(*[d] * n_norm), (C.c_float * n_norm)(*[0.1] * n_norm)]
    arr = (ops.FuseBwdProblem * 1)()
    pr = arr[0]
    pr.rows, pr.dOut, pr.lddo, pr.n_norm = rows, FAKE, d, n_norm
    pr.norm_terms, pr.norm_ld, pr.rates = C.cast(keep[0], C.c_void_p), C.cast(keep[1], C.c_void_p), C.cast(keep[2], C.c_void_p)
    pr.d_terms, pr.d_ld, pr.src_terms, pr.src_ld = pr.norm_terms, pr.norm_ld, pr.norm_terms, pr.norm_ld
    return arr, keep


def _tensors(n):
    arr = (ops.AdamwTensor * n)()
    for a in arr:
        a.p, a.g, a.m, a.v, a.n, a.g_scale = FAKE, FAKE, FAKE, FAKE, 8, 1.0
    return arr


def test_rows_group_entry_point_is_declared():
    protos = _lib.parse_header()
    assert "llmrec_step_rows_group_f32" in protos and len(protos["llmrec_step_rows_group_f32"][1]) == 21
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8
    chunk = _lib.CONST["LLMREC_ADAMW_CHUNK"]
    assert chunk >= 1024 and chunk % 1024 == 0            # whole float4 rounds of a 256-thread block


def test_rows_group_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_step_rows_group_f32
    fuse64, keep64 = _fuse_problem(64)
    fuse128, keep128 = _fuse_problem(128)
    one, many = _tensors(1), _tensors(_lib.CONST["LLMREC_ADAMW_MAX_TENSORS"] + 1)
    bad = [
        ((-1, None, 64, 0, None, None) + OPT + NO_SOFTMAX, b"step_rows_group"),                            # negative member count
        ((3, fuse64, 64, 0, None, None) + OPT + NO_SOFTMAX, b"fuse_bwd_src_multi"),                        # more than two fusion problems
        ((1, None, 64, 0, None, None) + OPT + NO_SOFTMAX, b"fuse_bwd_src_multi"),                          # problems announced, none given
        ((0, None, 64, len(many), many, FAKE) + OPT + NO_SOFTMAX, b"adamw_multi"),                         # more than LLMREC_ADAMW_MAX_TENSORS
        ((0, None, 64, 1, None, FAKE) + OPT + NO_SOFTMAX, b"adamw_multi"),                                 # tensors announced, none given
        ((0, None, 64, 1, one, None) + OPT + NO_SOFTMAX, b"adamw_multi"),                                  # no optimizer state
        ((0, None, 64, 0, None, None) + OPT + (16, 64, 1.0, None, 64, FAKE, 64, FAKE, 64), b"step_rows_group"),   # softmax rows without Y
        ((0, None, 64, 0, None, None) + OPT + (16, 64, 1.0, FAKE, 32, FAKE, 64, FAKE, 64), b"step_rows_group"),   # ld < d
    ]
    for args, needle in bad:
        assert call(*args, None) == -1, args
        assert needle in lib.llmrec_last_error(), (args, lib.llmrec_last_error())
    # valid arguments outside the compiled instance: LLMREC_EUNSUPPORTED, decided on the host (no launch)
    assert call(1, fuse128, 128, 0, None, None, *OPT, *NO_SOFTMAX, None) == _lib.EUNSUPPORTED
    assert b"step_rows_group" in lib.llmrec_last_error()
    assert call(0, None, 64, 0, None, None, *OPT, 16, 128, 1.0, FAKE, 128, FAKE, 128, FAKE, 128, None) == _lib.EUNSUPPORTED
    assert call(0, None, 64, 0, None, None, *OPT, 16, 64, 1.0, FAKE + 4, 64, FAKE, 64, FAKE, 64, None) == _lib.EUNSUPPORTED   # misaligned rows
    # no member present: nothing to do
    assert call(0, None, 64, 0, None, None, *OPT, *NO_SOFTMAX, None) == 0
    fuse64[0].rows = 0
    assert call(1, fuse64, 64, 0, None, None, *OPT, *NO_SOFTMAX, None) == 0
    del keep64, keep128
