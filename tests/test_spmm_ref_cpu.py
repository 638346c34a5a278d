"""CPU: the yardstick of tests/test_gpu_spmm_families.py is itself checked - the derived error bounds of tests/_spmm_ref.py hold for
fp32 emulations of the three epilogue ops in four summation orders (and are not vacuous), the case table reaches every SpMM kernel
(family, variant) in every row bucket and every alignment trigger, and the host refuses what lies outside the compiled families before
anything is launched (fake device pointers: the argument checks never dereference them). No test here needs a device; the last one
uses one, if present, only so that a call which passes its checks never launches over fake pointers."""
import ctypes as C
import dataclasses

import numpy as np
import torch

from llmrec_amd import _lib, ops

from tests import _spmm_ref as R

FAKE = 0x10000            # a 16-byte aligned "device" address
EHIP = -2                 # LLMREC_EHIP
ORDERS = ("forward", "reverse", "pairwise", "chunks16")
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _fma(w, x, acc):
    """fmaf(w, x, acc) per element: the product is exact in float64, one rounding to fp32 (up to a double rounding in the last place)"""
    return (np.float64(w) * x.astype(np.float64) + acc.astype(np.float64)).astype(F32)


def _pairwise(v):
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.concatenate([v, np.zeros((1,) + v.shape[1:], F32)])
        v = (v[0::2] + v[1::2]).astype(F32)
    return v[0]


def _row_sum(w, xs, order):
    """sum_j w_j xs[j] in fp32 (w None: plain additions), xs [n, d]"""
    n, d = xs.shape
    acc = np.zeros(d, F32)
    if n == 0:
        return acc
    if order in ("forward", "reverse"):
        idx = range(n) if order == "forward" else range(n - 1, -1, -1)
        for j in idx:
            acc = _fma(w[j], xs[j], acc) if w is not None else (acc + xs[j]).astype(F32)
        return acc
    if order == "pairwise":
        return _pairwise((w[:, None] * xs).astype(F32) if w is not None else xs)
    sums = []
    for b in range(0, n, 16):
        sums.append(_row_sum(None if w is None else w[b:b + 16], xs[b:b + 16], "forward"))
    for s in sums:
        acc = (acc + s).astype(F32)
    return acc


def _accumulate(case, order):
    """the unscaled row sums of a case in fp32, inactive columns skipped as the masked kernels do"""
    rowptr, colidx, _ = R.graph()
    inp = R.inputs(case)
    w = None
    if inp["val"] is not None or inp["cs"] is not None:
        w = inp["val"] if inp["val"] is not None else np.ones(colidx.size, F32)
        if inp["cs"] is not None:
            w = (w * inp["cs"][colidx]).astype(F32)
    out = np.zeros((R.N_ROWS, case.d), F32)
    for r in range(R.N_ROWS):
        sl = slice(rowptr[r], rowptr[r + 1])
        cols = colidx[sl]
        keep = np.ones(cols.size, bool) if inp["mask"] is None else inp["mask"][cols] == R.STAMP
        out[r] = _row_sum(None if w is None else w[sl][keep], inp["X"][cols[keep]], order)
    return out


def _vec_sum(v, order):
    """row sums of v [rows, d] in fp32"""
    if order == "pairwise":
        return _pairwise(np.ascontiguousarray(v.T))
    if order == "chunks16":
        parts = [np.cumsum(v[:, b:b + 16], axis=1, dtype=F32)[:, -1] for b in range(0, v.shape[1], 16)]
        return np.cumsum(np.stack(parts, 1), axis=1, dtype=F32)[:, -1]
    return np.cumsum(v if order == "forward" else v[:, ::-1], axis=1, dtype=F32)[:, -1]


def _epilogue(case, acc, order):
    inp = R.inputs(case)
    t = acc
    if inp["rs"] is not None:
        t = (t * inp["rs"][:, None]).astype(F32)
    if inp["Z"] is not None:
        t = _fma(inp["alpha"], inp["Z"], t)
    if case.op == "softmax":
        e = np.exp((t - t.max(1, keepdims=True)).astype(F32)).astype(F32)
        inv = (F32(1.0) / _vec_sum(e, order)).astype(F32)
        t = (e * inv[:, None]).astype(F32)
    elif case.op == "softmax_bwd":
        c = _vec_sum((t * inp["S"]).astype(F32), order)
        t = (inp["S"] * (t - c[:, None]).astype(F32)).astype(F32)
    if inp["ps"] is not None:
        t = (t * inp["ps"][:, None]).astype(F32)
    return t


def _ratio(got, want, bound, relative):
    err = np.abs(got.astype(np.float64) - want)
    tol = bound * np.abs(want) if relative else bound
    assert np.all(err[tol == 0] == 0.0)                       # a zero bound demands the exact zero
    return float((err[tol > 0] / tol[tol > 0]).max())


def test_bounds_hold_for_fp32_emulations_in_four_summation_orders():
    worst = {}
    for d in (1, 17, 64, 260):
        for kind in ("pattern_rs", "val_cs", "mask_cs"):
            for order in ORDERS:
                acc = _accumulate(R.Case(d, kind, "none", False, "buckets"), order)
                for op, post in (("none", False), ("z", True), ("softmax", False), ("softmax", True), ("softmax_bwd", False), ("softmax_bwd", True)):
                    case = R.Case(d, kind, op, post, "buckets")
                    want, bound, relative = R.reference(case)
                    r = _ratio(_epilogue(case, acc, order), want, bound, relative)
                    key = ("linear" if op in ("none", "z") else op, order)
                    worst[key] = max(worst.get(key, 0.0), r)
    print("worst error / bound of the fp32 emulations:", {k: round(v, 4) for k, v in sorted(worst.items())})
    assert len(worst) == 12
    for key, r in worst.items():
        assert r < 0.5, (key, r)                               # above: the bound is not sound
        assert r >= 1e-3, (key, r)                             # below: it would let anything through


def test_softmax_cases_of_the_table_cannot_underflow():
    n = 0
    for c in R.TABLE:
        if c.op == "softmax":
            want, bound, relative = R.reference(c)                # (asserts the spread of the pre-softmax row)
            assert relative and np.all(want != 0) and float(bound.max()) < 0.05
            n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_kernel_in_every_bucket():
    assert len(R.TABLE) == 822 and len(set(R.TABLE)) == len(R.TABLE)
    assert sorted(R.graph()[2][[(k * 5 + 2) % R.N_ROWS for k in range(len(R.ROW_LENGTHS))]]) == sorted(R.ROW_LENGTHS)
    assert int(R.graph()[2].max()) == 2100 and -(-2100 // R.TRIPLES["split"][2]) > 256 // 4        # a second trip of the finalize loop
    pairs, buckets, epilogues, plans = set(), set(), set(), set()
    for c in R.TABLE:
        f, v = R.family_and_variant(c)
        assert 0 <= f <= 9, c
        pairs.add((f, v))
        buckets |= {(f, v, int(b)) for b in np.unique(R.row_buckets(c.plan))}
        epilogues.add((f, v, c.op, c.post))
        plans.add((f, c.plan, c.permuted))
        # the widths sit where the issue puts them
        assert (c.width, bool(c.misaligned)) in R.FAMILY_WIDTHS[f] or c.slice_width or len(c.misaligned) == 1, c
    assert pairs == {(f, v) for f in range(10) for v in R.VARIANTS} and len(pairs) == 40
    assert buckets == {(f, v, b) for f in range(10) for v in R.VARIANTS for b in range(4)}
    assert epilogues == {(f, v, op, post) for f in range(10) for v in R.VARIANTS for op, post in R.EPILOGUES}
    assert plans == {(f, p, perm) for f in range(10) for p in R.TRIPLES for perm in (False, True)}
    for f, widths in R.FAMILY_WIDTHS.items():
        got = {(c.width, bool(c.misaligned)) for c in R.family_cases(f) if not c.slice_width and len(c.misaligned) != 1}
        assert got == set(widths), f
    # the threshold triples populate what the table's notes say
    deg = R.graph()[2]
    assert {int(b) for b in R.row_buckets("buckets")} == {0, 1, 2, 3} and {int(b) for b in R.row_buckets("split")} == {0, 3}
    assert R.row_buckets("block8")[deg == 1000][0] == 2 and R.row_buckets("block8")[deg == 2100][0] == 3
    # column slices: family 2 with 2 and 7 slices, family 8 with 2
    assert {(R.family_and_variant(c)[0], c.d // c.slice_width) for c in R.TABLE if c.slice_width} == {(2, 2), (2, 7), (8, 2)}


def test_every_alignment_trigger_resolves_to_a_scalar_family():
    for trig in R.TRIGGERS:
        cases = [c for c in R.TABLE if c.misaligned == (trig,)]
        assert len(cases) == 3, trig
        for c in cases:
            assert c.d == 64 and R.family_and_variant(c)[0] == 8, c
            assert R.family_and_variant(dataclasses.replace(c, misaligned=()))[0] == 2
    assert [R.family_of_width(w, True) for w in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, -1]
    assert [R.family_of_width(w, False) for w in (1, 16, 17, 64, 65, 256, 257)] == [7, 7, 8, 8, 9, 9, -1]


# ------------------------------------------------------------------------------------------------------------------------------------
# host refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def _problem(d, ld=None, epi=None, listed_only=False, y=FAKE):
    """(llmrec_spmm_problem_t, what it points to) over fake pointers; listed_only: an empty row list - a valid call that launches nothing"""
    ld = ld or d
    plan = ops.SpmmPlanC(64, 128, 128, 0, None, 0, None, 0, None, None, 0, None, 0, None)
    if listed_only:
        epi = ops.SpmmEpilogueC(rows_listed_only=1)
    pr = ops.SpmmProblemC(100, 2200, FAKE, FAKE, None, None, None, FAKE, ld, y, ld, d, 0, C.addressof(plan), None,
                          C.addressof(epi) if epi is not None else None)
    return pr, (plan, epi)


def _spmm(lib, pr):
    return lib.llmrec_spmm_f32(pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X, pr.ldx, pr.Y, pr.ldy,
                               pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, None)


def test_widths_outside_the_compiled_families_are_refused_before_any_launch():
    lib = _lib.load()
    for d in (257, 1028):                                      # one past the scalar and the vector families
        pr, keep = _problem(d)
        assert _spmm(lib, pr) == _lib.EUNSUPPORTED, d
        assert b"outside the compiled kernel family (vec4 = %d)" % (d % 4 == 0) in lib.llmrec_last_error()
    for d in (256, 1024):                                      # the last width of each: prepared, and an empty row list launches nothing
        pr, keep = _problem(d, ld=d + 1 if d == 256 else d, listed_only=True)
        assert _spmm(lib, pr) == 0, (d, lib.llmrec_last_error())
    # grouped launches: the vector-load families and the unmasked variants only
    two = [_problem(15, y=FAKE + 0x100000 * q) for q in range(2)]
    arr = (ops.SpmmProblemC * 2)(*[p for p, _ in two])
    assert lib.llmrec_spmm_multi_f32(2, arr, None) == _lib.EUNSUPPORTED
    assert b"grouped launches are compiled for the unmasked products with vector loads only" in lib.llmrec_last_error()
    masked = [_problem(64, epi=ops.SpmmEpilogueC(x_row_mask=FAKE, x_mask_active=R.STAMP), y=FAKE + 0x100000 * q) for q in range(2)]
    arr = (ops.SpmmProblemC * 2)(*[p for p, _ in masked])
    assert lib.llmrec_spmm_multi_f32(2, arr, None) == _lib.EUNSUPPORTED
    assert b"grouped launches are compiled for the unmasked products with vector loads only" in lib.llmrec_last_error()


def _compact(lib, d, ld, ptr):
    """llmrec_spmm_rows_compact_f32 with capacity 1; ptr(name, bytes) gives the device addresses"""
    need = lib.llmrec_spmm_rows_compact_workspace_bytes(1, d)
    return lib.llmrec_spmm_rows_compact_f32(4, 4, ptr("rowptr", 20), ptr("colidx", 16), None, ptr("X", 4 * ld * 4), ld, d, ptr("list", 4),
                                            ptr("n", 4), 1, ptr("out", ld * 4), ld, ptr("ws", need), need, None)


def test_rows_compact_outside_its_families_is_refused_before_any_launch():
    lib = _lib.load()
    fake = lambda name, nbytes: FAKE
    assert _compact(lib, 65, 65, fake) == _lib.EUNSUPPORTED and b"spmm_rows_compact: d = 65" in lib.llmrec_last_error()
    assert _compact(lib, 260, 260, fake) == _lib.EUNSUPPORTED and b"spmm_rows_compact: d = 260" in lib.llmrec_last_error()
    # The last compiled widths (64 scalar, 256 float4) pass every argument check. llmrec_spmm_rows_compact_f32 has no prepare-only
    # path: a call that passes its checks goes on to launch, and a launch must never see fake pointers on a machine that has a device.
    # So the proof of "prepared" is the status of the launch itself: without a device the launch fails in the HIP runtime (LLMREC_EHIP,
    # set only behind the last check); with one, the call gets real zeroed buffers and an empty list, runs, and writes one slot of zeros.
    # Either way the status is none of the refusals (LLMREC_EINVAL, LLMREC_EWORKSPACE, LLMREC_EUNSUPPORTED).
    have_device = torch.cuda.is_available()
    keep = {}

    def real(name, nbytes):
        keep[name] = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
        return keep[name].data_ptr()
    for d, ld in ((64, 65), (256, 256)):
        rc = _compact(lib, d, ld, real if have_device else fake)
        if have_device:
            torch.cuda.synchronize()
        assert rc == (0 if have_device else EHIP), (d, rc, lib.llmrec_last_error())
