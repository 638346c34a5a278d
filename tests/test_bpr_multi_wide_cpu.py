"""The eight-problem wide loss segment (llmrec_bpr_scatter_plan_wide, llmrec_bpr_multi_{scores,select_bwd,losses}_wide_f32) without a
GPU: the declarations, the workspace queries (host arithmetic), the refusals (decided before anything is launched: fake pointers), the
capped entry points' unchanged refusals, the trainer's routing predicate against a hand-written table and the plan's numpy restatement
against tests/_bpr_ref.py's notion of the plan (the sorted (id, slot) pairs its emulation walks)."""
import ctypes

import numpy as np
import pytest

from llmrec_amd import _lib, step_options
from tests import _plan_ref as P

FAKE = 0x1000                                                             # a non-null pointer that is never dereferenced: nothing is launched
CAP, WIDE = _lib.CONST["LLMREC_BPR_MAX_B"], _lib.CONST["LLMREC_BPR_WIDE_MAX_B"]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, _lib.EUNSUPPORTED
NEW = ("llmrec_bpr_scatter_plan_wide", "llmrec_bpr_multi_scores_wide_f32", "llmrec_bpr_multi_select_bwd_wide_f32",
       "llmrec_bpr_multi_losses_wide_f32")
QUERIES = ("llmrec_bpr_scatter_plan_wide_workspace_bytes", "llmrec_bpr_multi_wide_workspace_bytes")
SIZES = [0, 1, 4097, 12400, 1 << 16, 1 << 20, WIDE]


def test_header_declares_and_the_library_exports_the_wide_entry_points():
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in NEW + QUERIES:
        assert name in protos and hasattr(lib, name), name
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8 and lib.llmrec_abi_version() == 8
    assert (CAP, WIDE) == (4096, 1 << 22)
    # the twins take their capped forms' arguments (+ the workspace)
    assert protos["llmrec_bpr_multi_scores_wide_f32"][2] == protos["llmrec_bpr_multi_scores_step_f32"][2]
    assert protos["llmrec_bpr_multi_losses_wide_f32"][2] == protos["llmrec_bpr_multi_losses_assemble_f32"][2]
    a, b = protos["llmrec_bpr_multi_select_bwd_wide_f32"][2], protos["llmrec_bpr_multi_select_bwd_f32"][2]
    assert a == b[:-1] + ["workspace", "workspace_bytes", "stream"]
    a, b = protos["llmrec_bpr_scatter_plan_wide"][2], protos["llmrec_bpr_scatter_plan"][2]
    assert a == b[:-1] + ["workspace", "workspace_bytes", "stream"]


def test_workspace_queries_are_host_arithmetic():
    plan = lambda n: _lib.query("llmrec_bpr_scatter_plan_wide_workspace_bytes", n)
    for q in (plan, lambda n: _lib.query("llmrec_bpr_multi_wide_workspace_bytes", 8, n), lambda n: _lib.query("llmrec_bpr_multi_wide_workspace_bytes", 1, n)):
        got = [q(n) for n in SIZES]
        assert all(g > 0 for g in got)
        assert got == sorted(got) and got[-1] > got[0]
        assert q(-1) == -1 and q(WIDE + 1) == -1
    multi = lambda p, n: _lib.query("llmrec_bpr_multi_wide_workspace_bytes", p, n)
    assert multi(0, 5000) == -1 and multi(9, 5000) == -1
    assert multi(8, 5000) == 8 * multi(1, 5000)                           # a block of its own per problem
    assert multi(1, 5000) >= _lib.query("llmrec_bpr_prune_wide_workspace_bytes", 5000)


def _table(n=8, **bad):
    arr = (_lib.STRUCT["llmrec_bpr_problem_t"] * max(n, 1))()
    for i in range(max(n, 1)):
        arr[i].Eu, arr[i].ldu, arr[i].Ei, arr[i].ldi = FAKE, 64, FAKE, 64
        arr[i].dEu, arr[i].lddu, arr[i].dEi, arr[i].lddi = FAKE, 64, FAKE, 64
        arr[i].g_mf, arr[i].g_emb = 1.0, 1.0
    for k, v in bad.items():
        setattr(arr[max(n, 1) - 1], k, v)
    return arr


def _plan(lib, B=5000, ws=FAKE, ws_bytes=None):
    need = _lib.query("llmrec_bpr_scatter_plan_wide_workspace_bytes", min(B, WIDE))
    return lib.llmrec_bpr_scatter_plan_wide(FAKE, FAKE, FAKE, B, None, FAKE, ws, need if ws_bytes is None else ws_bytes, None)


def _scores(lib, n=8, table=None, B=5000):
    return lib.llmrec_bpr_multi_scores_wide_f32(n, table if table is not None else _table(n), 64, FAKE, FAKE, FAKE, B, None, FAKE, None, None,
                                                0.0, 0.0, 0.0, None)


def _select(lib, n=8, table=None, B=5000, ws=FAKE, ws_bytes=None):
    need = _lib.query("llmrec_bpr_multi_wide_workspace_bytes", min(max(n, 1), 8), min(B, WIDE))
    return lib.llmrec_bpr_multi_select_bwd_wide_f32(n, table if table is not None else _table(n), 64, FAKE, FAKE, FAKE, B, None, 0.29, 1e-5, 64.0,
                                                    FAKE, None, None, None, FAKE, ws, need if ws_bytes is None else ws_bytes, None)


def _losses(lib, n=8, B=5000, scal=FAKE):
    w = (ctypes.c_float * 8)(*([1.0] * 8))
    return lib.llmrec_bpr_multi_losses_wide_f32(n, B, None, 0.29, 1e-5, 64.0, FAKE, FAKE, w, None, 0, 0.0, scal, None, None)


def test_wide_entries_refuse_before_they_launch():
    lib = _lib.load()
    need_p = _lib.query("llmrec_bpr_scatter_plan_wide_workspace_bytes", 5000)
    need_s = _lib.query("llmrec_bpr_multi_wide_workspace_bytes", 8, 5000)
    cases = [
        ("plan: short workspace", lambda: _plan(lib, ws_bytes=need_p - 1), EWORKSPACE, b"bpr_scatter_plan_wide"),
        ("plan: no workspace", lambda: _plan(lib, ws=None), EWORKSPACE, b"bpr_scatter_plan_wide"),
        ("plan: above the cap", lambda: _plan(lib, B=WIDE + 1), EUNSUPPORTED, b"bpr_scatter_plan_wide"),
        ("plan: negative", lambda: _plan(lib, B=-1), EINVAL, b"bpr_scatter_plan_wide"),
        ("scores: above the cap", lambda: _scores(lib, B=WIDE + 1), EUNSUPPORTED, b"bpr_multi_scores_wide"),
        ("scores: nine problems", lambda: _scores(lib, n=9, table=_table(9)), EINVAL, b"bpr_multi_scores_wide"),
        ("scores: no problems", lambda: _scores(lib, n=0), EINVAL, b"bpr_multi_scores_wide"),
        ("scores: ld < d", lambda: _scores(lib, table=_table(8, ldi=63)), EINVAL, b"bpr_multi_scores_wide"),
        ("scores: null table", lambda: _scores(lib, table=_table(8, Eu=None)), EINVAL, b"bpr_multi_scores_wide"),
        ("select: short workspace", lambda: _select(lib, ws_bytes=need_s - 1), EWORKSPACE, b"bpr_multi_select_bwd_wide"),
        ("select: the workspace of one problem", lambda: _select(lib, ws_bytes=need_s // 8), EWORKSPACE, b"bpr_multi_select_bwd_wide"),
        ("select: no workspace", lambda: _select(lib, ws=None), EWORKSPACE, b"bpr_multi_select_bwd_wide"),
        ("select: above the cap", lambda: _select(lib, B=WIDE + 1), EUNSUPPORTED, b"bpr_multi_select_bwd_wide"),
        ("select: nine problems", lambda: _select(lib, n=9, table=_table(9)), EINVAL, b"bpr_multi_select_bwd_wide"),
        ("select: no gradient target", lambda: _select(lib, table=_table(8, dEi=None)), EINVAL, b"bpr_multi_select_bwd_wide"),
        ("select: ldd < d", lambda: _select(lib, table=_table(8, lddu=63)), EINVAL, b"bpr_multi_select_bwd_wide"),
        ("losses: above the cap", lambda: _losses(lib, B=WIDE + 1), EUNSUPPORTED, b"bpr_multi_losses_wide"),
        ("losses: nine problems", lambda: _losses(lib, n=9), EINVAL, b"bpr_multi_losses_wide"),
        ("losses: no problems", lambda: _losses(lib, n=0), EINVAL, b"bpr_multi_losses_wide"),
    ]
    for what, call, status, text in cases:
        assert call() == status, what
        assert text in lib.llmrec_last_error(), (what, lib.llmrec_last_error())
    # an empty capacity: nothing launched, as the capped twins
    assert _plan(lib, B=0) == 0 and lib.llmrec_bpr_scatter_plan(FAKE, FAKE, FAKE, 0, None, FAKE, None) == 0
    assert _select(lib, B=0) == 0
    assert lib.llmrec_bpr_multi_select_bwd_f32(8, _table(8), 64, FAKE, FAKE, FAKE, 0, None, 0.29, 1e-5, 64.0, FAKE, None, None, None, FAKE, None) == 0
    assert _scores(lib, B=0) == EINVAL                                   # (the launch carries the step's counters: the capped twin's answer)
    assert lib.llmrec_bpr_multi_scores_step_f32(8, _table(8), 64, FAKE, FAKE, FAKE, 0, None, FAKE, None, None, 0.0, 0.0, 0.0, None) == EINVAL


def test_the_capped_entry_points_still_refuse_4097():
    lib = _lib.load()
    t, w = _table(8), (ctypes.c_float * 8)(*([1.0] * 8))
    B = CAP + 1
    calls = {
        b"bpr_scatter_plan: B_max 4097 > 4096": lambda: lib.llmrec_bpr_scatter_plan(FAKE, FAKE, FAKE, B, None, FAKE, None),
        b"bpr_scatter_plan_reach_mark: B_max 4097 > 4096": lambda: lib.llmrec_bpr_scatter_plan_reach_mark(FAKE, FAKE, FAKE, B, None, FAKE, 100, 100,
                                                                                                         FAKE, FAKE, FAKE, None),
        b"bpr_multi_scores: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_scores_f32(8, t, 64, FAKE, FAKE, FAKE, B, None, FAKE, None, None),
        b"bpr_multi_scores_step: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_scores_step_f32(8, t, 64, FAKE, FAKE, FAKE, B, None, FAKE, None,
                                                                                                 None, 0.0, 0.0, 0.0, None),
        b"bpr_multi_select_bwd: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_select_bwd_f32(8, t, 64, FAKE, FAKE, FAKE, B, None, 0.29, 1e-5,
                                                                                               64.0, FAKE, None, None, None, FAKE, None),
        b"bpr_multi_losses: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_losses_f32(8, B, None, 0.29, 1e-5, 64.0, FAKE, FAKE, None),
        b"bpr_multi_losses_assemble: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_losses_assemble_f32(8, B, None, 0.29, 1e-5, 64.0, FAKE, FAKE, w,
                                                                                                         None, 0, 0.0, FAKE, None, None),
        b"bpr_multi_fwd: B_max 4097 > 4096": lambda: lib.llmrec_bpr_multi_fwd_f32(8, t, 64, FAKE, FAKE, FAKE, B, None, 0.29, 1e-5, 64.0, FAKE, FAKE,
                                                                                 None),
    }
    for text, call in calls.items():
        assert call() == EUNSUPPORTED, text
        assert text in lib.llmrec_last_error(), (text, lib.llmrec_last_error())


# the routing predicate: (LLMREC_FUSED, b_max) -> the path of a trainer whose other conditions hold
ROUTES = {
    (None, 4096): "fused", (None, 4097): "modular", (None, 1 << 22): "modular", (None, (1 << 22) + 1): "modular",
    ("1", 4096): "fused", ("1", 4097): "modular", ("1", 1 << 22): "modular", ("1", (1 << 22) + 1): "modular",
    ("wide", 4096): "fused", ("wide", 4097): "fused_wide", ("wide", 1 << 22): "fused_wide", ("wide", (1 << 22) + 1): "modular",
    ("0", 4096): "modular", ("0", 4097): "modular", ("0", 1 << 22): "modular", ("0", (1 << 22) + 1): "modular",
}
# (mask, mask_rate, drop_rate, LLMREC_FUSED_DROPOUT) -> do the trainer's other conditions hold?
CONDITIONS = {
    (False, 0.0, 0.0, None): True, (False, 0.0, 0.0, "1"): True, (False, 0.0, 0.0, "0"): True,
    (True, 0.0, 0.0, None): False, (True, 0.0, 0.0, "1"): False,
    (False, 0.2, 0.0, None): False, (False, 0.2, 0.0, "1"): False, (True, 0.2, 0.0, None): False,
    (False, 0.0, 0.1, None): False, (False, 0.0, 0.1, "0"): False, (False, 0.0, 0.1, "1"): True,
    (True, 0.0, 0.1, "1"): False, (False, 0.2, 0.1, "1"): False,
}


def test_routing_table():
    assert len(ROUTES) == 16 and len(CONDITIONS) == 13
    for (fused, b_max), want in ROUTES.items():
        for (mask, mask_rate, drop_rate, fd), holds in CONDITIONS.items():
            got = step_options.route(fused, fd, mask=mask, mask_rate=mask_rate, drop_rate=drop_rate, b_max=b_max, cap=CAP, wide_cap=WIDE)
            assert got == (want if holds else "modular"), (fused, b_max, mask, mask_rate, drop_rate, fd, got)
    # any other value of the variable is the per-op path, as before "wide" existed
    for other in ("", "2", "WIDE", "true"):
        assert step_options.route(other, None, mask=False, mask_rate=0.0, drop_rate=0.0, b_max=1024, cap=CAP, wide_cap=WIDE) == "modular"
    assert "LLMREC_FUSED" in step_options.TRAINER_SWITCHES and len(step_options.ENV_SWITCHES + step_options.TRAINER_SWITCHES) == 13


def test_plan_restatement_is_the_reference_emulations_plan():
    """tests/_bpr_ref.py's emulation walks  sorted((id, slot))  grouped by id, the item side's negatives at slot B_max + b: the restated
    plan's runs are those lists, its keys ascend per side, the unused slots come last and carry no run."""
    rng = np.random.default_rng(40)
    B, n = 40, 33
    users, pos, neg = rng.integers(0, 6, B), rng.integers(0, 9, B), rng.integers(0, 9, B)
    neg[3] = pos[3]                                                       # one item on both sides of a sample
    words, runlen = P.plan(users, pos, neg, B, n)
    keys, runlen2 = P.split(np.concatenate([words, runlen.view(np.int64), np.zeros(B // 2, dtype=np.int64)]), B)
    assert np.array_equal(keys, words) and np.array_equal(runlen, runlen2)
    got = P.runs(keys, runlen, B)
    for side, pairs in (("u", [(int(users[b]), b) for b in range(n)]),
                        ("i", [(int(pos[b]), b) for b in range(n)] + [(int(neg[b]), B + b) for b in range(n)])):
        want = {}
        for id_, slot in sorted(pairs):
            want.setdefault(id_, []).append(slot)
        assert got[side] == want, side
        assert max(len(v) for v in want.values()) > 3                    # duplicates: runs longer than one
    ku, ki = keys[:B].view(np.uint64), keys[B:].view(np.uint64)
    assert np.all(ku[1:] > ku[:-1]) and np.all(ki[1:] > ki[:-1])
    assert np.all(ku[n:] >> np.uint64(32) == P.NO_ID) and np.all(ki[2 * n:] >> np.uint64(32) == P.NO_ID)
    assert not runlen[n:B].any() and not runlen[B + 2 * n:].any()
    assert int(runlen[:B].sum()) == n and int(runlen[B:].sum()) == 2 * n
    # n_valid is clamped as the kernels clamp it
    assert np.array_equal(P.plan(users, pos, neg, B, 50)[0], P.plan(users, pos, neg, B, None)[0])
    assert not P.plan(users, pos, neg, B, -3)[1].any()


def test_fused_step_takes_the_wide_route_above_the_capped_entry_points_limit():
    from llmrec_amd import dp, fused
    assert fused.FusedStep.WIDE_FROM == CAP
    with pytest.raises(RuntimeError, match="LLMREC_BPR_MAX_B = 4096"):    # the replicas' step names the cap before it allocates anything
        dp.DataParallelStep(None, None, None, None, None, CAP + 1)
