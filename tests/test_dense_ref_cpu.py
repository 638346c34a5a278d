"""The yardstick of tests/test_gpu_dense_families.py, checked without a device (tests/_dense_ref.py): the case table reaches every
instantiation the host of llmrec_amd/csrc/dense.hip can launch, the restated slab and fast-path rules agree with the library's own workspace
queries, split3 is exact, the thresholds are sound (emulations stay below them) and not vacuous (emulations are not far below, and CPU
mutants of the emulation - a lost term, swapped terms, a duplicated tile row, a doubled bias - exceed them), and the closed-rounding fma
chain agrees with oracle.scores_fma_chain."""
import ctypes

import numpy as np
import pytest

from tests import _dense_ref as R


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def _reached():
    fwd_plain = {c.expect for c in R.plain_cases()}
    fwd_grouped = {R.grouped_expect(c, pr) for c in R.grouped_cases() for pr in ("f32", "bf16x3")}
    wgrad, reduce_ = set(), set()
    for c in R.wgrad_cases():
        plan = R.wgrad_grouped(R.wg_problems(c), c.N, c.K, c.kind, c.db, c.accumulate)
        wgrad |= plan["kernels"] - {"memset"}
        reduce_ |= plan["reduce"]
    for c in R.multi_cases():
        plan = R.wgrad_multi(R.multi_targets(c), c.N, c.budget)
        wgrad |= plan["kernels"]
        reduce_ |= plan["reduce"]
    for c in R.adamw_cases():
        plan = R.wgrad_multi(R.multi_targets(c), c.N, c.budget)
        wgrad |= plan["kernels"]
        reduce_ |= {r.replace("<false>", "<true>") for r in plan["reduce"]}
    return fwd_plain, fwd_grouped, wgrad, reduce_


def test_the_table_reaches_every_instantiation(capsys):
    fwd_plain, fwd_grouped, wgrad, reduce_ = _reached()
    with capsys.disabled():
        for title, got in (("linear_fwd_kernel<NT, RT, SPLITK>", fwd_plain), ("grouped forward <NT, RT, MODE>", fwd_grouped),
                           ("weight gradient", wgrad), ("reduction / accumulate / bias gradient", reduce_)):
            print("\n[dense table] %s: %d reached\n    %s" % (title, len(got), "\n    ".join(str(g) for g in sorted(got, key=str))))
    assert fwd_plain == R.ALL_FWD_PLAIN and len(fwd_plain) == 16
    assert fwd_grouped == R.ALL_FWD_GROUPED and len(fwd_grouped) == 24 + 24
    assert wgrad == R.ALL_WGRAD
    assert reduce_ == R.ALL_REDUCE


def test_the_table_holds_the_cases_the_kernels_can_go_wrong_at():
    plain = R.plain_cases()
    sk = [c for c in plain if c.expect[3]]
    assert {c.N for c in sk} == {1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128}
    for K in (1, 16, 17, 64, 65, 100):
        assert sum(c.K == K for c in sk) >= 2, K
    for M in (1, 15, 16, 17, 33):
        assert sum(c.M == M for c in sk) >= 2, M
    rows = [c for c in plain if not c.expect[3]]
    assert {c.expect[1] for c in rows if c.M == 65573 and c.N % 16 and c.K in (20, 21)} == set(range(1, 9))
    assert any((c.M, c.N, c.K) == (65536, 64, 4) for c in rows)
    g = R.grouped_cases()
    assert {c.N for c in g} == set(R.GROUPED_N)
    for c in g:
        assert {0, 1, 63, 64, 65, 129, 300} <= {j.M for j in c.jobs} and len(c.jobs) <= R.MAX_PROBLEMS
        assert (R.FILLER_M in {j.M for j in c.jobs}) == (c.rt == 2)
        assert {"none", "bias", "scale"} == {j.bias for j in c.jobs} and {True, False} == {j.y_slice for j in c.jobs}
    assert {j.K for c in g if c.mode == 1 for j in c.jobs if j.M != R.FILLER_M} == {4, 36, 100}
    assert {j.K for c in g if c.mode == 2 for j in c.jobs} == {32, 96, 128}
    for kernel_class, classes in (("plain", {c.cls for c in plain}), ("grouped", {j.cls for c in g for j in c.jobs}),
                                  ("f32 gradient", {c.cls for c in R.wgrad_cases() if c.kind == "f32"}),
                                  ("bf16x3 gradient", {c.cls for c in R.wgrad_cases() if c.expect == "linear_wgrad_bf16x3_kernel"}),
                                  ("multi", {c.cls for c in R.multi_cases()})):
        assert classes == set(R.VALUE_CLASSES), (kernel_class, classes)
    w = R.wgrad_cases()
    assert {M for c in w if c.kind == "f32" for M in c.Ms} >= {0, 1, 47, 48, 49, 143, 144, 145, 433}
    assert {M for c in w if c.expect == "linear_wgrad_bf16x3_kernel" for M in c.Ms} >= {1, 31, 32, 33, 63, 64, 65, 97, 300}
    assert {(c.N, c.K) for c in w if c.expect == "linear_wgrad_bf16x3_kernel"} >= {(64, 64), (64, 192), (128, 64), (128, 128)}
    m = R.multi_cases()
    assert {len(c.targets) for c in m if c.version == 1} >= {2, 4} and all(any(t.K == 192 for t in c.targets) for c in m if c.version == 1)
    assert {t.K for c in m if c.version == 2 for t in c.targets} == {128, 256, 384}
    assert {c.budget for c in m if c.version == 1} == {0, 1, 7} == {c.budget for c in m if c.version == 2}
    assert {c.N for c in m if c.version == 1} == {64, 128} == {c.N for c in m if c.version == 2}
    assert {p.M for c in m for t in c.targets for p in t.problems} == {1, 15, 16, 17, 33, 517}
    lists = [p for c in m for t in c.targets for p in t.problems if p.n_list is not None]
    assert {p.n_list for p in lists} >= {0, 1, 15, 16, 17, 33, 517}
    assert any(p.hint == 0 for p in lists) and any(0 < p.hint < p.n_list for p in lists) and any(p.hint > p.M for p in lists)


# ------------------------------------------------------------------------------------------------------------------------------------
# the restated rules against the library's host arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _c_targets(targets, N, budget=0):
    from llmrec_amd import ops
    arr = (ops.WgradTarget * max(len(targets), 1))()
    arr[0].block_budget = budget
    keep = []
    for i, t in enumerate(targets[:len(arr)]):
        probs = (ops.WgradProblem * max(len(t.problems), 1))()
        for j, q in enumerate(t.problems[:len(probs)]):
            probs[j].dY, probs[j].lddy, probs[j].X, probs[j].ldx, probs[j].M = 0x10000 + q.ymod, q.lddy, 0x20000 + q.xmod, q.ldx, q.M
            probs[j].db_row_weight = 0x30000 if q.weighted else None
            if q.listed:
                probs[j].row_list, probs[j].n_rows, probs[j].rows_expected = 0x40000 + q.list_mod64, (0x50000 if q.has_n_rows else None), q.rows_expected
        keep.append(probs)
        arr[i].n_problems, arr[i].problems, arr[i].K = len(t.problems), ctypes.cast(probs, ctypes.c_void_p), t.K
        arr[i].dW, arr[i].lddw, arr[i].db, arr[i].accumulate = 0x60000, t.lddw, (0x70000 if t.db else None), int(t.accumulate)
    return arr, keep


def test_restated_slab_rules_give_the_library_workspace_sizes():
    from llmrec_amd import _lib
    for c in R.wgrad_cases():
        Mt = sum(c.Ms)
        assert _lib.query("llmrec_linear_wgrad_workspace_bytes", Mt, c.N, c.K) == R.wgrad_workspace_bytes(Mt, c.N, c.K), c.name
        plan = R.wgrad_grouped(R.wg_problems(c), c.N, c.K, c.kind, c.db, c.accumulate)
        assert plan["bytes"] <= plan["bound"], (c.name, plan)          # what the launch will ask of the buffer the query sized
        if c.expect.startswith("linear_wgrad_bf16x3_v2"):               # the hand-over: the library's own figure for the one-target launch
            arr, keep = _c_targets((R.WgT(c.K, c.K, tuple(R.wg_problems(c)), c.db, c.accumulate),), c.N)
            assert _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", 1, arr, c.N) == plan["bytes"]
    for M, N, K in ((0, 64, 64), (1, 1, 1), (17366, 64, 1536), (10 ** 6, 128, 4096), (143, 65, 65)):
        assert _lib.query("llmrec_linear_wgrad_workspace_bytes", M, N, K) == R.wgrad_workspace_bytes(M, N, K)
    assert _lib.query("llmrec_linear_wgrad_workspace_bytes", -1, 64, 64) == R.wgrad_workspace_bytes(-1, 64, 64) == -1
    for c in R.multi_cases() + R.adamw_cases():
        ts = R.multi_targets(c)
        arr, keep = _c_targets(ts, c.N, c.budget)
        plan = R.wgrad_multi(ts, c.N, c.budget)
        assert _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", len(ts), arr, c.N) == plan["bytes"] == R.wgrad_multi_workspace_bytes(ts, c.N, c.budget), c.name
        assert plan["MC"] % 32 == 0 and plan["MC"] >= 64


def test_every_refusal_clause_of_the_multi_launch_answers_minus_one():
    from llmrec_amd import _lib
    ok = R.WgP(33, 64, 128)
    T = lambda K=128, lddw=None, probs=(ok,): R.WgT(K, K if lddw is None else lddw, tuple(probs))
    cases = {
        "n_targets": ((T(),) * 5, 64), "N % 64": ((T(),), 96), "n_problems": ((T(probs=(ok,) * 9),), 64), "K % 64": ((T(K=100),), 64),
        "lddw < K": ((T(lddw=64),), 64), "M <= 0": ((T(probs=(ok, R.WgP(0, 64, 128))),), 64),
        "ld too small": ((T(probs=(R.WgP(33, 60, 128),)),), 64), "alignment": ((T(probs=(R.WgP(33, 64, 128, 4, 0),)),), 64),
        "offsets": ((T(probs=(R.WgP((1 << 23) - 256, 64, 128),)),), 64),
        "list without n_rows": ((T(probs=(R.WgP(33, 64, 128, listed=True, has_n_rows=False),)),), 64),
        "list with K % 128": ((T(K=192, probs=(R.WgP(33, 64, 192, listed=True),)),), 64),
        "list offsets": ((T(probs=(R.WgP(1 << 22, 64, 128, listed=True),)),), 64),
        "list alignment": ((T(probs=(R.WgP(33, 64, 128, listed=True, list_mod64=4),)),), 64),
    }
    seen = set()
    for clause, (ts, N) in cases.items():
        assert R.wgrad_multi_ok(ts, N) == clause, (clause, R.wgrad_multi_ok(ts, N))
        arr, keep = _c_targets(ts, N)
        assert _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", len(ts), arr, N) == -1 == R.wgrad_multi_workspace_bytes(ts, N), clause
        seen.add(clause)
    assert len(seen) == 13
    arr, keep = _c_targets((T(),), 64)                                    # the same argument block inside the fast path
    assert _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", 1, arr, 64) == R.wgrad_multi_workspace_bytes((T(),), 64) > 0
    # near the limits: just inside
    assert R.wgrad_multi_ok((T(probs=(R.WgP((1 << 23) - 257, 64, 128),)),), 64) is None
    arr, keep = _c_targets((T(probs=(R.WgP((1 << 23) - 257, 64, 128),)),), 64)
    assert _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", 1, arr, 64) > 0


def test_dispatch_spot_values():
    assert R.fwd_plain(65535, 64, 64) == ("linear_fwd_kernel", 4, 1, True) and R.fwd_plain(65536, 65, 64) == ("linear_fwd_kernel", 5, 1, False)
    assert R.fwd_plain(1, 129, 4) is None and R.fwd_grouped([R.FwdP(4, 4, 4, 4)], 65, "f32") is None
    a = R.FwdP(300, 32, 32, 32)
    assert R.fwd_grouped([a], 64, "bf16x3")[1:] == (4, 1, 3) and R.fwd_grouped([a], 64, "f32")[1:] == (4, 1, 2)
    assert R.fwd_grouped([a, R.FwdP(0, 36, 36, 36)], 64, "bf16x3")[3] == 1             # an EMPTY problem's K still turns the launch
    assert R.fwd_grouped([a, R.FwdP(1, 36, 37, 36)], 64, "bf16x3")[3] == 0
    assert R.fwd_grouped([a, R.FwdP(252 * 128, 32, 32, 32)], 64, "f32")[2] == 1 and R.fwd_grouped([a, R.FwdP(252 * 128 + 1, 32, 32, 32)], 64, "f32")[2] == 2
    assert R.fwd_grouped([R.FwdP(1 << 24, 64, 64, 64)], 64, "bf16x3")[3] == 1          # the 2^30 limit of the scalar-k addressing
    assert R.wgrad_slab_rows(1, 64, False) == 144 and R.wgrad_slab_rows(10 ** 6, 64, False) == 528 and R.wgrad_slab_rows(10 ** 6, 64, True) == 512
    assert R.wgrad_rows_eff(R.WgP(517, 64, 128, listed=True, rows_expected=1)) == 16 and R.wgrad_rows_eff(R.WgP(517, 64, 128, listed=True, rows_expected=10 ** 6)) == 517
    assert R.wgrad_rows_eff(R.WgP(517, 64, 128, listed=False, rows_expected=5)) == 517


# ------------------------------------------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def test_fma32_rounds_once():
    a, b, c = np.float32(8 * (1 + 2.0 ** -23)), np.float32(8 * (1 - 2.0 ** -23)), np.float32(2.0 ** 30 + 2.0 ** 7)
    # a b = 64 - 2^-40: c + a b lies just below the midpoint of c and c + 2^7; fp64 rounds the sum ONTO the midpoint, and the tie then goes to even
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 30 + 2.0 ** 8)
    assert R.fma32(np.array([a]), np.array([b]), np.array([c]))[0] == c
    assert R.fma32(np.array([a]), np.array([-b]), np.array([-c]))[0] == -c
    a2 = np.float32(8 * (1 + 2.0 ** -23))
    assert R.fma32(np.array([a2]), np.array([a2]), np.array([c]))[0] == np.float32(2.0 ** 30 + 2.0 ** 8)       # just above the midpoint
    from fractions import Fraction
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((3, 4000)) * 2.0 ** rng.integers(-12, 12, (3, 4000))).astype(np.float32)
    x[2, :2000] = (-(x[0, :2000].astype(np.float64) * x[1, :2000].astype(np.float64))).astype(np.float32)      # heavy cancellation
    got = R.fma32(x[0], x[1], x[2])
    for i in range(0, 4000, 7):
        exact = Fraction(float(x[0, i])) * Fraction(float(x[1, i])) + Fraction(float(x[2, i]))
        g = Fraction(float(got[i]))
        for nb in (np.nextafter(got[i], np.float32(np.inf)), np.nextafter(got[i], np.float32(-np.inf))):
            assert abs(exact - g) <= abs(exact - Fraction(float(nb)))


def test_closed_rounding_chain_agrees_with_the_oracle_chain():
    from oracle.oracle import scores_fma_chain
    rng = np.random.default_rng(11)
    for d in (1, 5, 16, 20, 33, 64, 100, 128):                    # the widths of the evaluation tests
        eu, ei = rng.standard_normal((43, d)).astype(np.float32), rng.standard_normal((70, d)).astype(np.float32)
        want = scores_fma_chain(eu, ei, order="mfma16x16x4")
        assert np.array_equal(R.chain(eu, ei).view(np.int32), want.view(np.int32)), d
        assert R.chain_order(0, d) == [k for c in range((d + 15) // 16) for s in range(4) for q in range(4) for k in (16 * c + 4 * q + s,) if k < d]
    X, W = R.values("gauss", (5, 65), "sk", "X"), R.values("gauss", (7, 65), "sk", "W")
    b = R.values("gauss", (7,), "sk", "b")
    parts = [R.chain(X, W, lo, hi) for lo, hi in ((0, 32), (32, 64), (64, 65), (96, 65))]        # kq = 32: the fourth wave's range is empty
    assert np.array_equal(R.chain_fwd(X, W, b, splitk=True), (((parts[0] + parts[1]) + parts[2]) + parts[3]) + b[None, :])
    assert not parts[3].any() and np.abs(R.chain_fwd(X, W, b, splitk=True) - R.y64(X, W, b)).max() < 1e-4


def test_split3_is_exact_and_bounded():
    for cls in R.VALUE_CLASSES:
        x = R.values(cls, (301, 40), "split")
        h, m, l = R.split3(x)
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64)), cls
        r2 = (x - h) - m
        assert np.array_equal(l.view(np.uint32), r2.view(np.uint32)), cls              # cutting r2 to its high half loses nothing
        for t in (h, m, l):
            assert not (t.view(np.uint32) & np.uint32(0xffff)).any()                   # a bf16 value: <= 8 significant bits
        ax = np.abs(x.astype(np.float64))
        assert (np.abs(h) <= ax).all() and (np.abs(m) <= 2.0 ** -7 * ax).all() and (np.abs(l) <= 2.0 ** -14 * ax).all(), cls
        nz = ax > 0
        assert (np.abs(m)[nz] < 2.0 ** -7 * ax[nz]).all() and (np.abs(l)[nz] < 2.0 ** -14 * ax[nz]).all()
        if cls == "low16clear":
            assert not m.any() and not l.any()
        if cls == "full24":
            assert (np.abs(m) > 2.0 ** -9 * ax).all() and (np.abs(l) > 2.0 ** -17 * ax).all()
        assert np.array_equal(np.signbit(h), np.signbit(x))                            # -0.0 keeps its sign in h


# ------------------------------------------------------------------------------------------------------------------------------------
# thresholds: sound and not vacuous
# ------------------------------------------------------------------------------------------------------------------------------------
def _f32_sum(dY, X, order):
    """dW by one fp32 fma per row, rows in the given order"""
    acc = np.zeros((dY.shape[1], X.shape[1]), dtype=np.float32)
    for r in order:
        acc = R.fma32(dY[r][:, None], X[r][None, :], acc)
    return acc


@pytest.mark.parametrize("cls", ["gauss", "positive", "scaled", "negzero"])
def test_fp32_gradient_bound_is_sound_and_not_vacuous(cls):
    """fp32 emulations of the gradient (one fma per row, ascending / descending / slab-wise as the kernel sums) stay between 1e-3 and 0.5
    of (n + 6) u S in the worst element. (Value classes whose products can be exact in fp32 - low 16 bits clear, all bits set - are not used here.)"""
    for M in (1, 49, 433):
        dY, X = R.values(cls, (M, 16), "f32b", M, "dY", scale=2.0 ** -6), R.values(cls, (M, 24), "f32b", M, "X")
        want, S = R.dw64([(dY, X)]), R.s_dw([(dY, X)])
        slabs = [_f32_sum(dY, X, range(lo, min(M, lo + 144))) for lo in range(0, M, 144)]
        slabbed = slabs[0]
        for s in slabs[1:]:
            slabbed = slabbed + s
        for got in (_f32_sum(dY, X, range(M)), _f32_sum(dY, X, range(M - 1, -1, -1)), slabbed):
            assert (np.abs(got - want) <= R.bound_f32(M) * S).all()
            ratio = (np.abs(got - want) / (R.bound_f32(M) * np.where(S == 0, 1, S))).max()
            assert 1e-3 <= ratio <= 0.5, (cls, M, ratio)


def test_bf16x3_thresholds_hold_for_the_per_product_emulation():
    worst = {}
    for case in R.precision_cases():
        six, full, S = R.precision_reference(case)
        assert (np.abs(six - full) <= R.DROPPED * S).all(), case[1]
        for order in range(4):
            e = R.emulate(case[2], case[3], order=order, add=case[4])
            err = np.abs(e - six)
            assert (err <= R.T_ACC[case[0]] / 4 * S).all(), (case[1], order)               # by construction: T_ACC = 4 x this worst value
            assert (np.abs(e - full) <= (R.DROPPED + R.T_ACC[case[0]]) * S).all()
            worst[case[0]] = max(worst.get(case[0], 0.0), float((err / np.where(S == 0, 1, S)).max()))
    for k, v in worst.items():                                                            # ... and no looser than that: within 2 % of it
        assert 0.98 * R.T_ACC[k] / 4 <= v <= R.T_ACC[k] / 4, (k, v)
        print("[dense T_ACC] %s: worst |emulation - Y6| / S = %.4g, T_ACC = %.4g" % (k, v, R.T_ACC[k]))


def test_dropped_terms_come_within_a_factor_three_of_their_bound():
    """x = 1.0000000 1111111 1 1111111 1 (binary) x 2^e splits into h = 1, m ~ 2^-7, l ~ 2^-15: the largest m l a truncating split can
    leave (|l| < 2^-7 |m|), so for all-positive operands the dropped terms add up to ~ 2 x 2^-22 S against the bound's 2^-20 S."""
    rng = np.random.default_rng(5)
    x = np.float32(1 + 2.0 ** -7 - 2.0 ** -23)
    X, W = (x * 2.0 ** rng.integers(-3, 4, (40, 64))).astype(np.float32), (x * 2.0 ** rng.integers(-3, 4, (24, 64))).astype(np.float32)
    ratio = (np.abs(R.y6(X, W) - R.y64(X, W)) / (R.DROPPED * R.s_fwd(X, W))).max()
    assert 0.4 < ratio <= 1.0, ratio
    X, W = np.abs(R.values("full24", (40, 64), "drop", "X")), np.abs(R.values("full24", (24, 64), "drop", "W"))
    ratio = (np.abs(R.y6(X, W) - R.y64(X, W)) / (R.DROPPED * R.s_fwd(X, W))).max()
    assert 0.1 < ratio <= 1.0, ratio


MUTANTS = [("lost", "lh", 2), ("lost", "hl", 2), ("lost", "mm", 2), ("swap", "A"), ("swap", "B"), ("dup", 5), ("bias2",)]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: "-".join(str(x) for x in m))
def test_the_yardstick_sees_a_mutant(mutant):
    """every mutant of the emulation misses |. - Y6| <= T_ACC S by at least a factor 2 in its worst element. A lost or swapped low term
    changes nothing where the operands have no low terms (low 16 bits clear) - not a defect there; the doubled bias needs a bias."""
    n = 0
    for case in R.precision_cases():
        if mutant[0] in ("lost", "swap") and "low16clear" in case[1]:
            assert np.array_equal(R.emulate(case[2], case[3], add=case[4], mutant=mutant), R.emulate(case[2], case[3], add=case[4]))
            continue
        if mutant[0] == "bias2" and case[4] is None:
            continue
        six, full, S = R.precision_reference(case)
        e = R.emulate(case[2], case[3], add=case[4], mutant=mutant)
        over = (np.abs(e - six) / (R.T_ACC[case[0]] * np.where(S == 0, 1, S))).max()
        assert over >= 2.0, (case[1], mutant, over)
        n += 1
    assert n >= 6
