"""The yardstick of tests/test_gpu_bpr_families.py, checked without a device (tests/_bpr_ref.py): the case table reaches all sixteen
run_stream<NV, VEC, ITEM, REG> instances of the scatter, every scalar trigger alone, every run-length edge, both sides of the 1024-slot
tree, every entry point and every refusal clause; the restated rules agree with what the built library answers without a device (its
constants and macros, the refusals that return before any HIP call); the per-element bounds are sound (the fp32 emulation of the kernels'
own order stays below HALF of them on the whole table) and not vacuous (CPU mutants exceed them at least twofold on the balanced cases);
the selection margin and the balance of the two gradient shares hold wherever they apply; and the reason for the yardstick is pinned: with
the regulariser's gradient share deleted, the inputs of tests/test_gpu_ops.py::test_bpr_prune_forward_backward still pass its rel_err.

The bounds' constants were fixed here, before the first device run."""
import re

import numpy as np

from tests import _bpr_ref as R

CASES = R.cases()
SCATTER = [c for c in CASES if c.flow not in ("rows", "rows_big")]
_memo = {}


def data(case):
    """(inputs, reference, emulation) of a case, computed once for the module and never changed"""
    if case.name not in _memo:
        inp = R.inputs(case)
        _memo[case.name] = (inp, R.reference(inp), R.emulate(inp))
    return _memo[case.name]


def by_name(name):
    return [c for c in CASES if c.name == name][0]


def run_lengths(inp, r=0):
    n, (u, p, q) = inp.case.valid(r), inp.idx[r]
    return set(np.unique(u[:n], return_counts=True)[1].tolist()), set(np.unique(np.concatenate([p[:n], q[:n]]), return_counts=True)[1].tolist())


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_scatter_instance_and_every_scalar_trigger():
    reached = {i for c in SCATTER for i in c.instances()}
    assert reached == R.ALL_INSTANCES and len(reached) == 16, sorted(R.ALL_INSTANCES - reached)
    assert {c.d for c in CASES if c.P == 1 and c.probs[0].lay == ("contig",) * 4 and c.B == (40,)} >= set(R.WIDTHS)
    for d in R.WIDTHS:                                            # a float4 width takes the float4 rows, every other one the scalar rows
        assert R.vec_of(d, by_name("w%d_bal" % d).probs) == (d % 4 == 0) and R.nv_of(d) == (1 if d <= 64 else 2)
    assert R.passes_of(129) == 2 and R.passes_of(128) == 1 and R.passes_of(65) == 1 and R.passes_of(200) == 2
    for o, w in R.TRIGGERS:                                       # one clause of the float4 test fails, on ONE operand of an otherwise float4 shape
        mine = [c for c in SCATTER if c.P == 1 and c.d == 64 and c.probs[0].lay == tuple(w if x == o else "contig" for x in R.OPERANDS)]
        assert len(mine) == 1 and not R.vec_of(64, mine[0].probs), (o, w)
        ld, col0, mod = R.layout_spec(w, 64)
        assert (ld % 4 != 0, mod % 16 != 0) == ((True, False) if w == "odd" else (False, True)) and ld >= 64 + col0
    assert {(False, 2, True, True), (False, 2, False, True)} <= by_name("odd_Ei_128").instances()
    assert not R.vec_of(64, by_name("mis_p1_64").probs) and R.vec_of(64, by_name("mis_p1_64").probs[:1])
    for d in (64, 128):                                           # ld > d alone keeps the float4 rows
        assert R.vec_of(d, by_name("pad%d" % d).probs) and R.layout_spec("pad", d)[0] > d


def test_the_table_reaches_every_run_and_batch_edge():
    inp, ref, _ = data(by_name("runs_bal"))
    users, items = run_lengths(inp)
    assert users >= set(R.RUN_EDGES) and items >= set(R.RUN_EDGES), (sorted(users), sorted(items))
    u, p, q = inp.idx[0]
    assert (p == q).sum() == 1 and len(set(p.tolist()) & set(q[p != q].tolist())) >= 1      # the same item twice in a sample; positive here, negative there
    assert {2 * n for n in users} >= {16, 32, 30, 34} and by_name("runs_p2").P == 2         # (problems x members) around 16 and 32
    assert {5 * n for n in users} >= {15, 35} and by_name("runs_step").P == 5
    for name, reg in (("runs_bal", True), ("runs_mf", False)):    # a dropped sample in the middle of a sixteen: kept as a record with ds = 0 / skipped
        inp, ref, _ = data(by_name(name))
        keep, u = ref[0]["keep"][0], inp.idx[0][0]
        slots = np.flatnonzero(u == R.RUN_LENS.index(33))[:16]
        assert not keep[slots[1:15]].all() and keep[slots[1:15]].any()
        assert (True in {i[3] for i in by_name(name).instances()}) == reg
    assert {c.B[0] for c in CASES if len(c.B) == 1 and c.d == 16 and c.regime == "bal"} >= set(R.BATCHES)
    assert {c.valid(0) for c in CASES} >= {0, 1, 1023, 1024, 1025, 1126}                      # both sides of the 1024-slot tree
    nv = {c.name: c for c in CASES}
    assert nv["nv25"].valid(0) == 25 and nv["nv0"].valid(0) == 0 and nv["nv_over"].n_valid[0] > 40 and nv["nv_over"].valid(0) == 40
    assert nv["nv_neg"].n_valid[0] < 0 and nv["nv_neg"].valid(0) == 0
    big = nv["rows_big"]
    assert big.d == 4 and R.ceil_div(R.ceil_div(big.B[0], R.ROWS_PER_BLOCK), R.ROWS_BLOCKS) == 2 and big.valid(0) < big.B[0]


def test_the_table_reaches_every_entry_point_and_sharing_pattern():
    assert {e for c in CASES for e in R.FLOWS[c.flow]} == R.ENTRY_POINTS
    assert R.ENTRY_POINTS == {"llmrec_bpr_prune_fwd_f32", "llmrec_bpr_prune_bwd_f32", "llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_bwd_f32",
                              "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32", "llmrec_bpr_multi_losses_f32",
                              "llmrec_bpr_multi_fwd_sharded_f32", "llmrec_bpr_prune_fwd_sharded_f32", "llmrec_bpr_prune_bwd_rows_f32",
                              "llmrec_bpr_multi_zero_rows_f32"}
    assert {c.P for c in SCATTER} >= {1, 2, 5, 8} and {c.regime for c in CASES} == set(R.REGIMES)
    step = by_name("runs_step")
    assert [len(m) for _, m in R.groups(step.probs, "u")] == [5] and len(R.groups(step.probs, "i")) == 5
    assert [o for o, _ in R.groups(by_name("owner1").probs, "u")] == [0, 1] and R.groups(by_name("owner1").probs, "i")[0] == (0, [0, 2])
    mixed = by_name("mixed_reg")
    assert [p.g_emb != 0 for p in mixed.probs] == [False, True] and R.groups(mixed.probs, "u") == [(0, [0, 1])]
    sh = by_name("sharded")
    assert len(sh.B) == 3 and sorted(sh.valid(r) for r in range(3))[0] == 0 and len({sh.valid(r) for r in range(3)}) == 3
    for name in ("self_prune", "self_fused", "triple_prune", "triple_fused", "sharded_self", "prune_sharded_triple"):   # the threshold lies INSIDE a tie group
        inp, ref, _ = data(by_name(name))
        m = np.concatenate([o["m"][0][0] for o in ref])
        keep = np.concatenate([o["keep"][0] for o in ref])
        tie = np.concatenate([inp.tie[r][:ref[r]["n"]] for r in range(len(ref))])
        cls = tie[np.lexsort((np.arange(len(m)), m))[ref[0]["k"] - 1]]
        grp = np.flatnonzero(tie == cls)
        assert len(grp) >= 4 and np.ptp(m[grp]) == 0 and 0 < keep[grp].sum() < len(grp)
        assert keep[grp].tolist() == sorted(keep[grp].tolist(), reverse=True), "ties go to the lower global index"
        if len(ref) > 1:                                          # ... and across a rank boundary in the gathered forms
            rank_of = np.concatenate([np.full(o["n"], r) for r, o in enumerate(ref)])
            assert len(set(rank_of[grp][keep[grp]].tolist()) | set(rank_of[grp][~keep[grp]].tolist())) >= 2
    assert {c.name for c in CASES if R.k_of(c.remember or 0.5, sum(c.valid(r) for r in range(len(c.B)))) == 0 and c.valid(0) > 0} >= {"k0", "k0_bal", "k0_rows", "b1"}


# ------------------------------------------------------------------------------------------------------------------------------------
# the restated rules against the built library (nothing here initialises a device)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_restated_constants_and_macros():
    from llmrec_amd import _lib, ops
    assert _lib.CONST["LLMREC_BPR_MAX_B"] == R.MAX_B and _lib.CONST["LLMREC_BPR_MAX_PROBLEMS"] == R.MAX_PROBLEMS
    assert _lib.EUNSUPPORTED == R.EUNSUPPORTED
    text = open(_lib.HEADER).read()
    macros = {m[0]: (m[1], m[2]) for m in re.findall(r"#define\s+(LLMREC_BPR_\w+)\(([^)]*)\)\s+(\([^/\n]*\))", text)}
    assert set(macros) >= {"LLMREC_BPR_SAVED_FLOATS", "LLMREC_BPR_GATHER_FLOATS", "LLMREC_BPR_PLAN_WORDS"}

    def macro(name, *args):
        params, body = macros[name]
        return eval(body, {}, dict(zip([p.strip() for p in params.split(",")], args)))

    for B in (0, 1, 40, 1126, 4096):
        assert macro("LLMREC_BPR_SAVED_FLOATS", B) == R.saved_floats(B) == ops.bpr_saved_floats(B)
        assert macro("LLMREC_BPR_PLAN_WORDS", B) == R.plan_words(B) == ops.bpr_plan_words(B)
        for P in (1, 2, 8):
            assert macro("LLMREC_BPR_GATHER_FLOATS", P, B) == R.gather_floats(P, B)
    flat = np.arange(R.saved_floats(7), dtype=np.float32)
    sv = R.Saved(flat, 7)                                         # the layout bpr.hip states: coefficient | Su Sp Sq k | m, sg, nu, np, nq
    assert sv.coef[0] == 0 and sv.S[0] == 7 and sv.k == 10 and [x[0] for x in (sv.m, sv.sg, sv.nu, sv.np, sv.nq)] == [11, 18, 25, 32, 39] and len(sv.tail) == 4
    assert R.SHARDED_MULTI_CAP == 16384 and R.SHARDED_PRUNE_CAP == 3 * 4096


def test_refusals_return_before_any_hip_call():
    """every refusal clause once per entry point that has it, with made-up addresses that are never dereferenced: the checks run on the
    host, ahead of the launch. Where a device is present such addresses must not reach a kernel even by mistake, so the calls are made
    only on a machine without one."""
    import torch
    from tests.test_gpu_bpr_families import call
    if torch.cuda.is_available():
        return
    A = 0x10000000
    prob = dict(Eu=(A, 64), Ei=(A + 0x100000, 64), dEu=(A + 0x200000, 64), dEi=(A + 0x300000, 64), g_mf=0.7, g_emb=1.0)
    base = dict(probs=[prob], d=64, users=A + 0x400000, pos=A + 0x500000, neg=A + 0x600000, B_max=40, remember=0.29, decay=1.0, flag=1.0,
                out=A + 0x700000, saved=A + 0x800000, plan=A + 0x900000, grads2=A + 0xa00000, rows3=A + 0xb00000, gather_block=A + 0xc00000,
                gathered=A + 0xd00000, global_m=A + 0xe00000)
    multi = ["llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_bwd_f32", "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32",
             "llmrec_bpr_multi_losses_f32", "llmrec_bpr_multi_zero_rows_f32", "llmrec_bpr_multi_fwd_sharded_f32"]
    seen = set()

    def expect(clause, code, entry, **kw):
        assert code != 0 and call(entry, **{**base, **kw}) == code, (clause, entry)
        seen.add(clause)

    for entry in ("llmrec_bpr_prune_fwd_f32", "llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32",
                  "llmrec_bpr_multi_losses_f32", "llmrec_bpr_multi_fwd_sharded_f32", "llmrec_bpr_scatter_plan", "llmrec_bpr_prune_fwd_sharded_f32"):
        expect("B_max 4097", R.refuse_cap(4097), entry, B_max=4097, scores_only=1)
        assert R.refuse_cap(4096) == 0
    for entry in multi:
        expect("n_problems 0", R.refuse_n_problems(0), entry, n_problems=0)
        expect("n_problems 9", R.refuse_n_problems(9), entry, n_problems=9)
    short = lambda **kw: [dict(prob, **kw)]
    for entry, kw in (("llmrec_bpr_prune_fwd_f32", dict(Eu=(A, 63))), ("llmrec_bpr_multi_fwd_f32", dict(Ei=(A, 63))),
                      ("llmrec_bpr_prune_bwd_f32", dict(dEu=(A + 0x200000, 63))), ("llmrec_bpr_prune_bwd_rows_f32", dict(Ei=(A, 63))),
                      ("llmrec_bpr_multi_zero_rows_f32", dict(dEi=(A + 0x300000, 63))), ("llmrec_bpr_multi_bwd_f32", dict(dEu=(A + 0x200000, 63))),
                      ("llmrec_bpr_prune_fwd_sharded_f32", dict(Eu=(A, 63)))):
        expect("ld < d", R.refuse_ld(63, 64), entry, probs=short(**kw), scores_only=1)
    for entry, kw in (("llmrec_bpr_prune_fwd_f32", dict(Eu=(None, 64))), ("llmrec_bpr_multi_fwd_f32", dict(Ei=(None, 64))),
                      ("llmrec_bpr_prune_bwd_f32", dict(dEi=(None, 64))), ("llmrec_bpr_multi_bwd_f32", dict(dEu=(None, 64))),
                      ("llmrec_bpr_multi_scores_f32", dict(Eu=(None, 64))), ("llmrec_bpr_prune_bwd_rows_f32", dict(Eu=(None, 64)))):
        expect("null table", R.refuse_null(None), entry, probs=short(**kw))
    expect("dEu == dEi", R.refuse_same_target(1, 1), "llmrec_bpr_prune_bwd_f32", probs=short(dEi=prob["dEu"]))
    expect("phase 3", R.refuse_phase(3), "llmrec_bpr_multi_fwd_sharded_f32", phase=3)
    assert R.refuse_phase(1) == R.refuse_phase(2) == 0
    need = R.gather_floats(1, 40)
    expect("short rank_stride", R.refuse_rank_stride(need - 1, 1, 40), "llmrec_bpr_multi_fwd_sharded_f32", phase=2, n_ranks=3, rank_stride=need - 1)
    assert R.refuse_rank_stride(need, 1, 40) == 0
    expect("n_ranks B_max > 16384", R.refuse_sharded_capacity(5, 4096), "llmrec_bpr_multi_fwd_sharded_f32", phase=2, n_ranks=5, B_max=4096,
           rank_stride=R.gather_floats(1, 4096))
    assert R.refuse_sharded_capacity(4, 4096) == 0
    expect("global_B > 3 4096", R.refuse_global_batch(3 * 4096 + 1), "llmrec_bpr_prune_fwd_sharded_f32", global_B=3 * 4096 + 1)
    assert R.refuse_global_batch(3 * 4096) == 0
    assert seen == set(R.REFUSALS)
    for entry in ("llmrec_bpr_multi_bwd_f32", "llmrec_bpr_multi_select_bwd_f32", "llmrec_bpr_multi_zero_rows_f32", "llmrec_bpr_prune_bwd_f32",
                  "llmrec_bpr_prune_bwd_rows_f32", "llmrec_bpr_scatter_plan"):
        assert call(entry, **{**base, "B_max": 0}) == 0, entry    # an empty capacity: nothing to launch


# ------------------------------------------------------------------------------------------------------------------------------------
# soundness, margin, balance
# ------------------------------------------------------------------------------------------------------------------------------------
def test_emulations_stay_below_half_of_the_bounds(capsys):
    worst = {}
    for case in CASES:
        inp, ref, emu = data(case)
        for got, want in zip(emu, ref):
            assert np.array_equal(got["keep"], want["keep"]), case.name
            for g, v in R.ratios(got, want).items():
                assert v <= 0.5, (case.name, g, v)
                worst[g] = max(worst.get(g, 0.0), v)
    assert set(worst) == {"scores", "norms", "coef", "S", "mf", "emb", "dEu", "dEi", "rows3"}
    assert min(v for g, v in worst.items() if g not in ("mf", "emb", "S")) > 0.1, worst     # ... and not by orders of magnitude (a tree's errors
    #                                                                                        largely cancel: its worst-case bound is the issue's)
    with capsys.disabled():
        print("\n[bpr yardstick] worst emulation error / bound: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def test_the_selection_margin_holds_for_every_case_that_selects(capsys):
    """the fp64 gap between the k-th and the (k + 1)-th smallest m is at least 4 x the m bound of both - or both lie in one exact-tie
    class, and then the nearest samples outside the class are that far away. (rows_big selects nothing on the device: its `saved` is the
    reference's.)"""
    worst = np.inf
    for case in CASES:
        if case.flow == "rows_big":
            continue
        inp, ref, _ = data(case)
        margin = R.selection_margin(inp, ref)
        assert margin >= 4.0, (case.name, margin)
        worst = min(worst, margin)
    with capsys.disabled():
        print("\n[bpr yardstick] smallest selection gap / m bound: %.3g" % worst)


def test_the_balanced_regime_is_balanced_on_every_row(capsys):
    lo, hi, n = np.inf, 0.0, 0
    for case in CASES:
        inp, ref, _ = data(case)
        assert case.decay == 1.0 and case.flag == 1.0 and float(np.abs(inp.Eu[0]).max()) > 0.3     # (by the weights, never by the table scale)
        for r, want in enumerate(ref):
            a, b = R.balance(want, case.probs)
            mags = [k for k in want if k.startswith("mag_")]
            if case.regime != "bal" or not mags or want["k"] == 0 or want["n"] == 0:
                continue
            assert 0.1 <= a and b <= 30.0, (case.name, r, a, b)
            lo, hi, n = min(lo, a), max(hi, b), n + 1
    assert n >= 40
    with capsys.disabled():
        print("\n[bpr yardstick] sum|c self| / sum|ds (.)| per destination row, balanced cases: %.3g .. %.3g" % (lo, hi))


# ------------------------------------------------------------------------------------------------------------------------------------
# sharpness: CPU mutants exceed the bounds at least twofold on the balanced cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _applies(mutant, case, inp, ref):
    n, k = sum(o["n"] for o in ref), ref[0]["k"]
    dense = case.flow not in ("rows", "rows_big")
    if n == 0:
        return False
    if mutant in ("reg_deleted", "reg_sign", "reg_x10", "cp_cq_swap"):
        return True
    if mutant == "neg_ds_sign":
        return k > 0
    if mutant == "keep_next":
        return 0 < k < n
    if mutant == "tie_high":
        return case.idx in ("self", "triple")
    if mutant == "drop_17th":
        return dense and any(len(m) * ln == 17 for side, lens in zip("ui", run_lengths(inp)) for _, m in R.groups(case.probs, side) for ln in lens)
    if mutant == "overwrite":
        return dense
    if mutant == "rows3_swap":
        return case.P == 1
    raise KeyError(mutant)


def _worst(case, inp, ref, mutant):
    return max(v for got, want in zip(R.emulate(inp, mutant), ref) for v in R.ratios(got, want).values())


def test_mutants_exceed_the_bounds_twofold(capsys):
    """every mutant on every balanced case it applies to"""
    least = {}
    for case in CASES:
        if case.regime != "bal":
            continue
        inp, ref, _ = data(case)
        for mutant in R.MUTANTS:
            if mutant == "no_eps" or not _applies(mutant, case, inp, ref):
                continue
            r = _worst(case, inp, ref, mutant)
            assert r >= 2.0, (case.name, mutant, r)
            least[mutant] = min(least.get(mutant, np.inf), r)
    assert set(least) == set(R.MUTANTS) - {"no_eps"}
    with capsys.disabled():
        print("\n[bpr yardstick] least mutant error / bound over the balanced cases: " + ", ".join("%s %.3g" % kv for kv in sorted(least.items())))


def test_the_epsilon_of_x_is_below_the_resolution_of_every_stored_value(capsys):
    """x = dp - dn + 1e-8 is never stored; it reaches memory through m = logsigmoid(x) and sigmoid(-x) only, and both have slopes <= 1
    where their values are ~0.69 and ~0.5: omitting the 1e-8 moves them by at most 1e-8, a sixth of one rounding of m. So no fp32 check
    of the stored values can see that mutant, and none is claimed - the issue's list names it, and it is the one mutant that is NOT shown
    twofold: here it moves no stored value by more than two ulp (a rounding that falls the other way) and stays inside HALF of every
    bound, like the unmutated emulation. (The other epsilon, 2 S + 1e-8, IS pinned: n_valid = 0 gives emb = 3 decay / (1e-8 flag), finite,
    in the nv0 cases.)"""
    worst_ulp, worst_ratio = 0.0, 0.0
    for name in ("w16_bal", "self_prune", "w200_bal"):
        case = by_name(name)
        inp, ref, emu = data(case)
        mut = R.emulate(inp, "no_eps")
        for key in ("m", "sg"):
            ulp = np.abs(mut[0][key].astype(np.float64) - emu[0][key]) / np.spacing(np.abs(emu[0][key]))
            worst_ulp = max(worst_ulp, float(ulp.max()))
        worst_ratio = max(worst_ratio, _worst(case, inp, ref, "no_eps"))
    assert worst_ulp <= 2.0 and worst_ratio <= 0.5
    inp, ref, emu = data(by_name("nv0"))
    want = 3.0 / R.EPS32
    assert np.isfinite(ref[0]["emb"][0]).all() and abs(ref[0]["emb"][0][0] - want) <= 1e-12 * want and abs(float(emu[0]["emb"][0]) - want) <= ref[0]["emb"][1][0]
    with capsys.disabled():
        print("\n[bpr yardstick] 1e-8 omitted from x: at most %.2g ulp of m / sigmoid(-x), %.3g of a bound" % (worst_ulp, worst_ratio))


# ------------------------------------------------------------------------------------------------------------------------------------
# why this yardstick: the old regime hides the regulariser's gradient share
# ------------------------------------------------------------------------------------------------------------------------------------
def test_a_deleted_regulariser_share_passes_the_old_rel_err_and_fails_the_bound():
    """the inputs of tests/test_gpu_ops.py::test_bpr_prune_forward_backward (B = 1126, d = 64: tables x 0.3, decay 1e-5, flag 1024, weights
    0.7 / 1.3): there the regulariser's share is ~1e-12 of the tensor maximum, so the kernel with the share deleted, sign-flipped or
    multiplied by ten passes max|a - b| / max|b| < 2e-5. On a balanced case the same mutants are far outside the per-element bound."""
    rng = np.random.default_rng(1126)
    U_, I_, d, B = 300, 500, 64, 1126
    Eu = (rng.standard_normal((U_, d)) * 0.3).astype(np.float32)
    Ei = (rng.standard_normal((I_, d)) * 0.3).astype(np.float32)
    idx = tuple(rng.integers(0, n, size=B).astype(np.int64) for n in (U_, I_, I_))
    case = R.Case("old", "prune", d, (B,), (None,), U_, I_, (R.Prob(0.7, 1.3, 0, 0),), "bal", 1 - 0.71, decay=1e-5, flag=1024.0)
    inp = R.Inputs(case, [Eu], [Ei], [idx], {0: np.zeros((U_, d), dtype=np.float32)}, {0: np.zeros((I_, d), dtype=np.float32)}, 1 - 0.71,
                   [-1 - np.arange(B, dtype=np.int64)])
    ref = R.reference(inp)[0]

    def rel_err(a, b):                                            # tests/test_gpu_ops.py
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)

    share = max(float(ref["mag_u0"][1].max() / np.abs(ref["dEu0"][0]).max()), float(ref["mag_i0"][1].max() / np.abs(ref["dEi0"][0]).max()))
    assert share < 1e-10
    for mutant in (None, "reg_deleted", "reg_sign", "reg_x10", "cp_cq_swap"):
        got = R.emulate(inp, mutant)[0]
        assert np.array_equal(got["keep"], ref["keep"])
        assert rel_err(got["dEu0"], ref["dEu0"][0]) < 2e-5 and rel_err(got["dEi0"], ref["dEi0"][0]) < 2e-5, mutant   # the old check passes
    balanced = by_name("w64_bal")
    inp2, ref2, emu2 = data(balanced)
    for mutant in ("reg_deleted", "reg_sign", "reg_x10", "cp_cq_swap"):
        r = R.ratios(R.emulate(inp2, mutant)[0], ref2[0])
        assert min(r["dEu"] if mutant != "cp_cq_swap" else r["dEi"], r["dEi"]) >= 2.0, (mutant, r)                    # the new one does not
    assert max(R.ratios(emu2[0], ref2[0]).values()) <= 0.5
