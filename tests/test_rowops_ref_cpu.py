"""The yardstick of tests/test_gpu_rowops_families.py, checked without a device (tests/_rowops_ref.py): the case table reaches every
<VEC, NCHUNK> instance of the six templated row kernels, every refusal clause and both regimes of every grid-stride sweep; the restated
rules agree with what the built library answers without a device (its constants, its workspace queries, the refusals that return before
any HIP call); the per-element bounds are sound (the fp32 emulations of the kernels' order stay below HALF of them) and not vacuous (CPU
mutants of the emulations exceed them at least twofold); and the reason for the new yardstick is pinned: an error the per-tensor
max-normalised rel_err of tests/test_gpu_ops.py lets through fails the per-element bound.

The bounds' constants were fixed here, before the first device run."""
import numpy as np

from tests import _rowops_ref as R


def _inst(case):
    return [case.expect(m) for m in R.MODES.get(case.entry, (None,))]


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_instance_and_every_refusal_clause():
    cases = R.cases()
    for entry in R.TEMPLATED:
        mine = [c for c in cases if c.entry == entry]
        assert {i for c in mine for i in _inst(c)} == R.ALL_INSTANCES, entry
        assert {c.d for c in mine if c.layout == "contig" and c.d % 4 == 0 and max(c.rows + c.rows1) < R.BIG_ROWS} >= set(R.D_FLOAT4)
        assert {c.d for c in mine if c.layout == "contig" and c.d % 4} >= set(R.D_SCALAR) - {16}
        for c in mine:
            assert set(c.rows) == set(R.SMALL_ROWS) or max(c.rows + c.rows1) == R.BIG_ROWS
        forced = [c for c in mine if c.layout in R.FORCED and c.d != 20]
        assert {(c.d, c.layout) for c in forced} == {(d, w) for d in (64, 128) for w in R.FORCED} | {(16, "ld1")}
        assert [_inst(c) for c in forced if c.d == 16][0][-1] == (1, 1)
        forced = [c for c in forced if c.d != 16]
        for c in forced:                                          # one clause of vec4_of decides, on ONE operand
            specs = [c.spec(o) for o in R.OPERANDS[entry]]
            assert sum(s != R.layout_spec("contig", c.d) for s in specs) == 1 and c.d % 4 == 0
            lds_ok, bases_ok = all(s[0] % 4 == 0 for s in specs), all(s[2] % 16 == 0 for s in specs)
            assert (lds_ok, bases_ok) == ((True, False) if c.layout == "mis_base" else (False, True))
            assert (1, {64: 4, 128: 8}[c.d]) in _inst(c)
        assert len({c.operand for c in forced}) >= min(3, len(R.OPERANDS[entry]) - 1), "the deviating operand rotates"
        assert {c.d for c in mine if c.layout == "slice"} == {64, 128, 256, 512}
        assert all(c.vec4() for c in mine if c.layout == "slice")
    ref = R.refusals()
    for entry in R.TEMPLATED:
        mine = [c for c in ref if c.entry == entry]
        assert {(c.d, c.layout) for c in mine} == {(516, "contig"), (257, "contig"), (260, "mis_base")}
        for c in mine:
            assert all(i is None for i in _inst(c))
        assert [c.vec4("source") for c in mine] == [True, False, False]
    compact = [c for c in ref if c.entry == "fuse_fwd_multi_sumsq_compact"]
    assert len(compact) == 1 and compact[0].expect() is None and R.instance(compact[0].d, False) is not None


def test_the_table_reaches_both_regimes_of_every_sweep():
    cases = R.cases()
    assert R.row_passes(R.MAX_BLOCKS * R.ROWS_PER_BLOCK) == 1 and R.row_passes(R.BIG_ROWS) == 2
    for entry in R.TEMPLATED:
        mine = [c for c in cases if c.entry == entry]
        for vec4, d, layout in ((True, 64, "contig"), (False, 20, "ld1")):
            sel = [c for c in mine if c.d == d and c.layout == layout]
            assert [i for c in sel for i in _inst(c)][-1] == ((4, 1) if vec4 else (1, 4))
            fam = [c for c in mine if c.vec4("source") == vec4]   # (one pass: the small row counts at every d)
            assert {R.row_passes(r) for c in sel for r in c.rows} >= {2} and {R.row_passes(r) for c in fam for r in c.rows} == {1, 2}, (entry, d)
            if sel[0].rows1:                                      # the paired launches: a second pass in either problem's block range
                assert {(R.row_passes(a), R.row_passes(b)) for c in sel for a, b in zip(c.rows, c.rows1)} >= {(2, 1), (1, 2)}
                assert (1, 1) in {(R.row_passes(a), R.row_passes(b)) for c in fam for a, b in zip(c.rows, c.rows1)}
            assert all(c.vec4("source") == vec4 for c in sel)
    g = R.group_cases()
    assert {(R.row_passes(c.fuse_rows[0]), R.row_passes(c.sm_rows)) for c in g} == {(1, 1), (2, 1), (1, 2)}
    flat = R.flat_cases()
    for entry, per_block, cap in (("sumsq", 256 * 8, R.SUMSQ_BLOCKS), ("axpy", 256 * 4, R.MAX_BLOCKS), ("adamw", 256 * 4, R.MAX_BLOCKS),
                                  ("scale_rows", 256 * 4, R.MAX_BLOCKS)):
        passes = {R.flat_passes(c.rows * c.d, per_block, cap) for c in flat if c.entry == entry}
        assert min(passes) <= per_block // 256 < max(passes), (entry, passes)      # (a block's own share is per_block / 256 trips of a thread)
    big = [c for c in flat if c.entry == "sumsq" and c.rows * c.d == R.FLAT_BIG]
    assert len(big) == 1 and big[0].ld > big[0].d
    assert {c.rows * c.d for c in flat if c.entry in ("axpy", "adamw")} == {1000, R.FLAT_BIG}


def test_visits_of_the_sweep():
    for rows in (1, 16, 17, 67, R.BIG_ROWS):
        assert (R.visits(rows, R.row_blocks(rows)) == 1).all()
    twice = R.visits(R.BIG_ROWS, R.MAX_BLOCKS, R.MAX_BLOCKS - 1)      # the mutant stride nvb 16 - 16
    assert twice.min() == 1 and twice.max() == 2


# ------------------------------------------------------------------------------------------------------------------------------------
# the restated rules against the built library (nothing here initialises a device)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_restated_constants_and_workspace_queries():
    from llmrec_amd import _lib
    assert _lib.CONST["LLMREC_MAX_TERMS"] >= max(R.N_MEAN, R.N_NORM)
    assert _lib.CONST["LLMREC_ADAMW_CHUNK"] == 1024 and _lib.CONST["LLMREC_ADAMW_MAX_TENSORS"] >= 2
    assert _lib.CONST["LLMREC_COLSUM_MAX_GROUPS"] == 8
    assert _lib.EUNSUPPORTED == R.EUNSUPPORTED
    for rows, d in ((0, 0), (1, 1), (50, 20), (51169, 41), (1 << 30, 64)):
        assert _lib.query("llmrec_sumsq_workspace_bytes", rows, d) == 4 * R.SUMSQ_BLOCKS
    for d in (1, 40, 192, 512):
        assert _lib.query("llmrec_weighted_colsum_workspace_bytes", d) == 4 * R.COLSUM_BLOCKS * d
    assert _lib.query("llmrec_weighted_colsum_workspace_bytes", 513) == -1 and _lib.query("llmrec_weighted_colsum_workspace_bytes", 0) == -1
    assert R.sumsq_blocks(R.FLAT_BIG) == R.SUMSQ_BLOCKS and R.sumsq_blocks(1000) == 1 and R.sumsq_blocks(0) == 1


def _fake_pointers(case):
    """made-up, never dereferenced addresses with the case's alignment: a refusal returns before the first HIP call"""
    return {o: (0x10000000 + 0x1000000 * k + case.spec(o)[2], case.spec(o)[0]) for k, o in enumerate(R.OPERANDS[case.entry])}


def test_refusals_return_before_any_hip_call():
    """dispatch_rows refuses on the host, ahead of the launch: LLMREC_EUNSUPPORTED for every refusal of the table, LLMREC_EINVAL for an
    ld < d. Where a device is present the addresses below must not reach a kernel even by mistake, so the calls are made only on a
    machine without one; tests/test_gpu_rowops_families.py makes them with real buffers."""
    import ctypes
    import torch
    from tests.test_gpu_rowops_families import launch
    if torch.cuda.is_available():
        return
    for case in R.refusals():
        n = (case.rows[0], case.rows1[0]) if case.rows1 else case.rows[0]
        extra = {}
        if case.entry == "fuse_fwd_multi_sumsq_compact":
            extra = dict(sumsq=(2, 0x50000000, 64, ctypes.c_int32(-1)), compact=(100, 0x60000000, 0x61000000, 0x62000000))
        for mode in R.MODES.get(case.entry, (None,)):
            assert launch(case.entry, case.d, n, _fake_pointers(case), mode=mode, **extra) == R.EUNSUPPORTED, (case.name, mode)
    for entry in R.TEMPLATED:
        case = R.Case(entry, 64, "contig", None, **R._rows(entry, (17,)))
        P = _fake_pointers(case)
        first = R.OPERANDS[entry][0]
        P[first] = (P[first][0], 63)
        n = (17, 37) if case.rows1 else 17
        for mode in R.MODES.get(entry, (None,)):
            assert launch(entry, 64, n, P, mode=mode) == R.EINVAL, (entry, mode)
            assert launch(entry, 64, (0, 0) if case.rows1 else 0, _fake_pointers(case), mode=mode) == 0, (entry, mode)


# ------------------------------------------------------------------------------------------------------------------------------------
# soundness: the emulations of the kernels' own order stay below half of the bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _maths():
    """the distinct (d, rows, instance) the table runs, per arithmetic (the paired kernels run the single kernels' row bodies)"""
    seen = {}
    for c in R.cases():
        kind = {"softmax_fwd": "softmax_fwd", "softmax_bwd": "softmax_bwd", "fuse_fwd": "fuse_fwd", "fuse_fwd_multi": "fuse_fwd"}.get(c.entry, "fuse_bwd")
        for mode in R.MODES.get(c.entry, ("source",) if kind == "fuse_bwd" else (None,)):
            for rows in {max(c.rows)} | ({max(c.rows1)} if c.rows1 else set()):
                seen[(kind, mode, c.d, rows, c.expect(mode))] = True
    return sorted(seen, key=str)


def _ratio(got, want, bound):
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)                 # (a mutant may produce inf / nan: as wrong as can be)
    return float((err / np.maximum(bound, 1e-300)).max())


def _bases(f, mode):
    return {"overwrite": (None,) * R.N_NORM, "accumulate": f.olds, "source": f.srcs}[mode]


def _run(kind, mode, d, rows, inst, mutant=None, **kw):
    """(worst emulation error / bound, worst bound / |value| ... ) of one arithmetic at one shape"""
    VEC, NCHUNK = inst
    L = VEC * NCHUNK
    if kind.startswith("softmax"):
        Z, Y, dY = R.softmax_inputs(rows, d, "softmax", d)
        if kind == "softmax_fwd":
            return _ratio(R.emu_softmax_fwd(Z, VEC, NCHUNK, mutant), *R.softmax_fwd(Z, L))
        return _ratio(R.emu_softmax_bwd(Y, dY, R.ALPHA, VEC, NCHUNK, mutant), *R.softmax_bwd(Y, dY, R.ALPHA, L))
    f = R.fuse_inputs(rows, d, "fuse", d, 0)
    if kind == "fuse_fwd":
        return _ratio(R.emu_fuse_fwd(f.means, R.MEAN_SCALE, f.norms, R.RATES, VEC, NCHUNK, mutant), *R.fuse_fwd(f.means, R.MEAN_SCALE, f.norms, R.RATES, L))
    bases = kw.get("bases", _bases(f, mode))
    got = R.emu_fuse_bwd(f.G, f.norms, R.RATES, bases, R.N_REG, R.REG2, VEC, NCHUNK, mutant, kw.get("count"))
    ref = R.fuse_bwd(f.G, f.norms, R.RATES, L, _bases(f, mode), R.N_REG, R.REG2)
    return max(_ratio(g, want, bound) for g, (want, bound) in zip(got, ref))


def test_emulations_stay_below_half_of_the_bounds(capsys):
    worst = {}
    for kind, mode, d, rows, inst in _maths():
        if inst is None:
            continue
        r = _run(kind, mode, d, rows, inst)
        assert r <= 0.5, (kind, mode, d, rows, inst, r)
        key = "%s%s" % (kind, " " + mode if mode else "")
        worst[key] = max(worst.get(key, 0.0), r)
    for fc in R.flat_cases():
        if fc.entry == "sumsq":
            X = R.mixed(fc.rows, fc.d, "sumsq", fc.rows)
            blocks = R.sumsq_blocks(X.size)
            for old in (None, 0.375):
                want, bound = R.sumsq(X, 1e-5 * 0.5 / 80, old, blocks)
                r = abs(float(R.emu_sumsq(X, 1e-5 * 0.5 / 80, old, blocks)) - want) / bound
                assert r <= 0.5, (fc, old, r)
                worst["sumsq"] = max(worst.get("sumsq", 0.0), r)
    assert min(v for k, v in worst.items() if k != "sumsq") > 0.1, worst     # ... and not by orders of magnitude (sumsq: a tree's errors
    #                                                                          largely cancel, its worst-case bound is the issue's)
    with capsys.disabled():
        print("\n[rowops yardstick] worst emulation error / bound: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def test_every_row_of_a_normalised_term_is_clamped_or_far_from_the_clamp():
    for rows, d in ((67, 1), (67, 4), (67, 255), (67, 512), (R.BIG_ROWS, 64), (R.BIG_ROWS, 20)):
        f = R.fuse_inputs(rows, d, "fuse", d, 0)                  # (asserts the split itself)
        R.check_fuse_split(R.fuse_cut(f, min(rows, 17)))
        r = np.arange(rows)
        assert (r % 16 == R.ZERO_ROW).any() == (rows > 1) and not f.norms[0][r % 16 == R.ZERO_ROW].any()


def test_adamw_reference_holds_the_edges():
    p, g, m, v = R.adamw_inputs(1000, "edges")
    state = R.adamw_state(1, R.ADAMW["lr"], R.ADAMW["b1"], R.ADAMW["b2"])
    assert state.view(np.int32)[0] == 1 and abs(float(state[1]) / (1e-3 / 0.1) - 1) < 1e-6 and abs(float(state[2]) / np.sqrt(1e-3) - 1) < 1e-5
    ref = R.adamw(p, g, m, v, state, **R.ADAMW)
    assert g[0] == 0 and v[0] == 0 and ref["p"][0][0] == float(p[0]) * float(np.float32(1 - float(np.float32(1e-3)) * float(np.float32(0.01))))
    assert abs(g[2]) == np.float32(1e-30) and abs(g[4]) == np.float32(1e19) and np.isfinite(ref["v"][0][4])
    assert np.isinf(ref["v"][0][6]) and np.isinf(ref["v"][0][7]) and ref["p"][0][6] == float(p[6]) * float(np.float32(1 - float(np.float32(1e-3)) * float(np.float32(0.01))))
    assert (p[8:12] < 0).all()
    f = np.float32                                                # an fp32 evaluation in the kernel's order stays inside half the bound
    w1, w2 = f(1) - f(0.9), f(1) - f(0.999)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m1 = (m + (w1 * (g - m).astype(f)).astype(f)).astype(f)
        v1 = ((((w2 * g).astype(f)).astype(np.float64) * g.astype(np.float64)) + (v * f(0.999)).astype(f).astype(np.float64)).astype(f)
        den = ((np.sqrt(v1).astype(f) / state[2]).astype(f) + f(1e-8)).astype(f)
        dec = f(1.0 - float(f(1e-3)) * float(f(0.01)))
        p1 = ((p * dec).astype(f) - (state[1] * (m1 / den).astype(f)).astype(f)).astype(f)
    for got, k in ((p1, "p"), (m1, "m"), (v1, "v")):
        want, bound = ref[k]
        inf = np.isinf(want)
        assert np.array_equal(got[inf].astype(np.float64), want[inf])
        assert (np.abs(got[~inf].astype(np.float64) - want[~inf]) <= bound[~inf] / 2).all(), k
    bad = p1.copy()
    for _ in range(6):                                            # six ulp off: outside
        bad[20] = np.nextafter(bad[20], f(9))
    assert abs(float(bad[20]) - ref["p"][0][20]) > ref["p"][1][20]


# ------------------------------------------------------------------------------------------------------------------------------------
# sharpness: CPU mutants of the emulations exceed the bounds at least twofold
# ------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {"softmax_fwd": ("no_last_chunk", "no_last_step"), "softmax_bwd": ("no_last_chunk", "no_last_step", "no_alpha"),
           "fuse_fwd": ("no_last_chunk", "no_last_step", "clamp_wrong", "mean_scale_late"),
           "fuse_bwd": ("no_last_chunk", "no_last_step", "clamp_wrong", "reg_one_more")}


def test_mutants_exceed_the_bounds_twofold():
    """every mutant, at every instance, on the table's own inputs. (A mutant can be the kernel itself at a shape: the last chunk may be
    all padding, at d = 1 or 4 only lane 0 holds data, and the softmax backward of a one-column row is 0 whatever alpha is - so the
    demand is per (kernel, mutant, instance), over the d's of the table.)"""
    hit = set()
    for kind, mode, d, rows, inst in _maths():
        if inst is None or rows != 67:
            continue
        VEC, NCHUNK = inst
        for mutant in MUTANTS[kind]:
            if _run(kind, mode, d, rows, inst, mutant) >= 2.0:
                hit.add((kind, mutant, inst))
            else:
                assert d <= (NCHUNK - 1) * R.RL * VEC or d in (1, 4), (kind, mode, d, inst, mutant)
    for kind, mutants in MUTANTS.items():                         # every mutant was shown at every instance
        for mutant in mutants:
            assert {i for k, m, i in hit if (k, m) == (kind, mutant)} == R.ALL_INSTANCES, (kind, mutant)


def test_a_source_read_with_the_gradient_stride_exceeds_the_bound():
    for d, inst in ((64, (4, 1)), (20, (1, 4))):
        f = R.fuse_inputs(67, d, "fuse", d, 0)
        flat = np.zeros(67 * (d + 4), dtype=np.float32)           # the source lives at ld = d + 4, the mutant walks it with dOut's ld = d
        flat.reshape(67, d + 4)[:, :d] = f.srcs[0]
        wrong = (flat[:67 * d].reshape(67, d), None, f.srcs[2])
        assert _run("fuse_bwd", "source", d, 67, inst, bases=wrong) >= 2.0
        assert _run("fuse_bwd", "source", d, 67, inst, bases=f.srcs) <= 0.5


def test_a_row_stride_one_block_short_exceeds_the_bound():
    """stride nvb 16 - 16: every row is still visited, the last block's rows (and what follows them) twice - invisible where a pass
    overwrites, caught where it accumulates: the accumulate mode of the backward, the partial sums of the paired forward"""
    for d, inst in ((64, (4, 1)), (20, (1, 4))):
        count = R.visits(R.BIG_ROWS, R.MAX_BLOCKS, R.MAX_BLOCKS - 1)
        assert _run("fuse_bwd", "accumulate", d, R.BIG_ROWS, inst, count=count) >= 2.0
        assert _run("fuse_bwd", "accumulate", d, R.BIG_ROWS, inst, count=R.visits(R.BIG_ROWS, R.MAX_BLOCKS)) <= 0.5
        f = R.fuse_inputs(R.BIG_ROWS, d, "fuse", d, 0)
        want, bound = R.multi_sumsq(f.norms[:2], inst[0] * inst[1], 2 * 2)
        twice = sum(float((x.astype(np.float64) ** 2 * count[:, None]).sum()) for x in f.norms[:2])
        assert abs(twice - want) >= 2.0 * bound
    assert (R.visits(16, 1, 0 + 1) == 1).all()                    # (one block: no stride is taken)


def test_sumsq_mutant_exceeds_the_bound():
    for fc in R.flat_cases():
        if fc.entry == "sumsq":
            X = R.mixed(fc.rows, fc.d, "sumsq", fc.rows)
            blocks = R.sumsq_blocks(X.size)
            want, bound = R.sumsq(X, 0.5, None, blocks)
            assert abs(float(R.emu_sumsq(X, 0.5, None, blocks, "no_last_step")) - want) >= 2.0 * bound


# ------------------------------------------------------------------------------------------------------------------------------------
# why this yardstick: the per-tensor maximum hides a row
# ------------------------------------------------------------------------------------------------------------------------------------
def test_an_error_the_max_normalised_rel_err_passes_fails_the_bound():
    """test_fuse_mean_normalize_add zeroes row 5 of a normalised term: its gradient is rate 1e12 g ~ 3e12, and max |a - b| / max |b| < 2e-5
    then admits an error of 6e7 anywhere else in the tensor. A gradient wrong by 1.0 in a row that is not clamped passes that expression
    and is several orders of magnitude outside the per-element bound."""
    rng = np.random.default_rng(65)
    rows, d = 203, 64
    x = rng.standard_normal((rows, d)).astype(np.float32)
    x[5] = 0.0
    G = rng.standard_normal((rows, d)).astype(np.float32)
    (want, bound), = R.fuse_bwd(G, [x], [2.8], 4, [None], 0, 0.0)
    assert np.abs(want[5]).max() > 1e12 and np.abs(np.delete(want, 5, axis=0)).max() < 10
    dev = want.copy()
    dev[7, 3] += 1.0

    def rel_err(a, b):                                            # tests/test_gpu_ops.py
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)

    assert rel_err(dev, want) < 2e-5                              # the old check passes
    assert np.abs(dev - want)[7, 3] > 1e4 * bound[7, 3]           # the new one does not, by far
    assert (np.abs(want.astype(np.float32) - want) <= bound).all()    # while the correctly rounded result passes it everywhere
