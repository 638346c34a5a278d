"""GPU: every SpMM kernel family of llmrec_amd/csrc/spmm.hip - the seven float4 families and the three scalar ones, each as the plain,
weighted, masked and masked + weighted kernel, in every row bucket - against the float64 reference of tests/_spmm_ref.py, element by
element under its derived bound (tests/test_spmm_ref_cpu.py checks that yardstick). Every operand and output is a view inside a larger
buffer: X / Z / S guards (and the inactive X rows of a masked product) hold NaN, Y and its guards a finite sentinel; after a call every
guard must be bit-unchanged and every result finite. Beside the bound: the bit-exact relations the code promises (permuted plan = plain
plan, every column active = unmasked, a repeated call, grouped launch = single launches), the output row flags, and the other entry
points over this file (spmm_listed, spmm_rows_compact, the autograd drop-in through a misaligned view)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import _spmm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GR = 3                                # guard rows on either side of a view
FAMILY_CASES = {0: 75, 1: 69, 2: 102, 3: 66, 4: 71, 5: 80, 6: 67, 7: 86, 8: 123, 9: 83}      # the table, per family (sum: 822)
NAN = float("nan")


def _i32(t):
    return t.view(torch.int32)


class View:
    """rows x d floats at row stride ld inside a larger flat buffer; `odd_ld`: ld % 4 == 3, `off1`: the first element one float past a
    16-byte boundary (everything else 16-byte aligned, ld % 4 == 0)."""

    def __init__(self, rows, d, fill, odd_ld=False, off1=False, values=None):
        ld = (d + 3) // 4 * 4 + (7 if odd_ld else 8)
        off = GR * ld + 4
        off += (-off) % 4 + (1 if off1 else 0)
        self.buf = torch.full(((rows + 2 * GR) * ld + 16,), fill, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.v = self.buf.as_strided((rows, d), (ld, 1), off)
        self.ld = ld
        if values is not None:
            self.v.copy_(values if isinstance(values, torch.Tensor) else torch.from_numpy(np.array(values)))
        self.pristine = self.buf.clone()
        assert (self.v.data_ptr() % 16 == 0) == (not off1) and (ld % 4 == 0) == (not odd_ld)

    def unchanged(self):
        return torch.equal(_i32(self.buf), _i32(self.pristine))

    def guards_unchanged(self):
        """the bytes outside the view (the view itself is put back to its first contents for the comparison)"""
        keep = self.v.clone()
        self.v.copy_(self.pristine.as_strided(self.v.shape, self.v.stride(), self.v.storage_offset()))
        ok = self.unchanged()
        self.v.copy_(keep)
        return ok


class Env:
    def __init__(self):
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from llmrec_amd import _lib, ops
        self.ops, self.lib = ops, _lib
        rowptr, colidx, deg = R.graph()
        self.rowptr, self.colidx = torch.from_numpy(np.array(rowptr)).to(DEV), torch.from_numpy(np.array(colidx)).to(DEV)
        self.g = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in R.graph_inputs().items()}
        zr = R.graph_inputs()["z_rows"]
        self.z_flag = torch.from_numpy(np.where(zr, np.uint8(R.STAMP), np.uint8(5))).to(DEV)
        self.plans = {}
        for name, triple in R.TRIPLES.items():
            self.plans[(name, False)] = ops.SpmmPlan.build(self.rowptr, *triple)
            self.plans[(name, True)] = ops.SpmmPlan.build(self.rowptr, *triple, colidx=self.colidx, order_rows=True)
            assert self.plans[(name, True)].slot_row is not None and self.plans[(name, False)].slot_row is None
            b = R.row_buckets(name)
            pl = self.plans[(name, False)]
            assert (pl.n_wave, pl.n_block, pl.n_split) == tuple(int((b == k).sum()) for k in (1, 2, 3))
        self.views = {}

    def view(self, key, make):
        if key not in self.views:
            self.views[key] = make()
        return self.views[key]

    def operands(self, case):
        """(X, Z, S) views of a case; read-only, shared between the cases of one width"""
        inp = R.inputs(case)
        mis = case.misaligned

        def x():
            X = torch.from_numpy(np.array(inp["X"])).to(DEV)
            if inp["mask"] is not None:
                X[torch.from_numpy(inp["mask"] != R.STAMP).to(DEV)] = NAN               # promised zero, never read
            return View(R.N_COLS, case.d, NAN, odd_ld="ldx" in mis, off1="X" in mis, values=X)
        mask_name = {"mask_cs": "mask_some"}.get(case.kind, case.kind) if case.masked else None
        X = self.view(("X", case.d, mask_name, "ldx" in mis, "X" in mis), x)
        Z = S = None
        if case.op in ("z", "softmax_bwd"):
            Z = self.view(("Z", case.d, "Z" in mis), lambda: View(R.N_ROWS, case.d, NAN, off1="Z" in mis, values=inp["Z"]))
        if case.op == "softmax_bwd":
            S = self.view(("S", case.d, "S" in mis), lambda: View(R.N_ROWS, case.d, NAN, off1="S" in mis, values=inp["S"]))
        return X, Z, S


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.views.clear()


def _actual_family(case, X, Y, Z, S, partials):
    """the dispatch rule (tests/_spmm_ref.py's header) applied to the addresses and strides the call really gets"""
    w = case.width
    al = lambda t: t is None or t.data_ptr() % 16 == 0
    vec4 = w % 4 == 0 and X.ld % 4 == 0 and Y.ld % 4 == 0 and (Z is None or (Z.ld % 4 == 0 and al(Z.v))) and \
        (S is None or (S.ld % 4 == 0 and al(S.v))) and al(X.v) and al(Y.v) and al(partials)
    return R.family_of_width(w, vec4)


class Launch:
    """One llmrec_spmm_problem_t of a case over fresh output buffers (and everything it points to)."""

    def __init__(self, env, case, gate=None):
        ops = env.ops
        self.env, self.case = env, case
        inp = R.inputs(case)
        mis = case.misaligned
        self.X, self.Z, self.S = env.operands(case)
        y0 = inp["Z"] if case.op == "acc" else None                                   # Y += A X: Y holds the addend
        self.Y = View(R.N_ROWS, case.d, R.SENTINEL, odd_ld="ldy" in mis, off1="Y" in mis, values=y0)
        Zt = self.Y if case.op == "acc" else self.Z
        pl = self.plan = env.plans[(case.plan, case.permuted)]
        self.part = self.part_view = None
        if pl.n_seg:
            self.part = torch.full((pl.n_seg * case.d + 32,), R.SENTINEL, dtype=torch.float32, device=DEV)
            o = 16 + (1 if "partials" in mis else 0)
            self.part_view = self.part[o:o + pl.n_seg * case.d]
        g = env.g
        self.y_flag = self.mask = None
        if case.masked:
            self.mask = torch.from_numpy(np.array(inp["mask"])).to(DEV)
            self.y_flag = torch.full((R.N_ROWS + 32,), 200, dtype=torch.uint8, device=DEV)
        self.gate = gate
        self.epi = ops.SpmmEpilogueC(
            {"softmax": ops.EPI_SOFTMAX, "softmax_bwd": ops.EPI_SOFTMAX_BWD}.get(case.op, ops.EPI_NONE), float(case.alpha),
            Zt.v.data_ptr() if case.has_z else None, Zt.ld if case.has_z else 0, self.S.v.data_ptr() if self.S else None, self.S.ld if self.S else 0,
            g["ps"].data_ptr() if case.post else None, self.mask.data_ptr() if case.masked else None, R.STAMP if case.masked else 0,
            self.y_flag[16:].data_ptr() if case.masked else None, env.z_flag.data_ptr() if case.masked and case.has_z else None,
            gate.data_ptr() if gate is not None else None, None, 0)
        rp, ci = (pl.p_rowptr, pl.p_colidx) if case.permuted else (env.rowptr, env.colidx)
        self.pc = pl.c_struct()
        self.pr = ops.SpmmProblemC(R.N_ROWS, R.N_COLS, rp.data_ptr(), ci.data_ptr(), g["val"].data_ptr() if case.has_val else None,
                                   g["rs"].data_ptr() if case.has_rs else None, g["cs"].data_ptr() if case.has_cs else None,
                                   self.X.v.data_ptr(), self.X.ld, self.Y.v.data_ptr(), self.Y.ld, case.d, case.slice_width,
                                   ctypes.addressof(self.pc), ops._ptr(self.part_view), ctypes.addressof(self.epi))
        f = _actual_family(case, self.X, self.Y, Zt if case.has_z else None, self.S, self.part_view)
        assert f == R.family_and_variant(case)[0], (case.label(), f)

    def run(self):
        pr = self.pr
        self.env.lib.call("llmrec_spmm_f32", pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X, pr.ldx,
                          pr.Y, pr.ldy, pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, self.env.ops._stream())
        return self

    def result(self):
        """the output after the guard checks: (Y float32 numpy, y_row_flag numpy or None)"""
        torch.cuda.synchronize()
        c = self.case.label()
        for name, v in (("X", self.X), ("Z", self.Z), ("S", self.S)):
            assert v is None or v.unchanged(), "%s: the call wrote to %s or its guards" % (c, name)
        assert self.Y.guards_unchanged(), "%s: the call wrote outside Y" % c
        if self.part is not None:
            o = self.part_view.storage_offset()
            edge = torch.cat([self.part[:o], self.part[o + self.part_view.numel():]])
            assert bool((edge == R.SENTINEL).all()), "%s: the call wrote outside the partial sums" % c
        got = self.Y.v.contiguous().cpu().numpy()
        assert np.isfinite(got).all(), "%s: %d results are not finite (a guard or an inactive row was read)" % (c, int((~np.isfinite(got)).sum()))
        flag = None
        if self.y_flag is not None:
            f = self.y_flag.cpu().numpy()
            assert np.all(f[:16] == 200) and np.all(f[16 + R.N_ROWS:] == 200), "%s: the call wrote outside y_row_flag" % c
            flag = f[16:16 + R.N_ROWS]
        return got, flag


def _assert_within_bound(case, got, want, bound, relative):
    """|got - want| <= bound element by element (softmax: relative); returns the worst error / bound"""
    err = np.abs(got.astype(np.float64) - want)
    tol = bound * np.abs(want) if relative else bound
    bad = err > tol
    if bad.any():
        excess = np.where(bad, err - tol, -1.0)
        r, k = np.unravel_index(int(np.argmax(excess)), err.shape)
        raise AssertionError("%s: row %d (%d nnz, %s bucket), column %d: got %r, want %r, |error| %.3e > bound %.3e; %d elements in %d rows out of bound"
                             % (case.label(), r, int(R.graph()[2][r]), R.BUCKETS[int(R.row_buckets(case.plan)[r])], k, float(got[r, k]),
                                float(want[r, k]), err[r, k], tol[r, k], int(bad.sum()), int(bad.any(1).sum())))
    pos = tol > 0
    return float((err[pos] / tol[pos]).max()) if pos.any() else 0.0


def _assert_flags(case, got, flag):
    """y_row_flag: exact for lane-group and wavefront rows, set for every longer row, only 0 / the active value; unflagged rows are zero"""
    c = case.label()
    hit, bucket = R.row_hit(case), R.row_buckets(case.plan)
    assert set(np.unique(flag)) <= {0, R.STAMP}, c
    short = bucket <= 1
    wrong = np.nonzero(short & ((flag == R.STAMP) != hit))[0]
    assert wrong.size == 0, "%s: y_row_flag of rows %s (nnz %s) is not exact" % (c, wrong[:8], R.graph()[2][wrong[:8]])
    assert np.all(flag[~short] == R.STAMP), "%s: a block or split row is not flagged" % c
    if case.op != "softmax":                                                           # (the softmax of a zero row is 1 / d)
        assert np.all(got[flag == 0] == 0.0), "%s: an unflagged row is not all-zero" % c


@pytest.mark.parametrize("family", range(10))
def test_family_against_float64(env, family):
    cases = R.family_cases(family)
    results, worst, ran = {}, {}, 0
    for case in cases:
        run = Launch(env, case).run()
        got, flag = run.result()
        want, bound, relative = R.reference(case)
        v = R.family_and_variant(case)[1]
        worst[v] = max(worst.get(v, 0.0), _assert_within_bound(case, got, want, bound, relative))
        if case.masked:
            _assert_flags(case, got, flag)
        # a repeated call (the accumulating one from the same addend) gives the same bits
        again, flag2 = Launch(env, case).run().result()
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), "%s: a repeated call differs" % case.label()
        assert flag is None or np.array_equal(flag, flag2)
        if case.kind in ("mask_some", "mask_cs") and case.op != "softmax":
            # behind a row gate built from the rows that can be non-zero: gated-out rows are written as zeros unread
            gate = torch.from_numpy(np.where(R.row_hit(case), np.uint8(R.STAMP), np.uint8(9))).to(DEV)
            gated, _ = Launch(env, case, gate=gate).run().result()
            assert np.array_equal(got, gated), "%s: the gated product differs" % case.label()
        results[case] = got
        ran += 1
    n_perm = n_all = 0
    for case, got in results.items():
        if case.permuted:                                                              # permuted plan = plain plan, bit for bit
            twin = results[dataclasses.replace(case, permuted=False)]
            assert np.array_equal(got.view(np.int32), twin.view(np.int32)), "%s: differs from the plain plan" % case.label()
            n_perm += 1
        if case.kind == "mask_all":                                                    # every column active = unmasked (include/llmrec_hip.h:
            twin = results[dataclasses.replace(case, kind="pattern_rs")]               # "up to the sign of a zero")
            assert np.array_equal(got, twin), "%s: differs from the unmasked product" % case.label()
            n_all += 1
    print("family %d <%d,%d,%d>: %d cases, worst error / bound %s" % ((family,) + R.FAMILY_SHAPE[family] + (ran, {k: round(x, 4) for k, x in sorted(worst.items())})))
    assert ran == len(cases) == FAMILY_CASES[family] and sum(FAMILY_CASES.values()) == len(R.TABLE)
    assert n_perm == 6 and n_all >= 2 and set(worst) == set(R.VARIANTS)
    env.views.clear()


@pytest.mark.parametrize("family", range(7))
def test_grouped_launch_equals_the_single_launches(env, family):
    """llmrec_spmm_multi_f32 over 2, 3 and 4 problems of one family: the bits of separate llmrec_spmm_f32 calls (whose values the test
    above holds to the reference). Every plan of the table has split rows: spmm_finalize_multi_kernel runs in every group."""
    ops = env.ops
    ran = 0
    for variant, sizes in (("plain", (2, 3, 4)), ("weighted", (2, 3))):
        pool = [c for c in R.family_cases(family) if R.family_and_variant(c)[1] == variant]
        pool = pool[::max(1, len(pool) // 4)][:4]
        assert len(pool) == 4 and len({(c.plan, c.op, c.d) for c in pool}) > 1
        single = [Launch(env, c).run().result()[0] for c in pool]
        for n in sizes:
            group = [Launch(env, c) for c in pool[:n]]
            assert sum(1 for g in group if g.plan.n_split > 0) >= 2
            assert ops.spmm_multi([g.pr for g in group]), "the library refused a group of one family and variant"
            for g, want in zip(group, single):
                got, _ = g.result()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), "grouped launch of %d: %s differs from its single launch" % (n, g.case.label())
                ran += 1
    assert ran == 2 + 3 + 4 + 2 + 3
    env.views.clear()


def _pattern_csr(env):
    return env.ops.Csr(R.N_ROWS, R.N_COLS, env.rowptr, env.colidx, None, env.g["rs"], None, {})


def _listed_rows():
    deg = R.graph()[2]
    special = [int(np.nonzero(deg == n)[0][0]) for n in R.ROW_LENGTHS]
    return sorted(set(special) | {0, 1, R.N_ROWS - 1})


@pytest.mark.parametrize("d", [50, 64])
def test_spmm_listed_writes_exactly_the_listed_rows(env, d):
    """ops.spmm_listed at a scalar and a float4 width: the listed rows (every row length of the table) within the bound, every other
    row and every guard keeps the sentinel bit for bit."""
    case = R.Case(d, "pattern_rs", "none", False, "buckets")
    X = env.operands(case)[0]
    Y = View(R.N_ROWS, d, R.SENTINEL)
    rows = _listed_rows()
    env.ops.spmm_listed(_pattern_csr(env), X.v, torch.tensor(rows, dtype=torch.int64, device=DEV), Y.v)
    torch.cuda.synchronize()
    assert X.unchanged() and Y.guards_unchanged()
    got = Y.v.contiguous().cpu().numpy()
    other = np.setdiff1d(np.arange(R.N_ROWS), rows)
    assert np.array_equal(got[other].view(np.int32), np.full((other.size, d), R.SENTINEL, np.float32).view(np.int32))
    want, bound, relative = R.reference(case)
    assert np.isfinite(got).all()
    sel = np.zeros(R.N_ROWS, bool); sel[rows] = True
    _assert_within_bound(case, np.where(sel[:, None], got, want.astype(np.float32)), want, np.where(sel[:, None], bound, np.inf), relative)
    env.views.clear()


@pytest.mark.parametrize("d", [12, 20, 64, 68, 132, 15, 50])
def test_spmm_rows_compact_per_compiled_family(env, d):
    """ops.spmm_rows_compact at one width per compiled instance (five float4, two scalar): slot j holds listed row j within the bound,
    the slots past the device-side count are zero, the guards of the output block stay."""
    case = R.Case(d, "pattern_rs", "none", False, "buckets")
    assert R.family_of_width(d, d % 4 == 0) == {12: 0, 20: 1, 64: 2, 68: 3, 132: 4, 15: 7, 50: 8}[d]
    X = env.operands(case)[0]
    rows = _listed_rows()
    cap = len(rows) + 9
    lst = torch.full((cap,), -7, dtype=torch.int32, device=DEV)                         # (slots past the count are never read)
    lst[:len(rows)] = torch.tensor(rows, dtype=torch.int32, device=DEV)
    n = torch.tensor([len(rows)], dtype=torch.int32, device=DEV)
    out = View(cap, d, R.SENTINEL)
    env.ops.spmm_rows_compact(_pattern_csr(env), X.v, lst, n, out.v)
    torch.cuda.synchronize()
    assert X.unchanged() and out.guards_unchanged()
    got = out.v.contiguous().cpu().numpy()
    assert np.isfinite(got).all() and np.all(got[len(rows):] == 0.0)
    want, bound, relative = R.reference(case)
    err = np.abs(got[:len(rows)].astype(np.float64) - want[rows])
    bad = np.nonzero(err > bound[rows])
    assert bad[0].size == 0, "rows_compact d = %d: slot %d (row %d, %d nnz), column %d: |error| %.3e > bound %.3e" % (
        d, bad[0][0], rows[bad[0][0]], R.graph()[2][rows[bad[0][0]]], bad[1][0], err[bad[0][0], bad[1][0]], bound[rows][bad[0][0], bad[1][0]])
    env.views.clear()


@pytest.mark.parametrize("through_view", [False, True])
def test_autograd_drop_in_through_the_scalar_kernels(env, through_view):
    """ops.spmm forward + backward with general values at d = 50, and through big[:, 1:65] with the gradient handed in behind the same
    kind of view: the scalar weighted kernels (families 8) in both directions, each element under the linear bound."""
    ops = env.ops
    rowptr, colidx, deg = R.graph()
    gi = R.graph_inputs()
    rows = np.repeat(np.arange(R.N_ROWS), deg)
    op = ops.SparseOperand.from_coo(torch.from_numpy(rows).to(DEV), torch.from_numpy(colidx.astype(np.int64)).to(DEV),
                                    torch.from_numpy(np.array(gi["val"])).to(DEV), R.N_ROWS, R.N_COLS)
    assert op.fwd.val is not None and op.bwd.val is not None
    d = 64 if through_view else 50
    rng = np.random.default_rng(50 + d)
    Xn, Gn = rng.standard_normal((R.N_COLS, d)).astype(np.float32), rng.standard_normal((R.N_ROWS, d)).astype(np.float32)
    if through_view:
        big = torch.full((R.N_COLS, 70), NAN, device=DEV); big[:, 1:65] = torch.from_numpy(Xn).to(DEV); big.requires_grad_(True)
        gbig = torch.full((R.N_ROWS, 70), NAN, device=DEV); gbig[:, 1:65] = torch.from_numpy(Gn).to(DEV)
        X, G = big[:, 1:65], gbig[:, 1:65]
        assert X.data_ptr() % 16 != 0 and G.data_ptr() % 16 != 0
    else:
        big = torch.from_numpy(Xn).to(DEV).requires_grad_(True)
        X, G = big, torch.from_numpy(Gn).to(DEV)
    Y = ops.spmm(op, X)
    Y.backward(G)
    torch.cuda.synchronize()
    A = np.zeros((R.N_ROWS, R.N_COLS)); A[rows, colidx] = gi["val"].astype(np.float64)
    got_y = Y.detach().cpu().numpy()
    got_dx = big.grad.cpu().numpy()
    if through_view:
        assert np.all(got_dx[:, :1] == 0.0) and np.all(got_dx[:, 65:] == 0.0)
        got_dx = got_dx[:, 1:65]
    for name, got, want, bound in (("forward", got_y, A @ Xn.astype(np.float64), R.linear_bound(deg, np.abs(A) @ np.abs(Xn).astype(np.float64))),
                                   ("backward", got_dx, A.T @ Gn.astype(np.float64),
                                    R.linear_bound(np.bincount(colidx, minlength=R.N_COLS), np.abs(A).T @ np.abs(Gn).astype(np.float64)))):
        assert np.isfinite(got).all(), name
        err = np.abs(got.astype(np.float64) - want)
        bad = np.nonzero(err > bound)
        assert bad[0].size == 0, "%s d = %d: row %d column %d: |error| %.3e > bound %.3e (%d elements)" % (
            name, d, bad[0][0], bad[1][0], err[bad[0][0], bad[1][0]], bound[bad[0][0], bad[1][0]], bad[0].size)
