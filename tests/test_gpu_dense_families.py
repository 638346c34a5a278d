"""GPU: every projection and weight-gradient kernel of llmrec_amd/csrc/dense.hip, through llmrec_amd.ops, against tests/_dense_ref.py
element by element: the fp32 forward kernels bit for bit against their fma chain, the fp32 gradient under (n + 6) u S, the bf16x3 kernels
under |dev - Y6| <= T_ACC S and |dev - Y64| <= (2^-20 (1 + 2^-6) + T_ACC) S (tests/test_dense_ref_cpu.py checks that yardstick and that
the table reaches every instantiation). Operands are views of NaN-filled allocations (tests._eval_ref.Table: a read outside a view shows
as NaN), outputs views inside sentinel-filled buffers whose surroundings are checked after every call, the unlisted rows of a listed dY
hold NaN. Beside the thresholds: the bit-exact relations the code promises (64- and 128-row units, the bf16x3 forward's three load modes,
repeated calls, the hand-over of the grouped entry to the multi launch, accumulate = fl(old + plain), the fall-back to the fp32 kernel,
the AdamW update inside the reduction) and the refusals."""
import numpy as np
import pytest
import torch

from tests import _dense_ref as R
from tests._eval_ref import GUARD, Table, layouts

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def tab(layout, src):
    """a NaN-guarded operand; "slice": the middle third of a [M, 3 d] buffer"""
    src = np.ascontiguousarray(src, dtype=np.float32)
    d = src.shape[1]
    if layout == "slice":
        return Table("slice", src, 3 * d, d, (4 * (GUARD + d)) % 16, DEV)
    t = layouts(d)[layout](src, DEV)
    assert (t.ld, t.col0, t.base_mod16) == R.layout_spec(layout, d)
    return t


def vec(v):
    """a NaN-guarded contiguous vector"""
    return Table("contig", np.asarray(v, dtype=np.float32).reshape(-1, 1), 1, 0, 0, DEV)


class Out:
    """an output view [rows, cols] (row stride ld, first column col0) inside a sentinel-filled buffer"""

    def __init__(self, rows, cols, ld=None, col0=0, init=None):
        ld = ld or cols
        self.buf = torch.full((2 * GUARD + rows * ld,), R.SENTINEL, dtype=torch.float32, device=DEV)
        self.v = torch.as_strided(self.buf, (rows, cols), (ld, 1), GUARD + col0)
        idx = GUARD + col0 + torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        if init is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(DEV))

    def fill(self, init=None):
        self.v.fill_(R.SENTINEL) if init is None else self.v.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(DEV))

    def get(self):
        """the view as numpy, after checking that nothing around it was written"""
        assert bool((self.buf[self.outside] == R.SENTINEL).all()), "something wrote outside the output view"
        return self.v.cpu().numpy().copy()

    def untouched(self):
        return bool((self.buf == R.SENTINEL).all())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ in bits, first at %s: %r != %r, max |diff| %.3g"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i], float(np.nanmax(np.abs(got.astype(np.float64) - want)))))


def within(got, want, bound, what):
    """element by element |got - want| <= bound (bound == 0 demands the exact value); returns the worst error / bound"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: %d non-finite results" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements over the bound, first at %s: got %r want %r err %.3g bound %.3g; worst err / bound %.3g"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i], err[i], bound[i],
                                float((err[bad] / np.maximum(bound[bad], 1e-300)).max())))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def tiled(fn, M):
    """a reference over the first PERIOD rows, repeated to M rows (R.long_rows operands)"""
    ref = fn(min(M, R.PERIOD))
    return ref[np.arange(M) % R.PERIOD] if M > R.PERIOD else ref


# ------------------------------------------------------------------------------------------------------------------------------------
# forward, plain entry: split-K and row mode
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.plain_cases(), ids=lambda c: "%s-%dx%dx%d" % (c.name, c.M, c.N, c.K))
def test_plain_forward_is_the_fma_chain(ops, case):
    X, W, b = R.plain_inputs(case)
    tx, tw = tab(case.xl, X), tab(case.wl, W)
    tb = vec(b) if b is not None else None
    wide = case.N % 2 == 1
    Y = Out(case.M, case.N, ld=case.N + 3 if wide else None, col0=2 if wide else 0)
    ops.linear_fwd_raw(tx.t, tw.t, tb.t[:, 0] if tb is not None else None, out=Y.v)
    want = tiled(lambda m: R.chain_fwd(X[:m], W, b, splitk=case.expect[3]), case.M)
    same_bits(Y.get(), want, case.name)
    for t in (tx, tw) + ((tb,) if tb is not None else ()):
        t.check()


# ------------------------------------------------------------------------------------------------------------------------------------
# forward, grouped entries
# ------------------------------------------------------------------------------------------------------------------------------------
class GroupedLaunch:
    """the operands of one table launch; the seven small problems are shared by the 64- and the 128-row-unit launch of a (N, mode)"""

    def __init__(self, case, shared=None):
        self.case, self.inp, self.tabs, self.outs = case, [], [], []
        for j, job in enumerate(case.jobs):
            X, W, b, bs = R.grouped_inputs(case, j)
            self.inp.append((X, W, b, bs))
            if shared is not None and j < len(shared.tabs):
                self.tabs.append(shared.tabs[j])
            else:
                self.tabs.append((tab(job.xl, X), tab(job.wl, W), vec(b) if b is not None else None, vec(bs) if bs is not None else None))
            self.outs.append(Out(job.M, case.N, ld=2 * case.N + 4 if job.y_slice else None, col0=case.N // 2 if job.y_slice else 0))

    def run(self, ops, precision):
        jobs = []
        for (tx, tw, tb, ts), out in zip(self.tabs, self.outs):
            out.fill()
            jobs.append((tx.t, tw.t, tb.t[:, 0] if tb is not None else None, out.v, ts.t[:, 0] if ts is not None else None))
        ops.linear_fwd_grouped(jobs, self.case.N, precision=precision)
        got = [o.get() for o in self.outs]
        for ts in self.tabs:
            for t in ts:
                if t is not None:
                    t.check()
        return got


_GROUPED = {(c.N, c.mode, c.rt): c for c in R.grouped_cases()}


@pytest.mark.parametrize("N,mode", sorted({(c.N, c.mode) for c in R.grouped_cases()}))
def test_grouped_forward(ops, N, mode, record_property):
    small = GroupedLaunch(_GROUPED[(N, mode, 1)])
    big = GroupedLaunch(_GROUPED[(N, mode, 2)], shared=small)
    refs = []
    for (X, W, b, bs), job in zip(big.inp, big.case.jobs):
        M = job.M
        cut = (lambda v, m: None if v is None else v[:m])
        refs.append(dict(chain=tiled(lambda m: R.chain_fwd(X[:m], W, b, cut(bs, m)), M), y6=tiled(lambda m: R.y6(X[:m], W, b, cut(bs, m)), M),
                         y64=tiled(lambda m: R.y64(X[:m], W, b, cut(bs, m)), M), S=tiled(lambda m: R.s_fwd(X[:m], W, b, cut(bs, m)), M)))
    worst = 0.0
    for precision in ("f32", "bf16x3"):
        assert R.grouped_expect(small.case, precision)[2] == 1 and R.grouped_expect(big.case, precision)[2] == 2
        got1, got2 = small.run(ops, precision), big.run(ops, precision)
        for j, (g, ref) in enumerate(zip(got2, refs)):
            what = "%s %s problem %d (M %d, K %d)" % (big.case.name, precision, j, big.case.jobs[j].M, big.case.jobs[j].K)
            if precision == "f32":
                same_bits(g, ref["chain"], what)
            else:
                worst = max(worst, within(g, ref["y6"], R.T_ACC["fwd"] * ref["S"], what + " against Y6"))
                within(g, ref["y64"], (R.DROPPED + R.T_ACC["fwd"]) * ref["S"], what + " against fp64")
            if j < len(got1):                                     # the same problem in 64-row units: the same bits
                same_bits(got1[j], g, what + ": 64-row units against 128-row units")
    record_property("worst_err_over_T_ACC_S", worst)
    print("[dense] grouped forward N %d mode %d: bf16x3 worst |dev - Y6| / (T_ACC S) = %.3g" % (N, mode, worst))


def test_bf16x3_forward_gives_the_same_bits_in_its_three_load_modes(ops):
    """the same values through MODE 3 (alone, K % 32 == 0), MODE 1 (beside a K = 36 problem) and MODE 0 (beside an odd-ld problem, itself in a
    padded layout); the fp32 kernel's three modes all equal the chain"""
    N, M, K = 48, 65, 96
    X, W, b = R.values("gauss", (M, K), "modes", "X"), R.values("gauss", (N, K), "modes", "W", scale=0.25), R.values("gauss", (N,), "modes", "b")
    X2, W2 = R.values("gauss", (17, 36), "modes", "X2"), R.values("gauss", (N, 36), "modes", "W2")
    tb = vec(b)
    results = {}
    for precision in ("bf16x3", "f32"):
        for mode, xl, companion in ((2, "contig", None), (1, "padded", "contig"), (0, "padded", "odd_ld")):
            tx, tw = tab(xl, X), tab(xl, W)
            Y, Y2 = Out(M, N), Out(17, N)
            jobs, desc = [(tx.t, tw.t, tb.t[:, 0], Y.v)], [R.FwdP(M, K, *[R.layout_spec(xl, K)[0]] * 2)]
            if companion:
                t2, w2 = tab(companion, X2), tab("contig", W2)
                jobs.append((t2.t, w2.t, None, Y2.v))
                desc.append(R.FwdP(17, 36, R.layout_spec(companion, 36)[0], 36))
            assert min(R.fwd_grouped(desc, N, precision)[3], 2) == mode
            ops.linear_fwd_grouped(jobs, N, precision=precision)
            results[(precision, mode)] = Y.get()
            tx.check(), tw.check()
    for mode in (0, 1):
        same_bits(results[("bf16x3", mode)], results[("bf16x3", 2)], "bf16x3 MODE %d against MODE 3" % mode)
    for mode in (0, 1, 2):
        same_bits(results[("f32", mode)], R.chain_fwd(X, W, b), "fp32 grouped MODE %d against the chain" % mode)
    plain = Out(M, N)                                             # ... and the plain entry's split-K kernel differs from the chain only by its four-way sum
    ops.linear_fwd_raw(tab("contig", X).t, tab("contig", W).t, tb.t[:, 0], out=plain.v)
    same_bits(plain.get(), R.chain_fwd(X, W, b, splitk=True), "plain split-K")


# ------------------------------------------------------------------------------------------------------------------------------------
# weight gradient, grouped entries
# ------------------------------------------------------------------------------------------------------------------------------------
def check_gradient(kind, got_w, got_b, pairs, weights, old_w, old_b, n_rows, what):
    """kind "f32": (n + 6) u S;  "bf16x3": T_ACC against the six-term value and T_ACC + the dropped terms against fp64; db is an fp32 sum
    in every kernel. pairs = the (dY, X) rows that count (float32 numpy). Returns the worst error / bound of dW."""
    S = R.s_dw(pairs, old_w)
    if kind == "f32":
        worst = within(got_w, R.dw64(pairs, old_w), R.bound_f32(n_rows) * S, what + " dW")
    else:
        worst = within(got_w, R.dw6(pairs, old_w), R.T_ACC["wgrad"] * S, what + " dW against the six-term value")
        within(got_w, R.dw64(pairs, old_w), (R.DROPPED + R.T_ACC["wgrad"]) * S, what + " dW against fp64")
    if got_b is not None:
        dys = [p[0] for p in pairs]
        within(got_b, R.db64(dys, weights, old_b), R.bound_f32(n_rows) * R.db64(dys, weights, old_b, absolute=True), what + " db")
    return worst


@pytest.mark.parametrize("case", R.wgrad_cases(), ids=lambda c: c.name)
def test_grouped_weight_gradient(ops, case, record_property):
    N, K = case.N, case.K
    inp = [R.wg_inputs(case, p) for p in range(len(case.Ms))]
    tabs = [(tab(case.layout, dY), tab("contig" if case.layout == "slice" else case.layout, X)) for dY, X in inp]
    for (ty, tx), q in zip(tabs, R.wg_problems(case)):
        assert (ty.ld, tx.ld, ty.base_mod16, tx.base_mod16) == (q.lddy, q.ldx, q.ymod, q.xmod)
    pairs = [(ty.t, tx.t) for ty, tx in tabs]
    old_w, old_b = R.values("gauss", (N, K), case.name, "oldW"), R.values("gauss", (1, N), case.name, "oldb")
    dW = Out(N, K, ld=K + 8 if case.wide_dw else None, col0=4 if case.wide_dw else 0)
    db = Out(1, N) if case.db else None

    def run(precision, accumulate):
        dW.fill(old_w), (db.fill(old_b) if db else None)
        ops.linear_wgrad_grouped(pairs, dW.v, db.v[0] if db else None, accumulate, precision=precision)
        return dW.get(), (db.get()[0] if db else None)

    got_w, got_b = run(case.kind, case.accumulate)
    n = sum(case.Ms)
    kernel_kind = "bf16x3" if "bf16x3" in case.expect else "f32"
    if case.expect == "memset":
        assert not got_w.any() and not got_b.any()
        return
    worst = check_gradient(kernel_kind, got_w, got_b, inp, None, old_w if case.accumulate else None, old_b[0] if case.accumulate else None,
                           n, case.name)
    record_property("worst_err_over_bound", worst)
    print("[dense] %s (%s): worst dW error / bound = %.3g" % (case.name, case.expect, worst))
    again_w, again_b = run(case.kind, case.accumulate)                                  # a repeated call: the same bits
    same_bits(again_w, got_w, case.name + " repeated")
    if case.accumulate:                                                                 # accumulate = fl(old + the plain result)
        plain_w, plain_b = run(case.kind, False)
        same_bits(got_w, old_w + plain_w, case.name + " accumulate against fl(old + plain)")
        if db:
            same_bits(got_b, old_b[0] + plain_b, case.name + " db accumulate against fl(old + plain)")
    if case.kind == "bf16x3" and kernel_kind == "f32":                                  # the fall-back runs the fp32 kernel itself
        f32_w, f32_b = run("f32", case.accumulate)
        same_bits(got_w, f32_w, case.name + " fall-back against the fp32 entry")
        if db:
            same_bits(got_b, f32_b, case.name + " fall-back db against the fp32 entry")
    if case.expect.startswith("linear_wgrad_bf16x3_v2"):                                # the hand-over: the one-target multi launch
        dW.fill(old_w), db.fill(old_b)
        ops.linear_wgrad_multi([(pairs, dW.v, db.v[0], case.accumulate)])
        same_bits(dW.get(), got_w, case.name + " hand-over against the multi entry")
        same_bits(db.get()[0], got_b, case.name + " hand-over db")
    for ty, tx in tabs:
        ty.check(), tx.check()


# ------------------------------------------------------------------------------------------------------------------------------------
# weight gradient, multi-target launch
# ------------------------------------------------------------------------------------------------------------------------------------
class MultiLaunch:
    def __init__(self, case, contiguous_dw=False):
        self.case, self.targets = case, []
        for ti, t in enumerate(case.targets):
            probs = []
            for pi, p in enumerate(t.problems):
                dY, X, w, ids = R.multi_inputs(case, ti, pi)
                ty, tx = tab("slice" if p.slice_dy else "contig", dY), tab("contig", X)
                tw = vec(w) if w is not None else None
                lst = None
                if ids is not None:                               # unlisted rows of dY are never read: poison them
                    mask = torch.ones(p.M, dtype=torch.bool, device=DEV)
                    mask[torch.from_numpy(ids.astype(np.int64)).to(DEV)] = False
                    ty.t[mask] = NAN
                    rl = torch.zeros(p.M + 32, dtype=torch.int32, device=DEV)
                    rl[:len(ids)] = torch.from_numpy(ids).to(DEV)
                    lst = (rl, torch.tensor([len(ids)], dtype=torch.int32, device=DEV), p.hint)
                    assert rl.data_ptr() % 64 == 0
                    dY, X, w = dY[ids], X[ids], (w[ids] if w is not None else None)
                probs.append(dict(ty=ty, tx=tx, tw=tw, lst=lst, ref=(dY, X), w=w))
            old_w, old_b = R.values("gauss", (case.N, t.K), case.name, ti, "oldW"), R.values("gauss", (1, case.N), case.name, ti, "oldb")
            wide = t.wide_dw and not contiguous_dw
            self.targets.append(dict(t=t, probs=probs, old_w=old_w, old_b=old_b, dW=Out(case.N, t.K, ld=t.K + 8 if wide else None, col0=4 if wide else 0),
                                     db=Out(1, case.N) if t.db else None))

    def args(self, accumulate=None):
        out = []
        for tg in self.targets:
            pairs = [(p["ty"].t, p["tx"].t, p["tw"].t[:, 0] if p["tw"] is not None else None, p["lst"]) for p in tg["probs"]]
            out.append((pairs, tg["dW"].v, tg["db"].v[0] if tg["db"] else None, tg["t"].accumulate if accumulate is None else accumulate))
        return out

    def run(self, ops, accumulate=None):
        for tg in self.targets:
            tg["dW"].fill(tg["old_w"]), (tg["db"].fill(tg["old_b"]) if tg["db"] else None)
        ops.linear_wgrad_multi(self.args(accumulate), block_budget=self.case.budget)
        return [(tg["dW"].get(), tg["db"].get()[0] if tg["db"] else None) for tg in self.targets]

    def check_operands(self):
        for tg in self.targets:
            for p in tg["probs"]:
                assert bool(torch.isnan(p["ty"].buf[p["ty"]._outside]).all())
                p["tx"].check()


@pytest.mark.parametrize("case", R.multi_cases(), ids=lambda c: c.name)
def test_multi_target_weight_gradient(ops, case, record_property):
    L = MultiLaunch(case)
    plan = R.wgrad_multi(R.multi_targets(case), case.N, case.budget)
    assert ops.linear_wgrad_multi_workspace(L.args(), case.budget) == plan["bytes"]
    got = L.run(ops)
    worst = 0.0
    for ti, (tg, (gw, gb)) in enumerate(zip(L.targets, got)):
        acc = tg["t"].accumulate
        pairs = [p["ref"] for p in tg["probs"]]
        n = sum(len(p[0]) for p in pairs)
        what = "%s target %d (K %d, %d rows)" % (case.name, ti, tg["t"].K, n)
        if n == 0 and not acc:
            assert not gw.any() and (gb is None or not gb.any()), what
            continue
        worst = max(worst, check_gradient("bf16x3", gw, gb, pairs, [p["w"] for p in tg["probs"]], tg["old_w"] if acc else None,
                                          tg["old_b"][0] if acc else None, n, what))
    record_property("worst_err_over_T_ACC_S", worst)
    print("[dense] %s (organisation %d): worst |dW - dW6| / (T_ACC S) = %.3g" % (case.name, case.version, worst))
    again = L.run(ops)
    plain = L.run(ops, accumulate=False)
    for ti, (tg, (gw, gb), (aw, ab), (pw, pb)) in enumerate(zip(L.targets, got, again, plain)):
        same_bits(aw, gw, "%s target %d repeated" % (case.name, ti))
        if tg["t"].accumulate:          # reduce_chunks_multi_kernel: "const float g = m.accumulate[t] ? (*o + s) : s;"
            same_bits(gw, tg["old_w"] + pw, "%s target %d accumulate against fl(old + plain)" % (case.name, ti))
            if gb is not None:
                same_bits(gb, tg["old_b"][0] + pb, "%s target %d db accumulate" % (case.name, ti))
    L.check_operands()


@pytest.mark.parametrize("case", R.adamw_cases(), ids=lambda c: c.name)
def test_adamw_inside_the_reduction_equals_the_separate_launches(ops, case):
    """llmrec_linear_wgrad_multi_adamw_bf16x3 at N = 128 and in organisation 1: gradients, parameters and both moments bit for bit those of
    llmrec_linear_wgrad_multi_bf16x3 followed by the optimizer's own update, over two steps"""
    L = MultiLaunch(case, contiguous_dw=True)

    def run(fused):
        lin = []
        for ti, tg in enumerate(L.targets):
            W = torch.from_numpy(R.values("gauss", (case.N, tg["t"].K), case.name, ti, "W", scale=0.05)).to(DEV)
            b = torch.from_numpy(R.values("gauss", (case.N,), case.name, ti, "b", scale=0.05)).to(DEV) if tg["t"].db else None
            W.grad = torch.zeros_like(W)
            if b is not None:
                b.grad = torch.zeros_like(b)
            lin.append((W, b))
        params = [p_ for W, b in lin for p_ in (W, b) if p_ is not None]
        opt = ops.FusedAdamW(params, lr=1e-3)
        for step in range(2):
            targets = [(pairs, W.grad, b.grad if b is not None else None, False) for (pairs, _, _, _), (W, b) in zip(L.args(), lin)]
            opt.advance()
            if fused:
                ops.linear_wgrad_multi(targets, update=(opt, lin))
            else:
                ops.linear_wgrad_multi(targets)
                opt.step_params(params)
        torch.cuda.synchronize()
        out = []
        for p_ in params:
            out += [p_.detach().cpu(), p_.grad.cpu(), opt.state[p_][0].cpu(), opt.state[p_][1].cpu()]
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) == 4 * sum(2 if tg["t"].db else 1 for tg in L.targets)
    for i, (x, y) in enumerate(zip(a, b)):
        same_bits(y.numpy(), x.numpy(), "%s tensor %d fused against separate" % (case.name, i))
    assert float(a[2].abs().max()) > 0 and float(a[3].abs().max()) > 0
    tg = L.targets[0]                                             # and the gradient it stored is the table's: under the threshold
    pairs = [p["ref"] for p in tg["probs"]]
    check_gradient("bf16x3", a[1].numpy(), a[5].numpy() if tg["t"].db else None, pairs, [p["w"] for p in tg["probs"]], None, None,
                   sum(len(p[0]) for p in pairs), case.name)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(ops):
    from llmrec_amd import _lib
    X = tab("contig", R.values("gauss", (33, 128), "ref", "X"))
    W129, W65 = tab("contig", R.values("gauss", (129, 128), "ref", "W")), tab("contig", R.values("gauss", (65, 128), "ref", "W65"))
    Y = Out(33, 129)
    with pytest.raises(RuntimeError, match="N = 129"):                                   # plain forward, N > 128
        ops.linear_fwd_raw(X.t, W129.t, None, out=Y.v)
    assert Y.untouched()
    Y = Out(33, 65)
    for precision in ("f32", "bf16x3"):                                                  # grouped forward, N > 64
        with pytest.raises(RuntimeError, match="N = 65"):
            ops.linear_fwd_grouped([(X.t, W65.t, None, Y.v)], 65, precision=precision)
    assert Y.untouched()
    dY = tab("contig", R.values("gauss", (33, 64), "ref", "dY"))
    w = vec(R.values("positive", (33,), "ref", "w"))
    rl = torch.zeros(33 + 32, dtype=torch.int32, device=DEV)
    rl[:33] = torch.arange(33, dtype=torch.int32, device=DEV)
    lst = (rl, torch.tensor([33], dtype=torch.int32, device=DEV), 0)
    dW, db = Out(64, 128), Out(1, 64)
    for pair in ((dY.t, X.t, w.t[:, 0]), (dY.t, X.t, None, lst)):                        # row weights / a row list with the fp32 entry
        with pytest.raises(RuntimeError):
            ops.linear_wgrad_grouped([pair], dW.v, db.v[0], False, precision="f32")
    X192 = tab("contig", R.values("gauss", (33, 192), "ref", "X192"))
    dW192 = Out(64, 192)
    for pair in ((dY.t, X192.t, w.t[:, 0]), (dY.t, X192.t, None, lst)):                  # ... and with organisation 1 (K = 192)
        with pytest.raises(RuntimeError):
            ops.linear_wgrad_multi([([pair], dW192.v, db.v[0], False)])
    arr, keep, N = ops._wgrad_targets([([(dY.t, X.t)], dW.v, db.v[0], False)])
    need = _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", 1, arr, 64)
    assert need == R.wgrad_multi_workspace_bytes((R.WgT(128, 128, (R.WgP(33, 64, 128),)),), 64)
    ws = torch.empty(need + 32, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match="workspace"):                                 # too small a workspace
        _lib.call("llmrec_linear_wgrad_multi_bf16x3", 1, arr, 64, ops._p(ws), need - 1, ops._stream())
    with pytest.raises(RuntimeError, match="workspace"):                                 # a misaligned one
        _lib.call("llmrec_linear_wgrad_multi_bf16x3", 1, arr, 64, ops._p(ws[4:]), need, ops._stream())
    garr = (ops.WgradProblem * 1)()
    garr[0].dY, garr[0].lddy, garr[0].X, garr[0].ldx, garr[0].M = dY.t.data_ptr(), 64, X192.t.data_ptr(), 192, 33
    gneed = R.wgrad_grouped([R.WgP(33, 64, 192)], 64, 192, "f32")["bytes"]
    for entry in ("llmrec_linear_wgrad_grouped_f32", "llmrec_linear_wgrad_grouped_bf16x3"):
        with pytest.raises(RuntimeError, match="workspace"):
            _lib.call(entry, 1, garr, 64, 192, ops._p(dW192.v), 192, ops._p(db.v[0]), 0, ops._p(ws), min(gneed - 1, ws.numel()), ops._stream())
    torch.cuda.synchronize()
    assert dW.untouched() and db.untouched() and dW192.untouched()
    _lib.call("llmrec_linear_wgrad_multi_bf16x3", 1, arr, 64, ops._p(ws), need, ops._stream())      # the same block with the buffer it asked for
    check_gradient("bf16x3", dW.get(), db.get()[0], [(dY.src.numpy(), X.src.numpy())], None, None, None, 33, "after the refusals")
