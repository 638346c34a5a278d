"""The eight-problem wide loss segment on the GPU (llmrec_bpr_scatter_plan_wide, llmrec_bpr_multi_{scores,select_bwd,losses}_wide_f32):
(1) the plan against the capped plan, word for word, (2) against its numpy restatement (tests/_plan_ref.py) beyond LLMREC_BPR_MAX_B,
(3) scores -> select + backward -> losses against the capped launches, bit for bit, (4) the selection beyond the cap against
tests/_select_ref.py per problem on crafted lists, (5) the gradients beyond the cap against the fp64 reference and per-element bounds of
tests/_bpr_ref.py, (6) graph capture. Batches draw from the 300 x d / 500 x d tables of tests/test_gpu_bpr_wide.py: every destination
row is hit dozens of times."""
import numpy as np
import pytest
import torch

from tests import _bpr_ref as R
from tests import _plan_ref as P
from tests import _select_ref as S
from tests import test_gpu_bpr_families as F
from tests.test_gpu_bpr_wide import VECTORS, U, I, batch, bits, crafted, same_bits, tables

pytestmark = pytest.mark.gpu

DEV = "cuda"
NP = 8
SENT = 12345.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def dev(a, dtype=torch.int64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


# --------------------------------------------------------------------------------------------
# 1., 2. the plan
# --------------------------------------------------------------------------------------------
def plan_wide(ops, idx, nv, prefill=True):
    B = idx[0].numel()
    plan = torch.zeros(max(ops.bpr_plan_words(B), 1), dtype=torch.int64, device=DEV)
    ws = ops.bpr_plan_wide_workspace(B, DEV)
    if prefill:
        ws.fill_(0xA5)                                                    # the entry point initialises what it reads
    return ops.bpr_scatter_plan_wide(*idx, nv, plan, ws)


@pytest.mark.parametrize("B", [1, 16, 17, 1126, 4096])
def test_plan_equals_the_capped_plan_word_for_word(ops, B):
    idx = tuple(x.to(DEV) for x in batch(B, seed=3))
    for n in (0, B - 3, B):
        nv = torch.tensor([n], dtype=torch.int32, device=DEV)
        want = ops.bpr_scatter_plan(*idx, nv, torch.zeros(5 * B, dtype=torch.int64, device=DEV))
        got = plan_wide(ops, idx, nv)
        assert got.numel() == 5 * B and torch.equal(got, want), (B, n)
    assert torch.equal(plan_wide(ops, idx, None), ops.bpr_scatter_plan(*idx, None, torch.zeros(5 * B, dtype=torch.int64, device=DEV)))


def _plan_batches(B):
    rng = np.random.default_rng(B)
    u, p, q = (x.numpy() for x in batch(B, seed=4))
    yield "tables", (u, p, q), None
    yield "hub", (u, np.full(B, 7, dtype=np.int64), q), None              # one item as every sample's positive: one run of B (+ its negatives)
    big = (rng.integers(0, 5_000_000, B), rng.integers(0, 5_000_000, B), rng.integers(0, 5_000_000, B))
    big[1][B // 2] = (1 << 24) + 1                                         # the high digits of the sort
    big[0][5] = (1 << 24) + 1
    yield "high_ids", big, None
    if B == 8200:
        yield "n_valid", (u, p, q), 4099


@pytest.mark.parametrize("B", [4097, 8200, 20011])
def test_plan_equals_the_numpy_restatement_beyond_the_cap(ops, B):
    for name, (u, p, q), n in _plan_batches(B):
        nv = None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV)
        got = plan_wide(ops, (dev(u), dev(p), dev(q)), nv).cpu().numpy()
        keys, runlen = P.split(got, B)
        want_keys, want_runlen = P.plan(u, p, q, B, n)
        assert np.array_equal(keys, want_keys), (name, np.flatnonzero(keys != want_keys)[:8])
        assert np.array_equal(runlen, want_runlen), (name, np.flatnonzero(runlen != want_runlen)[:8])
        if name == "hub":
            assert runlen[B:].max() >= B


# --------------------------------------------------------------------------------------------
# the eight problems of a step: problems 3 .. 7 share one dEu
# --------------------------------------------------------------------------------------------
class Step:
    def __init__(self, ops, B, d, n_valid, seed=0, n_prob=NP):
        self.ops, self.B, self.d, self.n_prob = ops, B, d, n_prob
        Eu, Ei = tables(d)
        self.Eu = [(Eu * (1.0 + 0.125 * j)).to(DEV) for j in range(n_prob)]
        self.Ei = [(Ei * (1.0 - 0.0625 * j)).to(DEV) for j in range(n_prob)]
        self.idx = tuple(x.to(DEV) for x in batch(B, seed=seed))
        self.nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=DEV)
        self.w_mf = [1.0, 0.5, 0.5] + [0.25] * (n_prob - 3)
        self.partial = dev(np.random.default_rng(5).random(100), torch.float32)
        self.reset()

    def reset(self):
        f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)
        n_prob, d = self.n_prob, self.d
        self.dEu = [f(U, d) for _ in range(min(n_prob, 4))]
        self.dEi = [f(I, d) for _ in range(n_prob)]
        self.saved = f(n_prob * self.ops.bpr_saved_floats(self.B))
        self.out, self.scal, self.running = f(n_prob, 2), f(4), torch.zeros(3, dtype=torch.float64, device=DEV)
        self.flag_u = torch.zeros(U, dtype=torch.uint8, device=DEV)
        self.flag_i = torch.zeros(I, dtype=torch.uint8, device=DEV)
        self.stamp = torch.tensor([41], dtype=torch.int32, device=DEV)
        self.adamw = torch.zeros(3, dtype=torch.float32, device=DEV)
        self.plan = torch.zeros(5 * self.B, dtype=torch.int64, device=DEV)
        self.probs = (self.ops.BprProblem * n_prob)()
        for j, q in enumerate(self.probs):
            du = self.dEu[min(j, 3)]
            q.Eu, q.ldu, q.Ei, q.ldi = self.Eu[j].data_ptr(), d, self.Ei[j].data_ptr(), d
            q.dEu, q.lddu, q.dEi, q.lddi = du.data_ptr(), d, self.dEi[j].data_ptr(), d
            q.g_mf, q.g_emb = self.w_mf[j], 1.0 if j == 0 else 0.0

    def state(self):
        return {"saved": self.saved, "out": self.out, "scal": self.scal, "running": self.running, "flag_u": self.flag_u, "flag_i": self.flag_i,
                "stamp": self.stamp, "adamw": self.adamw, **{"dEu%d" % j: t for j, t in enumerate(self.dEu)},
                **{"dEi%d" % j: t for j, t in enumerate(self.dEi)}}

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.state().items()}

    def workspaces(self):
        self.ws_plan = self.ops.bpr_plan_wide_workspace(self.B, DEV)
        self.ws_sel = self.ops.bpr_multi_wide_workspace(self.n_prob, self.B, DEV)
        self.ws_plan.fill_(0xA5); self.ws_sel.fill_(0xA5)

    def scores_wide(self):
        self.ops.bpr_multi_scores_wide(self.probs, self.d, *self.idx, self.nv, self.saved, self.stamp, self.adamw, 1e-3, 0.9, 0.999)

    def select_wide(self, remember):
        self.ops.bpr_multi_select_bwd_wide(self.probs, self.d, *self.idx, self.nv, remember, 1e-5, 64.0, self.saved, self.flag_u, self.flag_i,
                                           self.stamp, self.plan, self.ws_sel)

    def losses_wide(self, remember):
        self.ops.bpr_multi_losses_wide(self.n_prob, self.B, self.nv, remember, 1e-5, 64.0, self.out, self.saved, self.w_mf, self.partial,
                                       self.partial.numel(), 0.01, self.scal, self.running)

    def wide(self, remember, plan=True):
        if plan:
            self.ops.bpr_scatter_plan_wide(*self.idx, self.nv, self.plan, self.ws_plan)
        self.scores_wide(); self.select_wide(remember); self.losses_wide(remember)

    def capped(self, remember):
        o, p, c = self.ops, self.ops._p, self.ops._lib.call
        idx = [p(x) for x in self.idx]
        c("llmrec_bpr_scatter_plan", *idx, self.B, p(self.nv), p(self.plan), o._stream())
        c("llmrec_bpr_multi_scores_step_f32", self.n_prob, self.probs, self.d, *idx, self.B, p(self.nv), p(self.saved), p(self.stamp), p(self.adamw),
          1e-3, 0.9, 0.999, o._stream())
        c("llmrec_bpr_multi_select_bwd_f32", self.n_prob, self.probs, self.d, *idx, self.B, p(self.nv), remember, 1e-5, 64.0, p(self.saved),
          p(self.flag_u), p(self.flag_i), p(self.stamp), p(self.plan), o._stream())
        import ctypes
        c("llmrec_bpr_multi_losses_assemble_f32", self.n_prob, self.B, p(self.nv), remember, 1e-5, 64.0, p(self.out), p(self.saved),
          (ctypes.c_float * self.n_prob)(*self.w_mf), p(self.partial), self.partial.numel(), 0.01, p(self.scal), p(self.running), o._stream())


def equal_states(a, b):
    for k in a:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        if x.dtype == np.float32:
            assert same_bits(x, y), k
        elif x.dtype == np.float64:
            assert np.array_equal(x, y, equal_nan=True), k
        else:
            assert np.array_equal(x, y), k


# --------------------------------------------------------------------------------------------
# 3. the same bits where both segments exist
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remember", [0.29, 1.0])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("B", [35, 1126, 4096])
def test_wide_segment_equals_the_capped_launches_bit_for_bit(ops, B, d, remember):
    st = Step(ops, B, d, n_valid=B - 5)
    st.capped(remember)
    want = st.snapshot()
    st.reset(); st.workspaces()
    st.wide(remember)
    got = st.snapshot()
    equal_states(got, want)
    n, k = B - 5, S.k_of(remember, B - 5)
    saved = got["saved"].view(NP, -1)
    assert int(got["stamp"]) == 42 and got["adamw"].view(torch.int32)[0] == 1
    assert all(int((saved[j, :B] != 0).sum()) == k and float(saved[j, B + 3]) == k for j in range(NP))
    assert not saved[:, n:B].any()
    u, p, q = (x[:n].cpu() for x in st.idx)
    assert int((got["flag_u"] != 0).sum()) == len(set(u.tolist())) and int((got["flag_i"] != 0).sum()) == len(set(p.tolist()) | set(q.tolist()))
    untouched = np.setdiff1d(np.arange(U), u.numpy())
    g3 = got["dEu3"].cpu().numpy()
    assert (g3[untouched] == SENT).all()                                 # rows no sample touches keep the sentinel


def test_wide_segment_edges_equal_the_capped_launches(ops):
    """k == 0, k >= B and an empty batch; the loss values alone (scal4 == NULL) carry llmrec_bpr_multi_losses_f32's bits"""
    for n_valid, remember in ((30, 1e-5), (30, 1.0), (0, 0.29), (None, 1.0), (None, 1e-5)):
        st = Step(ops, 35, 64, n_valid=n_valid)
        st.capped(remember)
        want = st.snapshot()
        st.reset(); st.workspaces()
        st.wide(remember)
        equal_states(st.snapshot(), want)
    st = Step(ops, 1126, 64, n_valid=1100)
    st.capped(0.29)
    st.out.fill_(SENT)
    ops._lib.call("llmrec_bpr_multi_losses_f32", NP, st.B, ops._p(st.nv), 0.29, 1e-5, 64.0, ops._p(st.out), ops._p(st.saved), ops._stream())
    want = st.snapshot()
    st.out.fill_(SENT)
    ops.bpr_multi_losses_wide(NP, st.B, st.nv, 0.29, 1e-5, 64.0, st.out, st.saved)
    equal_states(st.snapshot(), want)


# --------------------------------------------------------------------------------------------
# 4. the selection is exact beyond the cap, per problem
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [VECTORS[:8], VECTORS[8:] + VECTORS[:2]], ids=["first8", "rest"])
@pytest.mark.parametrize("B", [4097, 8200])
def test_selection_is_exact_beyond_the_cap_per_problem(ops, B, names):
    """Every problem of a call gets ANOTHER crafted list in its m slots: a problem that read another one's histograms, state or eq[]
    would keep another set. A call has ONE remember rate and the crafted lists come with theirs, so there is one call per rate that
    occurs among `names`; in each the eight problems cycle through all of the lists (rotated, so that every list also meets the rates
    of the others), and every list meets its own rate in one of them."""
    lists = [(name,) + crafted(name, B) for name in names]
    rates = sorted({remember for _, _, remember in lists})
    for shift, remember in enumerate(rates):
        st = Step(ops, B, 64, n_valid=None, seed=9)
        st.workspaces()
        ops.bpr_scatter_plan_wide(*st.idx, None, st.plan, st.ws_plan)
        st.scores_wide()
        saved = st.saved.view(NP, -1)
        mine = [lists[(j + shift) % len(lists)] for j in range(NP)]
        assert {name for name, _, r in lists if r == remember} <= {name for name, _, _ in mine}
        for j, (name, m, _) in enumerate(mine):
            saved[j, B + 4:2 * B + 4] = torch.from_numpy(m).to(DEV)
        sg = saved[:, 2 * B + 4:3 * B + 4].cpu().numpy().copy()
        st.select_wide(remember)
        got = st.saved.view(NP, -1).cpu().numpy()
        k = S.k_of(remember, B)
        for j, (name, m, _) in enumerate(mine):
            keep, coef, kept_m, _ = S.expected(m, sg[j], remember)
            assert int(keep.sum()) == k, (name, j)
            assert np.array_equal(got[j, :B] != 0, keep), (name, j, remember)
            assert same_bits(got[j, :B], coef) and same_bits(got[j, 2 * B + 4:3 * B + 4], kept_m), (name, j, remember)
            assert got[j, B + 3] == np.float32(k)


# --------------------------------------------------------------------------------------------
# 5. gradients beyond the cap: the fp64 reference and the per-element bounds of tests/_bpr_ref.py
# --------------------------------------------------------------------------------------------
def _wide_case(B, d):
    """eight problems with the step's sharing pattern over 300 users / 500 items (the tables keep a few rows more, which no sample
    touches: they must keep their bits)"""
    case = R._case("wide%d_%d" % (B, d), "fused", d, B, "bal", P=8, tu=[0, 1, 2, 3, 3, 3, 3, 3], n_users=308, n_items=512, seed=2)
    inp = R.inputs(case)
    u, p, q = inp.idx[0]
    u %= 300; p %= 500; q %= 500
    inp.tie[0][:] = np.where(p == q, 1 << 40, (u * 512 + p) * 512 + q)     # (R._indices' classes, for the folded ids)
    return case, inp


def _run_wide_case(ops, case, inp):
    rk = F.Rank(inp, 0, F._tables(inp))
    c, B = rk.common, rk.B
    lib = ops._lib
    ws_plan, ws_sel = ops.bpr_plan_wide_workspace(B, DEV), ops.bpr_multi_wide_workspace(case.P, B, DEV)
    ws_plan.fill_(0xA5); ws_sel.fill_(0xA5)
    idx = (c["users"], c["pos"], c["neg"])
    probs = F._problems(c["probs"])
    F.ok(lib._invoke("llmrec_bpr_scatter_plan_wide", idx + (B, c["n_valid"], c["plan"], ws_plan.data_ptr(), ws_plan.numel(), None)))
    F.ok(lib._invoke("llmrec_bpr_multi_scores_wide_f32", (case.P, probs, case.d) + idx + (B, c["n_valid"], c["saved"], None, None, 0.0, 0.0, 0.0, None)))
    F.ok(lib._invoke("llmrec_bpr_multi_select_bwd_wide_f32", (case.P, probs, case.d) + idx + (B, c["n_valid"], c["remember"], c["decay"], c["flag"],
                                                                                                c["saved"], None, None, None, c["plan"],
                                                                                                ws_sel.data_ptr(), ws_sel.numel(), None)))
    F.ok(lib._invoke("llmrec_bpr_multi_losses_wide_f32", (case.P, B, c["n_valid"], c["remember"], c["decay"], c["flag"], c["out"], c["saved"], None,
                                                          None, 0, 0.0, None, None, None)))
    got = {}
    rk.read_saved(got, True); rk.read_out(got); rk.read_targets(got)
    return got


@pytest.mark.parametrize("B,d", [(4097, 64), (8200, 64), (4097, 128), (8200, 128)])
def test_gradients_beyond_the_cap_meet_the_fp64_bounds(ops, B, d):
    case, inp = _wide_case(B, d)
    ref = R.reference(inp)
    assert R.selection_margin(inp, ref) >= 4                              # the keep set is decided by the fp64 scores alone
    got = _run_wide_case(ops, case, inp)
    worst = F.check(case, inp, [dict(got)], ref)
    print("\n[bpr wide] %-14s %s" % (case.name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    again = _run_wide_case(ops, case, inp)
    assert set(again) == set(got)
    for key, val in got.items():
        assert np.array_equal(np.asarray(val), np.asarray(again[key]), equal_nan=True), key
    for g, init in inp.init_u.items():                                  # rows no sample touches keep their bits
        assert np.array_equal(got["dEu%d" % g][300:].view(np.int32), init[300:].view(np.int32))
    for g, init in inp.init_i.items():
        assert np.array_equal(got["dEi%d" % g][500:].view(np.int32), init[500:].view(np.int32))


# --------------------------------------------------------------------------------------------
# 6. graph capture: the plan is rebuilt inside the graph
# --------------------------------------------------------------------------------------------
def test_wide_segment_replays_from_a_captured_graph(ops):
    cap, remember = 5000, 0.29
    st = Step(ops, cap, 64, n_valid=cap, seed=80)
    st.workspaces()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        st.wide(remember)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.wide(remember)
    eager = Step(ops, cap, 64, n_valid=cap, seed=80)
    eager.workspaces()
    for n in (4200, 4999):
        for s in (st, eager):
            s.nv.fill_(n)
            for name, t in s.state().items():
                t.fill_(0 if name in ("running", "flag_u", "flag_i", "adamw") else (41 if name == "stamp" else SENT))
            s.plan.fill_(-1)                                             # a stale plan: the graph has to rebuild it
        g.replay()
        eager.wide(remember)
        got, want = st.snapshot(), eager.snapshot()
        equal_states(got, want)
        assert torch.equal(st.plan[:4 * cap + cap // 2], eager.plan[:4 * cap + cap // 2])
        keys, runlen = P.split(st.plan.cpu().numpy(), cap)
        u, p, q = (x.cpu().numpy() for x in st.idx)
        want_keys, want_runlen = P.plan(u, p, q, cap, n)
        assert np.array_equal(keys, want_keys) and np.array_equal(runlen, want_runlen)
        assert int((got["saved"].view(NP, -1)[0, :cap] != 0).sum()) == S.k_of(remember, n)
