"""GPU: the BPR + prune loss kernels of llmrec_amd/csrc/bpr.hip through the C ABI (llmrec_amd._lib with ops.BprProblem), element by
element against the fp64 reference and the per-element bounds of tests/_bpr_ref.py (tests/test_bpr_ref_cpu.py checks that yardstick without
a device). The reference decides the keep mask, never the device. Tables are views of NaN-filled allocations (tests._eval_ref.Table);
targets, `saved`, the loss values, the gather blocks and rows3 are views inside sentinel-filled buffers whose surroundings - the columns
between d and ld, the rows no sample reaches, the slots beyond n_valid - must keep their bits. Targets start from non-zero contents.
Beside the bounds: the relations that hold bit for bit by construction (the scalar rows against the float4 rows, a shared target against
the members' launches in the contract's order, a repeated call, zero_rows) and the refusals, which write nothing."""
import numpy as np
import pytest
import torch

from tests import _bpr_ref as R
from tests._eval_ref import GUARD, Table

pytestmark = pytest.mark.gpu

DEV = "cuda"
assert GUARD == R.GUARD
WORST = {}                                                       # group -> the worst error / bound seen by this process
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------------------------------
# the calls (also made, with made-up addresses, by tests/test_bpr_ref_cpu.py for the refusals that return before any HIP call)
# ------------------------------------------------------------------------------------------------------------------------------------
def _problems(probs):
    from llmrec_amd import ops as O
    arr = (O.BprProblem * max(len(probs), 1))()
    for q, p in zip(arr, probs):
        (q.Eu, q.ldu), (q.Ei, q.ldi), (q.dEu, q.lddu), (q.dEi, q.lddi) = p["Eu"], p["Ei"], p.get("dEu", (None, 0)), p.get("dEi", (None, 0))
        q.g_mf, q.g_emb = p.get("g_mf", 0.0), p.get("g_emb", 0.0)
    return arr


def call(entry, probs=(), n_problems=None, d=0, users=None, pos=None, neg=None, B_max=0, n_valid=None, remember=1.0, decay=0.0, flag=1.0,
         out=None, saved=None, plan=None, grads2=None, rows3=None, phase=1, gather_block=None, gathered=None, n_ranks=1, rank_stride=0,
         my_rank=0, global_m=None, global_B=0, my_offset=0, scores_only=0, stream=None):
    """one call of `entry` -> the status. probs: dicts Eu / Ei / dEu / dEi -> (address, ld), g_mf, g_emb; everything else addresses or numbers"""
    from llmrec_amd import _lib
    n = len(probs) if n_problems is None else n_problems
    idx = (users, pos, neg)
    one = probs[0] if probs else {}
    flat = lambda *names: tuple(x for nm in names for x in one.get(nm, (None, 0)))
    if entry == "llmrec_bpr_prune_fwd_f32":
        args = flat("Eu", "Ei") + (d,) + idx + (B_max, n_valid, remember, decay, flag, out, saved, stream)
    elif entry == "llmrec_bpr_prune_fwd_sharded_f32":
        args = flat("Eu", "Ei") + (d,) + idx + (B_max, remember, decay, flag, global_m, global_B, my_offset, scores_only, out, saved, stream)
    elif entry == "llmrec_bpr_multi_fwd_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, remember, decay, flag, out, saved, stream)
    elif entry == "llmrec_bpr_multi_fwd_sharded_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, remember, decay, flag, phase, gather_block, gathered, n_ranks, rank_stride, my_rank,
                                                 out, saved, stream)
    elif entry == "llmrec_bpr_scatter_plan":
        args = idx + (B_max, n_valid, plan, stream)
    elif entry == "llmrec_bpr_multi_bwd_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, decay, flag, saved, plan, stream)
    elif entry == "llmrec_bpr_multi_scores_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, saved, None, stream)
    elif entry == "llmrec_bpr_multi_select_bwd_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, remember, decay, flag, saved, None, None, None, plan, stream)
    elif entry == "llmrec_bpr_multi_losses_f32":
        args = (n, B_max, n_valid, remember, decay, flag, out, saved, stream)
    elif entry == "llmrec_bpr_multi_zero_rows_f32":
        args = (n, _problems(probs), d) + idx + (B_max, n_valid, stream)
    elif entry == "llmrec_bpr_prune_bwd_f32":
        args = flat("Eu", "Ei") + (d,) + idx + (B_max, n_valid, decay, flag, saved, grads2) + flat("dEu", "dEi") + (plan, stream)
    elif entry == "llmrec_bpr_prune_bwd_rows_f32":
        args = flat("Eu", "Ei") + (d,) + idx + (B_max, n_valid, decay, flag, saved, grads2, rows3, stream)
    else:
        raise KeyError(entry)
    return _lib._invoke(entry, args)


def ok(status):
    from llmrec_amd import _lib
    assert status == 0, "status %d: %s" % (status, _lib.load().llmrec_last_error().decode())


# ------------------------------------------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """a float32 view [rows, cols] (row stride ld, first column col0) inside a sentinel-filled buffer, holding `init` before the calls"""

    def __init__(self, rows, cols, spec=None, init=None):
        ld, col0, mod = spec or (cols, 0, 0)
        ld = max(ld, cols + col0)
        self.buf = torch.full((2 * GUARD + rows * ld,), R.SENTINEL, dtype=torch.float32, device=DEV)
        self.v = torch.as_strided(self.buf, (rows, cols), (ld, 1), GUARD + col0)
        assert self.v.data_ptr() % 16 == mod
        idx = GUARD + col0 + torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        self.ld = ld
        if init is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=f32)).to(DEV))

    @property
    def p(self):
        return (self.v.data_ptr(), self.ld)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        """the view's contents, after checking that nothing around it was written"""
        assert bool((self.buf[self.outside] == R.SENTINEL).all()), "something wrote outside the view"
        return self.v.cpu().numpy().copy()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class Rank:
    """one rank's buffers of a case"""

    def __init__(self, inp, r, tables):
        case = inp.case
        self.case, self.r, self.B, self.n = case, r, case.B[r], case.valid(r)
        B, P, d = self.B, case.P, case.d
        self.idx = [_dev(a, torch.int64) for a in inp.idx[r]]
        self.nv = None if case.n_valid[r] is None else torch.tensor([case.n_valid[r]], dtype=torch.int32, device=DEV)
        self.saved = Out(P, R.saved_floats(B))
        self.out = Out(P, 2)
        self.plan = torch.zeros(max(R.plan_words(B), 1), dtype=torch.int64, device=DEV)
        self.tu = {g: Out(case.n_users, d, R.layout_spec(self._lay("tu", g, 2), d), inp.init_u[g]) for g in inp.init_u}
        self.ti = {g: Out(case.n_items, d, R.layout_spec(self._lay("ti", g, 3), d), inp.init_i[g]) for g in inp.init_i}
        self.probs = [dict(Eu=(tables[j][0].t.data_ptr(), tables[j][0].ld), Ei=(tables[j][1].t.data_ptr(), tables[j][1].ld),
                           dEu=self.tu[p.tu].p, dEi=self.ti[p.ti].p, g_mf=p.g_mf, g_emb=p.g_emb) for j, p in enumerate(case.probs)]
        self.common = dict(probs=self.probs, d=d, users=self.idx[0].data_ptr(), pos=self.idx[1].data_ptr(), neg=self.idx[2].data_ptr(), B_max=B,
                           n_valid=self.nv.data_ptr() if self.nv is not None else None, remember=inp.remember, decay=case.decay, flag=case.flag,
                           out=self.out.ptr, saved=self.saved.ptr, plan=self.plan.data_ptr())

    def _lay(self, field, g, op):
        lays = {p.lay[op] for p in self.case.probs if getattr(p, field) == g}
        assert len(lays) == 1, "problems that share a target share its layout"
        return lays.pop()

    def go(self, entry, **kw):
        ok(call(entry, **{**self.common, **kw}))

    def read_saved(self, got, selected, sums_written=False):
        """the `saved` slots into got; what lies beyond n_valid or was not written yet must be what the contract says"""
        n, B, P = self.n, self.B, self.case.P
        flat = self.saved.get()
        sv = [R.Saved(flat[j], B) for j in range(P)]
        for name in ("m", "nu", "np", "nq"):
            got[name] = np.stack([getattr(s, name)[:n] for s in sv])
            assert all((getattr(s, name)[n:] == R.SENTINEL).all() for s in sv), "a score slot beyond n_valid was written"
        assert all((s.tail == R.SENTINEL).all() for s in sv)
        if not selected:
            got["sg"] = np.stack([s.sg[:n] for s in sv])
            assert all((s.sg[n:] == R.SENTINEL).all() and (s.coef == R.SENTINEL).all() and (sums_written or (s.S == R.SENTINEL).all()) for s in sv)
            return
        got["coef"], got["kept_m"] = np.stack([s.coef[:n] for s in sv]), np.stack([s.sg[:n] for s in sv])
        assert all((s.coef[n:] == 0).all() and (s.sg[n:] == 0).all() for s in sv), "beyond n_valid: coefficient and kept value are 0"
        got["S"] = np.stack([s.S for s in sv])
        got["k_saved"] = [float(s.k) for s in sv]

    def read_targets(self, got):
        for g, o in self.tu.items():
            got["dEu%d" % g] = o.get()
        for g, o in self.ti.items():
            got["dEi%d" % g] = o.get()

    def read_out(self, got):
        o = self.out.get()
        got["mf"], got["emb"] = o[:, 0], o[:, 1]


def _tables(inp):
    case = inp.case
    return [(Table("Eu%d" % j, inp.Eu[j], *_spec(case, j, 0), DEV), Table("Ei%d" % j, inp.Ei[j], *_spec(case, j, 1), DEV)) for j in range(case.P)]


def _spec(case, j, op):
    ld, col0, mod = R.layout_spec(case.probs[j].lay[op], case.d)
    return max(ld, case.d + col0), col0, mod


def run(case, inp=None):
    """the case's flow on the device -> (inputs, per rank what the device holds: reference()'s names -> arrays)"""
    inp = inp or R.inputs(case)
    tables = _tables(inp)
    ranks = [Rank(inp, r, tables) for r in range(len(case.B))]
    gots = [{} for _ in ranks]
    fwd = {"prune": "llmrec_bpr_prune_fwd_f32", "rows": "llmrec_bpr_prune_fwd_f32", "multi": "llmrec_bpr_multi_fwd_f32",
           "zero": "llmrec_bpr_multi_fwd_f32"}
    grads2 = torch.tensor([case.probs[0].g_mf, case.probs[0].g_emb], dtype=torch.float32, device=DEV)
    if case.flow in fwd:
        rk, got = ranks[0], gots[0]
        rk.go(fwd[case.flow])
        rk.read_saved(got, True); rk.read_out(got)
    elif case.flow == "fused":
        rk, got = ranks[0], gots[0]
        rk.go("llmrec_bpr_multi_scores_f32")
        rk.read_saved(got, False)                                 # m, sigmoid(-x) and the norms right after the scores launch
        rk.go("llmrec_bpr_scatter_plan")
        rk.go("llmrec_bpr_multi_select_bwd_f32")
        rk.go("llmrec_bpr_multi_losses_f32")
        rk.read_saved(got, True); rk.read_out(got)
    elif case.flow == "sharded":
        P, cap = case.P, case.B[0]
        stride = R.gather_floats(P, cap) + 3                      # (a stride above the minimum)
        gathered = Out(len(ranks), stride)
        for r, rk in enumerate(ranks):
            block = Out(1, R.gather_floats(P, cap))
            rk.go("llmrec_bpr_multi_fwd_sharded_f32", phase=1, gather_block=block.ptr)
            b = block.get()[0]
            rk.read_saved(gots[r], False, sums_written=True)      # (phase 1 sums the local norms for the block)
            gots[r]["block"] = b
            gathered.v[r, :len(b)] = torch.from_numpy(b).to(DEV)
        for r, rk in enumerate(ranks):
            rk.go("llmrec_bpr_multi_fwd_sharded_f32", phase=2, gathered=gathered.ptr, n_ranks=len(ranks), rank_stride=stride, my_rank=r)
            rk.read_saved(gots[r], True); rk.read_out(gots[r])
        gathered.get()
    elif case.flow == "prune_sharded":
        ms = []
        for r, rk in enumerate(ranks):
            rk.go("llmrec_bpr_prune_fwd_sharded_f32", scores_only=1)
            rk.read_saved(gots[r], False)
            ms.append(gots[r]["m"][0])
        gm = Out(1, sum(case.B), init=np.concatenate(ms)[None])
        for r, rk in enumerate(ranks):
            rk.go("llmrec_bpr_prune_fwd_sharded_f32", scores_only=0, global_m=gm.ptr, global_B=sum(case.B), my_offset=sum(case.B[:r]))
            rk.read_saved(gots[r], True); rk.read_out(gots[r])
        gm.get()
    elif case.flow == "rows_big":                                 # the backward kernel alone: `saved` comes from the reference
        rk, ref = ranks[0], R.reference(inp)[0]
        flat = np.full((1, R.saved_floats(rk.B)), R.SENTINEL, dtype=f32)
        sv = R.Saved(flat[0], rk.B)
        sv.coef[:] = 0
        sv.coef[:rk.n] = ref["coef"][0][0].astype(f32)
        sv.S[:] = ref["S"][0][0].astype(f32)
        rk.saved.v.copy_(torch.from_numpy(flat).to(DEV))
    if case.flow in ("rows", "rows_big"):
        rk = ranks[0]
        rows3 = Out(3, rk.B * case.d)
        rk.go("llmrec_bpr_prune_bwd_rows_f32", grads2=grads2.data_ptr(), rows3=rows3.ptr)
        gots[0]["rows3"] = rows3.get().reshape(3, rk.B, case.d)
        rk.saved.get()
    else:
        for r, rk in enumerate(ranks):
            if case.flow != "fused":
                rk.go("llmrec_bpr_scatter_plan")
                rk.go("llmrec_bpr_prune_bwd_f32" if case.flow in ("prune", "prune_sharded") else "llmrec_bpr_multi_bwd_f32", grads2=grads2.data_ptr())
            rk.read_targets(gots[r])
    torch.cuda.synchronize()
    for t in tables:
        t[0].check(); t[1].check()
    return inp, gots, ranks


def check(case, inp, gots, ref):
    """everything the device holds against the reference, per element; returns group -> worst error / bound"""
    worst = {}
    for r, (got, want) in enumerate(zip(gots, ref)):
        n, k = want["n"], want["k"]
        if "coef" in got:
            assert got["k_saved"] == [float(k)] * case.P
            keep = got["coef"] != 0
            assert np.array_equal(keep, want["keep"]) and np.array_equal(got["kept_m"] != 0, want["keep"]), "the keep mask is the reference's"
        if "block" in got:                                        # the gather block: counts exact, +inf padding
            P, cap = case.P, case.B[r]
            b = got.pop("block")
            assert b[-1] == float(n)
            m = b[:P * cap].reshape(P, cap)
            assert np.isposinf(m[:, n:]).all() and np.array_equal(m[:, :n], got["m"])
            tail = b[P * cap:P * cap + 4 * P].reshape(P, 4)
            got["S_local"] = tail[:, :3]
            assert (tail[:, 3] == float(R.k_of(inp.remember, n))).all()
        if k == 0 and "mf" in got:
            assert np.isnan(got["mf"]).all()                      # k == 0: the empty mean
            for key, val in got.items():
                if key.startswith("dE") or key == "rows3":
                    assert np.isfinite(val).all(), key
        if "rows3" in got:
            assert not got["rows3"][:, n:].any(), "rows beyond n_valid are all-zero"
        for g, v in R.ratios(got, want).items():
            worst[g] = max(worst.get(g, 0.0), v)
    for g, v in worst.items():
        WORST[g] = max(WORST.get(g, 0.0), v)
    bad = {g: v for g, v in worst.items() if not v <= 1.0}
    assert not bad, (case.name, bad)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------------
CASES = R.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_family(ops, case):
    inp, gots, ranks = run(case)
    ref = R.reference(inp)
    worst = check(case, inp, gots, ref)
    print("\n[bpr yardstick] %-22s %s" % (case.name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if case.flow == "zero":                                       # zero_rows clears exactly the rows the batch touches
        rk = ranks[0]
        rk.go("llmrec_bpr_multi_zero_rows_f32")
        u, p, q = (a[:rk.n] for a in inp.idx[0])
        for outs, init, ids in ((rk.tu, inp.init_u, u), (rk.ti, inp.init_i, np.concatenate([p, q]))):
            for g, o in outs.items():
                now, touched = o.get(), np.isin(np.arange(len(init[g])), ids)
                assert not now[touched].any() and touched.any() and not touched.all()
                assert np.array_equal(now[~touched].view(np.int32), init[g][~touched].view(np.int32))


def test_worst_ratios_are_reported(ops):
    """what the table above left in WORST (pytest -s prints it: the figures of profiles/experiments/bpr_families.md)"""
    print("\n[bpr yardstick] worst device error / bound: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------------------------------------------
# relations that hold bit for bit by construction
# ------------------------------------------------------------------------------------------------------------------------------------
def _case(name):
    return [c for c in CASES if c.name == name][0]


def _bits(got):
    return {k: np.asarray(v).tobytes() for k, v in got.items() if k != "k_saved"}


@pytest.mark.parametrize("name", ["w64_bal", "w128_bal", "runs_step"])
def test_the_scalar_rows_equal_the_float4_rows(ops, name):
    """the same numbers behind an odd leading dimension of one target / a table 4 bytes off: the scalar instance adds the same records in the
    same order, element by element"""
    case = _case(name)
    inp = R.inputs(case)
    assert R.vec_of(case.d, case.probs)
    _, base, _ = run(case, inp)
    for lay in (("contig", "contig", "odd", "contig"), ("contig", "mis", "contig", "contig")):
        other = case._replace(probs=tuple(p._replace(lay=lay if (j == 0 or lay[2] == "odd") else p.lay) for j, p in enumerate(case.probs)))
        assert not R.vec_of(other.d, other.probs)
        _, got, _ = run(other, inp._replace(case=other))
        assert _bits(got[0]) == _bits(base[0]), lay


def test_a_shared_target_equals_its_members_one_after_the_other(ops):
    """the owner of a shared target adds, per row, problem 0's records and then problem 1's, in ascending slot: the bits of two launches
    that add problem 0 and then problem 1 into the same buffers"""
    case = _case("runs_p2")
    inp, both, _ = run(case)
    tables = _tables(inp)
    rk = Rank(inp, 0, tables)
    rk.go("llmrec_bpr_multi_fwd_f32")
    rk.go("llmrec_bpr_scatter_plan")
    for j in range(case.P):                                       # `saved` of problem j is where a one-problem call expects problem 0's
        rk.go("llmrec_bpr_multi_bwd_f32", probs=[rk.probs[j]], saved=rk.saved.ptr + 4 * j * R.saved_floats(rk.B))
    got = {}
    rk.read_targets(got)
    for key, val in got.items():
        assert np.array_equal(val, both[0][key]), key


@pytest.mark.parametrize("name", ["runs_bal", "p8", "sharded"])
def test_a_repeated_call_gives_the_same_bits(ops, name):
    case = _case(name)
    _, a, _ = run(case)
    _, b, _ = run(case)
    for x, y in zip(a, b):
        assert _bits(x) == _bits(y)


# ------------------------------------------------------------------------------------------------------------------------------------
# the refusals, with real buffers large enough for what is asked (tests/test_bpr_ref_cpu.py makes them, and the null tables, with made-up
# addresses where no device is present): the code of the restated rule, and nothing written
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    case = R._case("refuse", "multi", 16, R.MAX_B + 1, "bal", n_users=24, n_items=40)
    inp = R.inputs(case)
    rk = Rank(inp, 0, _tables(inp))
    stride = R.gather_floats(1, R.MAX_B + 1)
    block, gathered = Out(1, stride), Out(5, stride)
    gm = Out(1, R.SHARDED_PRUNE_CAP + 1)
    grads2 = torch.tensor([0.7, 1.0], dtype=torch.float32, device=DEV)
    extra = dict(gather_block=block.ptr, gathered=gathered.ptr, global_m=gm.ptr, grads2=grads2.data_ptr())
    status = lambda entry, **kw: call(entry, **{**rk.common, **extra, **kw})
    for entry in ("llmrec_bpr_prune_fwd_f32", "llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32",
                  "llmrec_bpr_multi_losses_f32", "llmrec_bpr_multi_fwd_sharded_f32", "llmrec_bpr_scatter_plan", "llmrec_bpr_prune_fwd_sharded_f32"):
        assert status(entry, scores_only=1) == R.refuse_cap(R.MAX_B + 1) == R.EUNSUPPORTED, entry
    small = dict(B_max=40)                                        # (the same buffers, a capacity the entries take)
    for entry in ("llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_bwd_f32", "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32",
                  "llmrec_bpr_multi_losses_f32", "llmrec_bpr_multi_zero_rows_f32", "llmrec_bpr_multi_fwd_sharded_f32"):
        assert status(entry, n_problems=0, **small) == R.refuse_n_problems(0) == R.EINVAL, entry
        assert status(entry, probs=rk.probs * 9, **small) == R.refuse_n_problems(9) == R.EINVAL, entry
    p = rk.probs[0]
    for entry, key in (("llmrec_bpr_prune_fwd_f32", "Eu"), ("llmrec_bpr_multi_fwd_f32", "Ei"), ("llmrec_bpr_prune_bwd_f32", "dEu"),
                       ("llmrec_bpr_prune_bwd_rows_f32", "Ei"), ("llmrec_bpr_multi_zero_rows_f32", "dEi"), ("llmrec_bpr_multi_bwd_f32", "dEu")):
        assert status(entry, probs=[dict(p, **{key: (p[key][0], case.d - 1)})], rows3=gathered.ptr, **small) == R.refuse_ld(case.d - 1, case.d) == R.EINVAL, entry
    assert status("llmrec_bpr_prune_bwd_f32", probs=[dict(p, dEi=p["dEu"])], **small) == R.refuse_same_target(1, 1) == R.EINVAL
    assert status("llmrec_bpr_multi_fwd_sharded_f32", phase=3, **small) == R.refuse_phase(3) == R.EINVAL
    need = R.gather_floats(1, 40)
    assert status("llmrec_bpr_multi_fwd_sharded_f32", phase=2, n_ranks=3, rank_stride=need - 1, **small) == R.refuse_rank_stride(need - 1, 1, 40) == R.EINVAL
    assert status("llmrec_bpr_multi_fwd_sharded_f32", phase=2, n_ranks=5, rank_stride=stride, B_max=R.MAX_B) == R.refuse_sharded_capacity(5, R.MAX_B) == R.EUNSUPPORTED
    assert status("llmrec_bpr_prune_fwd_sharded_f32", global_B=R.SHARDED_PRUNE_CAP + 1, **small) == R.refuse_global_batch(R.SHARDED_PRUNE_CAP + 1) == R.EUNSUPPORTED
    torch.cuda.synchronize()
    for o in [rk.saved, rk.out, block, gathered, gm] + list(rk.tu.values()) + list(rk.ti.values()):
        o.get()
    assert (rk.saved.get() == R.SENTINEL).all() and (rk.out.get() == R.SENTINEL).all() and (block.get() == R.SENTINEL).all()
    assert np.array_equal(rk.tu[0].get(), inp.init_u[0]) and np.array_equal(rk.ti[0].get(), inp.init_i[0]) and not rk.plan.any()
