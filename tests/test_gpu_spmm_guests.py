"""GPU: guest blocks in the grouped SpMM launch (llmrec_spmm_multi_guest_f32). Each case runs the guest launch and then the separate
calls (llmrec_spmm_f32 per product + the guest's own entry point) from the same state and compares with torch.equal: every product's Y
(split rows through their finalize launch) and every guest output - the sampler's users / pos / neg / n_valid, step counter and ticket
after two consecutive calls; the plan's 3 B_max keys and run lengths and the reach flags; the loss values' out / saved / scal / epoch
sums. Groups of 1, 2 and 3 products, unweighted and weighted, d = 64 and a 448-wide operand in 64-column slices, a graph with empty rows
and a row in each of the wavefront / block / split buckets, batch capacities around the 16-key, 256- and 512-thread block edges.
A refused group launches nothing and leaves every buffer untouched. And the whole step: six steps with the guests against six with
every guest refused, eager and as a replayed graph of four steps - parameters, Adam moments, scal and the sampled batches bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_spmm_multi import _problem, _rand, _single
from tests.test_gpu_reproducible import datasets          # noqa: F401  (the nf_mid_lr dataset fixture)

DEV = "cuda"
SENTINEL = -7
B_CAPS = [1, 16, 17, 255, 256, 257, 1126]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def graphs(ops):
    """small: ~300 x 200, 2 000 edges. buckets: empty rows and rows in the lane-group, wavefront (> 32), block (> 128) and split (> 2048
    non-zeros at 64 columns) buckets."""
    rng = np.random.default_rng(21)
    U, I = 300, 200
    e = np.unique(rng.integers(0, U * I, size=2100))[:2000]
    small = ops.BipartiteGraph.from_edges(torch.from_numpy(e // I).to(DEV), torch.from_numpy(e % I).to(DEV), U, I)
    n_rows, n_cols = 90, 6000
    degs = rng.integers(0, 20, size=n_rows)
    for k, dg in enumerate([0, 0, 1, 32, 33, 128, 129, 2048, 2049, 5000]):
        degs[(k * 7 + 1) % n_rows] = dg
    rows = np.repeat(np.arange(n_rows), degs)
    cols = np.concatenate([rng.choice(n_cols, size=dg, replace=False) for dg in degs])
    buckets = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), n_rows, n_cols)
    pl = buckets.ui.fwd.plan_for(64)[1]
    assert pl.n_split > 0 and pl.n_seg > 0
    return {"small": small, "buckets": buckets}


@pytest.fixture(scope="module")
def sampler_world(ops):
    """(train CSR, users with train items, augmented pairs with and without filtered ones)"""
    rng = np.random.default_rng(77)
    n_users, n_items = 2600, 211
    exist = np.arange(1, n_users, 2)
    degs = np.zeros(n_users, dtype=np.int64)
    rows = {int(u): np.sort(rng.choice(n_items, size=int(rng.integers(1, 12)), replace=False)) for u in exist}
    for u, r in rows.items():
        degs[u] = len(r)
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    colidx = np.concatenate([rows[u] for u in sorted(rows)])
    csr = ops.Csr(n_users, n_items, torch.tensor(rowptr, dtype=torch.int32, device=DEV), torch.tensor(colidx, dtype=torch.int32, device=DEV),
                  None, None, None)
    aug = {"filtered": (rng.integers(-3, int(1.3 * n_items), size=n_users), rng.integers(-3, int(1.3 * n_items), size=n_users)),
           "all_kept": (rng.integers(0, n_items, size=n_users), rng.integers(0, n_items, size=n_users))}
    aug = {k: tuple(torch.tensor(x, dtype=torch.int64, device=DEV) for x in v) for k, v in aug.items()}
    return csr, torch.tensor(exist, dtype=torch.int64, device=DEV), n_items, aug


# ---- the three guests: state() -> fresh buffers; guest(state) -> descriptor; alone(state) -> the stand-alone call; outputs(state) ----------
class SamplerGuest:
    def __init__(self, ops, world, b_cap, kind):
        self.ops, (self.csr, self.exist, self.n_items, aug) = ops, world
        self.n_aug = b_cap // 11
        self.B = b_cap - self.n_aug
        self.ap, self.an = aug[kind] if self.n_aug else (None, None)
        self.calls = 2

    def state(self):
        n = self.B + self.n_aug + 9
        return {"users": torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV), "pos": torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV),
                "neg": torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV), "n_valid": torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV),
                "step": torch.tensor([2 ** 32 + 5], dtype=torch.int64, device=DEV), "ticket": torch.zeros(1, dtype=torch.int32, device=DEV)}

    def _args(self, s):
        return (2022 + self.B, s["step"], self.exist, self.n_items, self.csr, self.B, 0, self.B, self.n_aug, self.ap, self.an,
                s["users"], s["pos"], s["neg"], s["n_valid"], s["ticket"])

    def guest(self, s):
        return self.ops.guest_sampler(*self._args(s))

    def alone(self, s):
        self.ops.sample_batch_wide(*self._args(s))

    def check(self, s):
        assert int(s["ticket"]) == 0 and self.B <= int(s["n_valid"]) <= self.B + self.n_aug


class PlanGuest:
    def __init__(self, ops, graph, b_cap, short):
        self.ops, self.by_item, self.B = ops, graph.iu.fwd, b_cap
        rng = np.random.default_rng(300 + b_cap)
        n_users, n_items = self.by_item.n_cols, self.by_item.n_rows
        self.users = torch.tensor(rng.integers(0, min(n_users, 40), size=b_cap), dtype=torch.int64, device=DEV)       # (shared ids: runs)
        self.pos = torch.tensor(rng.integers(0, n_items, size=b_cap), dtype=torch.int64, device=DEV)
        self.neg = torch.tensor(rng.integers(0, n_items, size=b_cap), dtype=torch.int64, device=DEV)
        self.n_valid = torch.tensor([max(1, 2 * b_cap // 3) if short else b_cap], dtype=torch.int32, device=DEV)
        self.calls = 1

    def state(self):
        return {"plan": torch.full((3 * self.B + (3 * self.B + 1) // 2 + 1,), SENTINEL, dtype=torch.int64, device=DEV),
                "flags": torch.zeros(self.by_item.n_cols + 5, dtype=torch.uint8, device=DEV)}

    def _args(self, s):
        return (self.users, self.pos, self.neg, self.B, self.n_valid, s["plan"], self.by_item.n_cols, self.by_item.n_rows, self.by_item.rowptr,
                self.by_item.colidx, s["flags"])

    def guest(self, s):
        return self.ops.guest_plan_reach(*self._args(s))

    def alone(self, s):
        from llmrec_amd import _lib
        _lib.call("llmrec_bpr_scatter_plan_reach_mark", *[self.ops._p(a) if isinstance(a, torch.Tensor) else a for a in self._args(s)],
                  self.ops._stream())

    def check(self, s):
        nv = int(self.n_valid)
        assert bool(s["flags"][self.users[:nv]].all()) and not bool(s["flags"][self.by_item.n_cols:].any())
        keys = s["plan"][:self.B]
        assert bool((keys[:nv] >> 32 == torch.sort(self.users[:nv]).values).all())                  # the user side, sorted by id


class LossesGuest:
    def __init__(self, ops, b_cap, short):
        self.ops, self.B, self.n_prob = ops, b_cap, 8
        rng = np.random.default_rng(500 + b_cap)
        self.saved0 = _rand(rng, self.n_prob, 6 * b_cap + 8)
        self.saved0[:, b_cap + 4 + 2 * b_cap:] = self.saved0[:, b_cap + 4 + 2 * b_cap:].abs()       # the squared norms' columns
        self.partial = _rand(rng, 37).abs()
        self.scal0, self.sums0 = _rand(rng, 4), torch.tensor(rng.standard_normal(3), dtype=torch.float64, device=DEV)
        self.n_valid = torch.tensor([max(1, 2 * b_cap // 3) if short else b_cap], dtype=torch.int32, device=DEV)
        self.w = [0.5 + 0.1 * k for k in range(self.n_prob)]
        self.calls = 1

    def state(self):
        return {"out": torch.full((2 * self.n_prob,), float(SENTINEL), device=DEV), "saved": self.saved0.clone(), "scal": self.scal0.clone(),
                "sums": self.sums0.clone()}

    def guest(self, s):
        return self.ops.guest_losses(self.n_prob, self.B, self.n_valid, 0.7, 1e-3, 1024.0, s["out"], s["saved"], self.w, self.partial, 37, 0.25,
                                     s["scal"], s["sums"])

    def alone(self, s):
        from llmrec_amd import _lib
        p = self.ops._p
        w = (ctypes.c_float * self.n_prob)(*self.w)
        _lib.call("llmrec_bpr_multi_losses_assemble_f32", self.n_prob, self.B, p(self.n_valid), 0.7, 1e-3, 1024.0, p(s["out"]), p(s["saved"]), w,
                  p(self.partial), 37, 0.25, p(s["scal"]), p(s["sums"]), self.ops._stream())

    def check(self, s):
        assert not bool((s["out"] == float(SENTINEL)).any()) and not torch.equal(s["scal"], self.scal0)


def _same(a, b):
    if a.dtype in (torch.float32, torch.float64):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _specs(ops, g, rng, n, weighted, wide):
    """n products of one kernel instance over graph g: [(a, X, Y0, epilogue of Y or None)]"""
    U, I = g.n_users, g.n_items
    if weighted:                                                        # the transposed (col_scale-weighted) operands of the backward
        Z, S = _rand(rng, U, 64), torch.softmax(_rand(rng, U, 64), dim=-1)
        pool = [(g.iu.bwd, _rand(rng, I, 64), torch.zeros(U, 64, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX_BWD, 1 / 3, Z, S)),
                (g.iu.bwd, _rand(rng, I, 448 if wide else 64), _rand(rng, U, 448 if wide else 64), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y)),
                (g.ui.bwd, _rand(rng, U, 64), _rand(rng, I, 64), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y))]
    else:
        pool = [(g.ui.fwd, _rand(rng, I, 64), torch.zeros(U, 64, device=DEV), (lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX)) if n == 1 else None),
                (g.iu.fwd, _rand(rng, U, 448 if wide else 64), torch.zeros(I, 448 if wide else 64, device=DEV), None),
                (g.iu.fwd, _rand(rng, U, 64), torch.zeros(I, 64, device=DEV), None)]
    if wide and n == 1:
        return pool[1:2]
    return pool[:n]


def _run(ops, specs, guest, with_guest):
    outs, probs, keep = [], [], []
    for a, X, Y0, epi_of in specs:
        Y = Y0.clone()
        pr, k = _problem(ops, a, X, Y, epi_of(Y) if epi_of is not None else None)
        outs.append(Y); probs.append(pr); keep.append(k)
    s = guest.state()
    for c in range(guest.calls):
        if with_guest:
            assert ops.spmm_multi_guest(probs, guest.guest(s)), "the guest launch was refused"
        else:
            guest.alone(s)
            for pr in probs:
                _single(ops, pr)
    torch.cuda.synchronize()
    return outs, s


def _check(ops, specs, guest, what):
    want, s_want = _run(ops, specs, guest, with_guest=False)
    got, s_got = _run(ops, specs, guest, with_guest=True)
    for i, (w, g) in enumerate(zip(want, got)):
        assert _same(w, g), (what, "Y", i)
    for k in s_want:
        assert _same(s_want[k], s_got[k]), (what, k)
    guest.check(s_got)


@pytest.mark.parametrize("b_cap", B_CAPS)
def test_guest_launch_equals_the_separate_calls(ops, graphs, sampler_world, b_cap):
    rng = np.random.default_rng(40 + b_cap)
    idx = B_CAPS.index(b_cap)
    short = idx % 2 == 1                                                 # n_valid < B_cap in half of the cases
    guests = [("sampler", SamplerGuest(ops, sampler_world, b_cap, "filtered" if idx % 2 == 0 else "all_kept")),
              ("plan", PlanGuest(ops, graphs["small"], b_cap, short)),
              ("losses", LossesGuest(ops, b_cap, short))]
    combos = [(n, weighted) for n in (1, 2, 3) for weighted in (False, True)]
    for j, (name, guest) in enumerate(guests):
        for c in range(2):                                               # every (group size, weighted) pair over two capacities, rotating
            n, weighted = combos[(2 * (idx * 3 + j) + c) % len(combos)]
            gname = "buckets" if (idx + j + c) % 2 else "small"
            wide = (idx + j) % 3 == 0
            _check(ops, _specs(ops, graphs[gname], rng, n, weighted, wide), guest, (name, b_cap, n, weighted, gname, wide))


def test_every_guest_with_every_group_shape_at_the_bench_capacity(ops, graphs, sampler_world):
    rng = np.random.default_rng(99)
    b_cap = 1126
    guests = [("sampler", SamplerGuest(ops, sampler_world, b_cap, "filtered")), ("plan", PlanGuest(ops, graphs["small"], b_cap, True)),
              ("losses", LossesGuest(ops, b_cap, True))]
    for name, guest in guests:
        for n in (1, 2, 3):
            for weighted in (False, True):
                _check(ops, _specs(ops, graphs["buckets"], rng, n, weighted, wide=n > 1), guest, (name, n, weighted))


def test_refused_groups_launch_nothing(ops, graphs, sampler_world):
    g = graphs["small"]
    rng = np.random.default_rng(9)
    U, I = g.n_users, g.n_items
    for name, guest in (("sampler", SamplerGuest(ops, sampler_world, 257, "filtered")), ("plan", PlanGuest(ops, g, 257, False)),
                        ("losses", LossesGuest(ops, 257, False))):
        s = guest.state()
        before = {k: v.clone() for k, v in s.items()}
        # mixed kernel instances: an unweighted forward product beside a weighted transposed one
        Y0, Y1 = torch.full((U, 64), 7.0, device=DEV), torch.full((U, 64), 7.0, device=DEV)
        p0, k0 = _problem(ops, g.ui.fwd, _rand(rng, I, 64), Y0)
        p1, k1 = _problem(ops, g.iu.bwd, _rand(rng, I, 64), Y1)
        assert not ops.spmm_multi_guest([p0, p1], guest.guest(s))
        # d = 128 as a whole row (the softmax epilogue: no 64-column slices): outside the guest launch's one compiled instance
        Y2 = torch.full((U, 128), 7.0, device=DEV)
        p2, k2 = _problem(ops, g.ui.fwd, _rand(rng, I, 128), Y2, ops.spmm_epilogue(ops.EPI_SOFTMAX))
        assert not ops.spmm_multi_guest([p2], guest.guest(s))
        torch.cuda.synchronize()
        assert bool((Y0 == 7.0).all()) and bool((Y1 == 7.0).all()) and bool((Y2 == 7.0).all()), name
        for k in s:
            assert _same(before[k], s[k]), (name, k)


# ---- the whole step --------------------------------------------------------------------------------------------------------------
def _six_steps(root, refuse, graph, monkeypatch):
    from tests._step_env import fused_trainer, snapshot
    from tests.conftest import GOLDEN
    from llmrec_amd.fused import FusedStep
    meta = json.load(open(os.path.join(GOLDEN, "nf_mid_lr", "meta.json")))
    env = {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1", "LLMREC_DEVICE_SAMPLER": "1"}
    argv = ["--dataset", meta["config"]["dataset"], "--data_path", root + "/"] + meta["config"]["argv"] + ["--epoch", "1"]
    _, tr, step, batcher = fused_trainer(monkeypatch, argv, env, train=True, step=True, batcher=True)
    assert step and not step.multi_stream and step.fold and step.wgrad_rows
    step._refuse_guests = refuse
    batches, calls = [], []
    if graph:
        step.capture(batcher=batcher, unroll=4)                         # (the capture's warm-up is the first step)
        step.run_steps(5)
        st = step.static
    else:
        st = step._make_static()
        from llmrec_amd import _lib
        invoke, names = _lib._invoke, []
        monkeypatch.setattr(_lib, "_invoke", lambda fn, args: (names.append(fn), invoke(fn, args))[1])
        for _ in range(6):
            del names[:]
            step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
            calls.append((step.entry_point_calls_per_step, list(names)))
            batches.append(step.static_block.clone())
        monkeypatch.setattr(_lib, "_invoke", invoke)
    torch.cuda.synchronize()
    out = snapshot(tr, step, ("scal", "static_block", "epoch_sums"), grads=False)
    out["step_dev"] = batcher.step_dev.clone()
    for i, b in enumerate(batches):
        out["batch%d" % i] = b
    return out, calls


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph_unroll4"])
def test_six_steps_with_guests_equal_six_steps_without(datasets, monkeypatch, graph):
    ride, calls_ride = _six_steps(datasets["nf_mid_lr"], False, graph, monkeypatch)
    sep, calls_sep = _six_steps(datasets["nf_mid_lr"], True, graph, monkeypatch)
    assert any(k.startswith("m/") for k in ride) and int(ride["step_dev"]) == 6
    assert sorted(ride) == sorted(sep)
    bad = [k for k in ride if not _same(ride[k].contiguous().view(-1), sep[k].contiguous().view(-1))]
    assert not bad, bad[:6]
    if not graph:                                                        # three launches ride: three entry-point calls fewer per step
        (n_ride, seq), (n_sep, seq_sep) = calls_ride[-1], calls_sep[-1]
        print("[guests] entry-point calls per step: %d with guests, %d with every guest refused\n  %s" % (n_ride, n_sep, "\n  ".join(seq)))
        alone = ("llmrec_sample_batch_wide", "llmrec_bpr_scatter_plan_reach_mark", "llmrec_bpr_multi_losses_assemble_f32")
        assert n_ride == len(seq) == n_sep - 3 and n_sep == len(seq_sep)           # (17 against 20 at the bench's shape)
        assert seq.count("llmrec_spmm_multi_guest_f32") == 3 and not any(a in seq for a in alone)
        assert all(seq_sep.count(a) == 1 for a in alone) and "llmrec_spmm_multi_guest_f32" not in seq_sep
        # the guests' hosts: the forward's first group, the chain's third product, the backward's first group
        spmm = [c for c in seq if c.startswith("llmrec_spmm")]
        assert spmm[0] == "llmrec_spmm_multi_guest_f32" and spmm[2] == "llmrec_spmm_multi_guest_f32" and spmm[4] == "llmrec_spmm_multi_guest_f32"
