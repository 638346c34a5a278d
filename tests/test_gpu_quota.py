"""GPU: per-group quotas in served lists - llmrec_score_topk_candidates_capped_f32 (csrc/quota.hip) through
ops.score_topk_candidates_capped, llmrec_amd.serve.Recommender's group_of / per_group on all four calls and recommend.py --item_groups /
--per_group. No tolerance anywhere: the expected list of a query is the greedy walk of tests/_quota_ref.py down the ranking of
tests/_candidates_ref.py over tests/_eval_ref.chain_scores, and ids and score bits are compared exactly. The shapes are those of
tests/test_gpu_candidates.py (its Case): 40 users x 300 items, 70 unsorted queries with a user listed twice who carries two different
rows, candidate rows of 0, 1, 63, 64, 65, 200 and 2100 entries drawn from [-1, 303). A row's repeats collapse before the walk, so at 300
items a walk is at most 5 chunks of 64 sorted entries - with one group and cap 1 it walks them all."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import _lib
from tests import _quota_ref as Q
from tests import test_gpu_candidates as TC
from tests._dropin import ROOT, golden_argv
from tests.conftest import GoldenCase

DEV = "cuda"
U, I, N_QUERY = TC.U, TC.I, TC.N_QUERY
KS = (1, 20, 64, 65, 150, 1024)
KMAX = max(KS)
GUARD = 4096
ABOVE = 3000                                                       # a cap above every row length
DEFAULT_OVERFETCH = 2                                              # Recommender.recommend's (profiles/experiments/serve_quota.md)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


def _groupings(rng):
    """name -> (item_group int32 [I], n_groups)"""
    seven = rng.integers(0, 7, I)
    seven[rng.random(I) < 0.2] = -1
    beyond = rng.integers(0, 10, I)                                # ids 7, 8, 9 with n_groups = 7: no group
    return {"one": (np.zeros(I, np.int32), 1), "identity": (np.arange(I, dtype=np.int32), I), "seven": (seven.astype(np.int32), 7),
            "beyond": (beyond.astype(np.int32), 7)}


def _caps(rng, n_groups):
    vector = rng.integers(0, 4, n_groups)
    vector[rng.permutation(n_groups)[:2] if n_groups > 1 else [0]] = (0, 2) if n_groups > 1 else (2,)
    return {"1": 1, "2": 2, "above": ABOVE, "vector": vector.astype(np.int32)}


def _cap_arg(cap):
    return torch.from_numpy(cap).to(DEV) if isinstance(cap, np.ndarray) else cap


def _want(c, K, group, n_groups, cap, train=True, filt=False, excl=False, cand=None, scores=None, qn=None):
    e = c.excl if excl else (None, None)
    cd = cand if cand is not None else c.cand
    out = Q.topk_candidates_capped(c.S if scores is None else scores, c.qn if qn is None else qn, c.trp if train else None,
                                   c.tci if train else None, K, cd[0], cd[1], group, n_groups, cap, e[0], e[1], c.new_id if filt else None)
    return torch.from_numpy(out[0]).to(DEV), torch.from_numpy(out[1]).to(DEV)


@pytest.fixture(scope="module")
def case64(ops):
    return TC.Case(ops, 64, 2164)


@pytest.mark.parametrize("d", [1, 64, 100])
def test_every_grouping_cap_and_cutoff_against_the_walk(ops, case64, d):
    c = case64 if d == 64 else TC.Case(ops, d, 2100 + d)
    rng = np.random.default_rng(500 + d)
    cand = TC._dev(c.cand)
    plain = {K: ops.score_topk_candidates(c.Eu, c.Ei, c.q, c.train, K, cand) for K in KS}
    survivors = (plain[KMAX][0] >= 0).sum(dim=1)
    assert int(survivors.max()) > 150 and int(survivors.min()) == 0
    cut = 0
    for gname, (group, n_groups) in _groupings(rng).items():
        g_dev = torch.from_numpy(group).to(DEV)
        for cname, cap in _caps(rng, n_groups).items():
            want = _want(c, KMAX, group, n_groups, cap)            # once: a list at K is the first K of the list at 1024
            for K in KS:
                what = "d = %d, grouping %s, cap %s, K = %d" % (d, gname, cname, K)
                got = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, cand, g_dev, _cap_arg(cap), n_groups=n_groups)
                TC._assert_lists(got, want, K, what)
                if gname == "identity" and cname != "vector" or cname == "above":
                    assert TC._same(got, plain[K]), what           # nothing is capped: the uncapped op, bit for bit
                elif not TC._same(got, plain[K]):
                    cut += 1
                if gname == "one" and cname != "vector":
                    length = (got[0] >= 0).sum(dim=1)
                    assert torch.equal(length, torch.clamp(survivors, max=min(cap, K))), what
        if gname == "seven":                                       # n_groups from the tensor itself: one host read
            got = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 20, cand, g_dev, 2)
            TC._assert_lists(got, _want(c, 20, group, 7, 2), 20, "n_groups read from item_group")
    assert cut > 20                                                # the caps did something
    group, n_groups = _groupings(rng)["seven"]
    g_dev = torch.from_numpy(group).to(DEV)
    with pytest.raises(RuntimeError, match="1024"):
        ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 1025, cand, g_dev, 2, n_groups=7)
    with pytest.raises(RuntimeError, match="item_group int32"):
        ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 20, cand, g_dev[:-1], 2, n_groups=7)
    with pytest.raises(RuntimeError, match="item_group int32"):
        ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 20, cand, g_dev.long(), 2, n_groups=7)
    with pytest.raises(RuntimeError, match="cap"):
        ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 20, cand, g_dev, 0, n_groups=7)
    with pytest.raises(RuntimeError, match="cap"):
        ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 20, cand, g_dev, torch.ones(7, dtype=torch.int64, device=DEV))


def test_every_combination_of_removals(ops, case64):
    c = case64
    rng = np.random.default_rng(77)
    group, n_groups = _groupings(rng)["seven"]
    g_dev = torch.from_numpy(group).to(DEV)
    cand, excl = TC._dev(c.cand), TC._dev(c.excl)
    K = 20
    lists = []
    for train, filt, ex in TC.COMBOS:
        got = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train if train else None, K, cand, g_dev, 2, excl if ex else None,
                                               c.filt if filt else None, n_groups=n_groups)
        TC._assert_lists(got, _want(c, K, group, n_groups, 2, train, filt, ex), K, "train %s, filter %s, exclusion rows %s" % (train, filt, ex))
        lists.append(got[0])
    assert all(not torch.equal(lists[0], other) for other in lists[1:])      # every removal does something


def test_equal_score_bits_straddle_groups(ops):
    c = TC.Case(ops, 64, 2200, ties=True)                          # item rows 100 .. 159 are copies of rows 20 .. 79
    group = (np.arange(I) % 7).astype(np.int32)                    # a copy stands in another group than its original: 80 % 7 = 3
    g_dev = torch.from_numpy(group).to(DEV)
    cand = TC._dev(c.cand)
    tied = 0
    for cap in (1, 2):
        got = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, 64, cand, g_dev, cap, n_groups=7)
        TC._assert_lists(got, _want(c, 64, group, 7, cap), 64, "ties, cap %d" % cap)
        gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint32)
        eq = (gs[:, 1:] == gs[:, :-1]) & (gi[:, 1:] >= 0)
        tied += int(eq.sum())
        assert np.all(gi[:, :-1][eq] < gi[:, 1:][eq])              # equal score bits: ascending ids
    assert tied > 0, "no list holds two items of equal score bits: this case shows nothing"


def test_a_candidate_row_is_a_set(ops, case64):
    c = case64
    rng = np.random.default_rng(9)
    group, n_groups = _groupings(rng)["seven"]
    g_dev = torch.from_numpy(group).to(DEV)
    excl = TC._dev(c.excl)
    messy = TC._dev(TC._to_csr([rng.permutation(np.concatenate([r, r])) for r in c.cand_rows]))
    for K in (20, 150):
        plain = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, TC._dev(c.cand), g_dev, 2, excl, c.filt, n_groups=n_groups)
        again = ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, messy, g_dev, 2, excl, c.filt, n_groups=n_groups)
        assert TC._same(plain, again), K
        TC._assert_lists(plain, _want(c, K, group, n_groups, 2, True, True, True), K, "the plain rows")


def _call(c, K, cand, cand_nnz, ws, ws_bytes, g_dev, n_groups, group_cap, cap):
    """The C entry with guard bands in front of and behind both outputs: (idx, scores), the four bands."""
    n, d = c.q.numel(), c.d
    body = n * K * 4
    idx = torch.full((GUARD + body + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    sc = torch.full((GUARD + body + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    _lib.call("llmrec_score_topk_candidates_capped_f32", n, c.q.data_ptr(), c.Eu.data_ptr(), d, c.Ei.data_ptr(), d, I, d,
              c.train.rowptr.data_ptr(), c.train.colidx.data_ptr(), K, idx.data_ptr() + GUARD, sc.data_ptr() + GUARD, ws.data_ptr(), ws_bytes,
              cand[0].data_ptr(), cand[1].data_ptr(), cand_nnz, None, None, 0, None,
              g_dev.data_ptr(), n_groups, group_cap.data_ptr() if group_cap is not None else None, cap, None)
    torch.cuda.synchronize()
    out = idx[GUARD:GUARD + body].view(torch.int32).view(n, K), sc[GUARD:GUARD + body].view(torch.float32).view(n, K)
    return out, (idx[:GUARD], idx[GUARD + body:], sc[:GUARD], sc[GUARD + body:])


@pytest.mark.parametrize("K", [20, 150, 1024])
def test_guard_bands_and_a_broken_cand_rowptr(ops, case64, K):
    c = case64
    rng = np.random.default_rng(K)
    group, n_groups = _groupings(rng)["seven"]
    g_dev = torch.from_numpy(group).to(DEV)
    vector = _caps(rng, n_groups)["vector"]
    rp, ci = c.cand
    nnz = len(ci)
    need = _lib.query("llmrec_score_topk_candidates_workspace_bytes", N_QUERY, K, nnz, 0)
    for group_cap, cap in ((None, 1), (torch.from_numpy(vector).to(DEV), 0)):
        ws = torch.full((need + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
        got, bands = _call(c, K, TC._dev(c.cand), nnz, ws, need, g_dev, n_groups, group_cap, cap)
        TC._assert_lists(got, _want(c, K, group, n_groups, vector if group_cap is not None else 1), K, "the C entry, K = %d" % K)
        assert all((b == 0xEE).all() for b in bands), "written outside the outputs"
        assert (ws[need:] == 0xEE).all(), "written behind the workspace"
    late = rp.copy(); late[0] = 1
    decreasing = rp.copy(); decreasing[40] = decreasing[41] + 1
    short = rp.copy(); short[-1] -= 1
    for what, rowptr in (("a cand_rowptr that starts at 1", late), ("a decreasing cand_rowptr", decreasing),
                         ("a cand_rowptr that ends one below cand_nnz", short)):
        ws = torch.full((need + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
        got, bands = _call(c, K, (torch.from_numpy(rowptr).to(DEV), torch.from_numpy(ci).to(DEV)), nnz, ws, need, g_dev, n_groups, None, 2)
        TC._assert_empty(got, what)
        assert all((b == 0xEE).all() for b in bands) and (ws[need:] == 0xEE).all(), what
    # no candidate entry at all: one launch, no workspace
    none = (torch.zeros(N_QUERY + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    TC._assert_empty(ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, none, g_dev, 2, n_groups=n_groups))


@pytest.mark.parametrize("K", [20, 150])
def test_a_captured_replay_gives_the_eager_bits(ops, case64, K):
    c = case64
    rng = np.random.default_rng(70 + K)
    group, n_groups = _groupings(rng)["seven"]
    g_dev = torch.from_numpy(group).to(DEV)
    vector = _caps(rng, n_groups)["vector"]
    for cap, filt, ex in ((2, None, False), (torch.from_numpy(vector).to(DEV), c.filt, True)):
        rp, ci = TC._dev(c.cand)
        excl = TC._dev(c.excl) if ex else None
        ws = ops.score_topk_candidates_workspace(N_QUERY, K, ci.numel(), excl[1].numel() if ex else 0, DEV)
        run = lambda: ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, (rp, ci), g_dev, cap, excl, filt, ws=ws, n_groups=n_groups)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        g.replay()
        torch.cuda.synchronize()
        assert TC._same(out, first), ex
        host_cap = vector if ex else 2
        TC._assert_lists(out, _want(c, K, group, n_groups, host_cap, True, filt is not None, ex), K, "first replay")
        # other candidates in the same buffers: the rows move to other queries, the sizes stay
        again = TC._to_csr([rng.integers(-1, I + 3, len(c.cand_rows[p])) for p in rng.permutation(N_QUERY)])
        assert len(again[1]) == ci.numel()
        rp.copy_(torch.from_numpy(again[0])); ci.copy_(torch.from_numpy(again[1]))
        g.replay()
        torch.cuda.synchronize()
        assert TC._same(out, ops.score_topk_candidates_capped(c.Eu, c.Ei, c.q, c.train, K, (rp, ci), g_dev, cap, excl, filt, n_groups=n_groups)), ex
        assert not torch.equal(out[0], first[0])
        TC._assert_lists(out, _want(c, K, group, n_groups, host_cap, True, filt is not None, ex, cand=again), K, "a replay with other candidates")


def _as_rank(want, k):
    return want[0][:, :k].long(), want[1][:, :k].contiguous()


def _padded(rows):
    width = max(len(r) for r in rows)
    out = np.full((len(rows), width), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_recommender_rank_with_quotas(ops, case64):
    from llmrec_amd.serve import Recommender
    c = case64
    rng = np.random.default_rng(31)
    group, n_groups = _groupings(rng)["seven"]
    vector = _caps(rng, n_groups)["vector"]
    rec = Recommender(c.Eu, c.Ei, c.train)
    users = c.qn.tolist()
    k = 65
    padded = _padded([r[(r >= 0) & (r < I)] for r in c.cand_rows])  # (the host forms refuse an id >= n_items; negative entries are padding)
    plain = rec.rank(users, padded, k)
    for per_group, cap in ((2, 2), (vector.tolist(), vector), (ABOVE, ABOVE)):
        want = _as_rank(_want(c, k, group, n_groups, cap), k)
        for chunk in (65536, 16):
            for group_of in (group, torch.from_numpy(group).to(DEV), group.tolist()):
                got = rec.rank(users, padded, k, chunk=chunk, group_of=group_of, per_group=per_group)
                assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (N_QUERY, k)
                assert TC._same(got, want), (per_group, chunk)
        assert TC._same(got, plain) == (per_group == ABOVE)
    erows = [r[(r >= 0) & (r < I)] for r in (c.excl[1][a:b] for a, b in zip(c.excl[0][:-1], c.excl[0][1:]))]
    got = rec.rank(users, padded, k, allow_items=np.flatnonzero(c.allow), exclude=erows, chunk=16, group_of=group, per_group=1)
    assert TC._same(got, _as_rank(_want(c, k, group, n_groups, 1, True, True, True), k))
    with pytest.raises(ValueError, match="per_group is missing"):
        rec.rank(users, padded, k, group_of=group)
    with pytest.raises(ValueError, match="group_of is missing"):
        rec.rank(users, padded, k, per_group=2)
    with pytest.raises(ValueError, match="group_of: 300 integers"):
        rec.rank(users, padded, k, group_of=group[:-1], per_group=2)
    with pytest.raises(RuntimeError, match="1024"):
        rec.rank(users, padded, 1025, group_of=group, per_group=2)


def _new_users(ops):
    from tests.test_gpu_foldin import _synthetic_recommender
    rec, rng = _synthetic_recommender(ops)
    hist = [rng.choice(rec.n_items, size=int(m), replace=False) for m in (1, 5, 20, 200, 0, 64, 257, 40)] * 3
    S = ops.scores(rec.embed_new(hist), rec.E_i, torch.arange(len(hist), device=DEV)).cpu().numpy()
    return rec, rng, hist, S


def test_recommender_rank_new_with_quotas(ops):
    rec, rng, hist, S = _new_users(ops)
    n, n_items = len(hist), rec.n_items
    cand = [rng.integers(0, n_items, (0, 1, 63, 64, 65, 200, 2100)[i % 7]) for i in range(n)]
    cand[3] = np.concatenate([cand[3], hist[3][:50]])              # candidates out of the history itself
    group = rng.integers(-1, 12, n_items).astype(np.int32)
    k = 70
    crp, cci = TC._to_csr(cand)
    hrp, hci = TC._to_csr(hist)
    want = Q.topk_candidates_capped(S, np.arange(n), None, None, k, crp, cci, group, 12, 3, hrp, hci)
    want = torch.from_numpy(want[0]).to(DEV).long(), torch.from_numpy(want[1]).to(DEV)
    assert (want[0][:, k - 1] >= 0).any() and (want[0][:, 0] < 0).any()
    for chunk in (65536, 5):
        got = rec.rank_new(hist, _padded(cand), k, chunk=chunk, group_of=group, per_group=3)
        assert got[0].dtype == torch.int64 and got[0].shape == (n, k) and TC._same(got, want), chunk
    assert not TC._same(got, rec.rank_new(hist, _padded(cand), k))


def _round2_expected(S, qn, trp, tci, k, K1, group, n_groups, cap, erp=None, eci=None):
    """From the restatement alone: the queries whose first K1 ranks are all taken (the fetched row is full) and whose walk over those
    ranks does not fill k slots."""
    n_items = S.shape[1]
    g, caps = Q.group_and_cap(group, n_groups, cap)
    count = 0
    for q, u in enumerate(qn):
        t = tci[trp[u]:trp[u + 1]] if trp is not None else ()
        e = eci[erp[q]:erp[q + 1]] if erp is not None else ()
        order = Q.ranking(S[u], Q.survivors(np.arange(n_items), n_items, t, e))
        count += len(order) >= K1 and len(Q.greedy(order[:K1], g, caps, k)) < k
    return count


def test_recommend_with_quotas_is_exact_over_the_whole_catalogue(ops, case64):
    from llmrec_amd.serve import Recommender
    c = case64
    rng = np.random.default_rng(2024)
    group = rng.integers(0, 10, I).astype(np.int32)
    k = 20
    rec = Recommender(c.Eu, c.Ei, c.train)
    users = c.qn.tolist()
    want = Q.recommend_capped(c.S, c.qn, c.trp, c.tci, k, group, 10, 2)
    want = torch.from_numpy(want[0]).to(DEV).long(), torch.from_numpy(want[1]).to(DEV)
    assert (want[0] >= 0).all()                                    # 10 groups x 2: every list is full
    assert not TC._same(want, rec.recommend(users, k))
    assert inspect.signature(Recommender.recommend).parameters["overfetch"].default == DEFAULT_OVERFETCH
    assert inspect.signature(Recommender.recommend_new).parameters["overfetch"].default == DEFAULT_OVERFETCH
    sent = {}
    for overfetch in (1, None, 64):
        kw = {} if overfetch is None else {"overfetch": overfetch}
        got = rec.recommend(users, k, group_of=group, per_group=2, **kw)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and TC._same(got, want), overfetch
        assert rec.last_quota["queries"] == N_QUERY
        sent[overfetch] = rec.last_quota["round2"]
        assert sent[overfetch] == _round2_expected(c.S, c.qn, c.trp, c.tci, k, min(1024, (overfetch or DEFAULT_OVERFETCH) * k), group, 10, 2), overfetch
    print("round 2 served %s of %d queries" % (sent, N_QUERY))
    assert sent[1] > 0                                             # round 2 ran ...
    assert sent[None] < N_QUERY                                    # ... and at the default round 1 settled at least one query
    assert sent[64] == 0                                           # 1024 > 300 items: no fetched row is full, every list is final
    # chunks below the query count, exclusion lists and a filter; a cap vector with a removed group
    got = rec.recommend(users, k, group_of=group, per_group=2, overfetch=1, chunk=16)
    assert TC._same(got, want) and rec.last_quota == {"queries": N_QUERY, "round2": sent[1]}
    erows = [r[(r >= 0) & (r < I)] for r in (c.excl[1][a:b] for a, b in zip(c.excl[0][:-1], c.excl[0][1:]))]
    caps = np.array([2, 0, 1, 3, 2, 2, 0, 1, 2, 5], dtype=np.int32)
    ref = Q.recommend_capped(c.S, c.qn, c.trp, c.tci, k, group, 10, caps, c.excl[0], c.excl[1], c.new_id)
    ref = torch.from_numpy(ref[0]).to(DEV).long(), torch.from_numpy(ref[1]).to(DEV)
    for overfetch, chunk in ((1, 16), (2, None), (4, 65536)):
        got = rec.recommend(users, k, allow_items=np.flatnonzero(c.allow), exclude=erows, group_of=group, per_group=caps.tolist(), overfetch=overfetch,
                            chunk=chunk)
        assert TC._same(got, ref), (overfetch, chunk)
        assert rec.last_quota["round2"] > 0                        # 18 slots at most: no list fills, every full fetched row goes on
    with pytest.raises(ValueError, match="overfetch"):
        rec.recommend(users, k, group_of=group, per_group=2, overfetch=0)
    with pytest.raises(ValueError, match="per_group is missing"):
        rec.recommend(users, k, group_of=group)
    assert rec.recommend([], k, group_of=group, per_group=2)[0].shape == (0, k)


def test_recommend_new_with_quotas_is_exact_over_the_whole_catalogue(ops):
    rec, rng, hist, S = _new_users(ops)
    n, n_items = len(hist), rec.n_items
    group = rng.integers(0, 10, n_items).astype(np.int32)
    k = 20
    hrp, hci = TC._to_csr(hist)
    want = Q.recommend_capped(S, np.arange(n), None, None, k, group, 10, 2, hrp, hci)
    want = torch.from_numpy(want[0]).to(DEV).long(), torch.from_numpy(want[1]).to(DEV)
    sent = {}
    for overfetch in (1, None, 64):
        kw = {} if overfetch is None else {"overfetch": overfetch}
        got = rec.recommend_new(hist, k, group_of=group, per_group=2, **kw)
        assert got[0].dtype == torch.int64 and TC._same(got, want), overfetch
        sent[overfetch] = rec.last_quota["round2"]
        assert sent[overfetch] == _round2_expected(S, np.arange(n), None, None, k, min(1024, (overfetch or DEFAULT_OVERFETCH) * k), group, 10, 2, hrp, hci), overfetch
    print("round 2 served %s of %d new users" % (sent, n))
    assert sent[1] > 0 and sent[None] < n
    got = rec.recommend_new(hist, k, group_of=group, per_group=2, overfetch=1, chunk=5)
    assert TC._same(got, want) and rec.last_quota == {"queries": n, "round2": sent[1]}
    assert not TC._same(got, rec.recommend_new(hist, k))


def test_the_script_in_a_fresh_process(ops, monkeypatch, tmp_path):
    """recommend.py --item_groups / --per_group on tests/golden/nf_tiny (96 users x 80 items), with and without --candidates, against
    Recommender.rank / recommend with group_of / per_group."""
    from llmrec_amd import checkpoint as CK
    from llmrec_amd.serve import Recommender
    from llmrec_amd.step_options import ENV_SWITCHES, TRAINER_SWITCHES
    from tests.test_gpu_serve import ENVS, FLAGS, _train_and_reload
    f, best = _train_and_reload(monkeypatch, "graph", tmp_path)
    rng = np.random.default_rng(5)
    users = rng.integers(0, 96, 70)
    pairs = np.stack([rng.integers(0, 96, 1500), rng.integers(0, 80, 1500)], axis=1)
    group = rng.integers(-1, 6, 80)
    (tmp_path / "users.txt").write_text("".join("%d\n" % u for u in users))
    (tmp_path / "cand.txt").write_text("".join("%d %d\n" % (u, i) for u, i in pairs))
    (tmp_path / "groups.txt").write_text("".join("%d\n" % g for g in group))
    np.save(str(tmp_path / "groups.npy"), group)
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES + TRAINER_SWITCHES + tuple(CK.CHECKPOINT_SWITCHES)}
    env.update(ENVS["graph"])
    argv = golden_argv(GoldenCase("nf_tiny")) + FLAGS + ["--epoch", "2"]
    rec = Recommender.from_checkpoint(f.trainer, best)
    by_user = {}
    for u, i in pairs:
        if u in users:
            by_user.setdefault(int(u), []).append(int(i))
    ranked = rec.rank(users, by_user, 20, group_of=group, per_group=2)
    whole = rec.recommend(users, 20, group_of=group, per_group=2)
    assert not torch.equal(ranked[0], rec.rank(users, by_user, 20)[0]) and not torch.equal(whole[0], rec.recommend(users, 20)[0])
    for name, extra, want in (("ranked", ["--candidates", str(tmp_path / "cand.txt"), "--item_groups", str(tmp_path / "groups.txt")], ranked),
                              ("whole", ["--item_groups", str(tmp_path / "groups.npy")], whole)):
        out = str(tmp_path / (name + ".npz"))
        cmd = [sys.executable, os.path.join(ROOT, "recommend.py"), "--checkpoint", best, "--users", str(tmp_path / "users.txt"), "--topk", "20",
               "--per_group", "2", "--out", out] + extra
        r = subprocess.run(cmd + argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        assert np.array_equal(z["users"], users) and z["items"].dtype == np.int64 and z["scores"].dtype == np.float32
        assert np.array_equal(z["items"], want[0].cpu().numpy()), name
        assert np.array_equal(z["scores"].view(np.uint32), want[1].cpu().numpy().view(np.uint32)), name
        items = z["items"]
        for row in items:                                          # the quota, from the file alone
            g = group[row[row >= 0]]
            assert all(np.count_nonzero(g == x) <= 2 for x in range(6))
