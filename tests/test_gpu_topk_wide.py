"""Cut-offs above 64: llmrec_score_topk_wide_f32 through ops.score_topk / ops.export_candidates / ops.topk_eval_sums / FusedStep.eval_topk /
the drop-in's Trainer.test. No tolerance anywhere on the lists: the expected list of a user is the candidates (items outside the train row)
ordered by (score desc, item id asc) over the bits ops.scores returns - the same arithmetic -, so ids and score bits are compared with
torch.equal and no case is excluded. The ordering is computed on the device by two stable sorts (score descending, then candidates first) and is
held to np.lexsort((ids, -scores)) on sampled rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS_WIDE = (65, 100, 112, 113, 128, 129, 200, 1000, 1024)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


def _csr(ops, rows, cols, U, I):
    rp, ci, _ = ops.csr_from_coo(torch.as_tensor(rows, dtype=torch.int64).to(DEV), torch.as_tensor(cols, dtype=torch.int64).to(DEV), None, U, I)
    return ops.Csr(U, I, rp, ci, None, None, None, ops.SpmmPlan())


def _train_csr(ops, U, I, rng, max_deg, duplicates=0):
    degs = rng.integers(0, max_deg + 1, size=U)
    rows = np.repeat(np.arange(U), degs)
    cols = np.concatenate([rng.choice(I, size=int(dg), replace=False) for dg in degs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    if duplicates and rows.size:                                   # llmrec_csr_build keeps repeated pairs: the merged mask must keep them too
        pick = rng.integers(0, rows.size, duplicates)
        rows, cols = np.concatenate([rows, rows[pick]]), np.concatenate([cols, cols[pick]])
    return _csr(ops, rows, cols, U, I)


def _masked(q, train, n_items):
    n = q.numel()
    masked = torch.zeros(n, n_items, dtype=torch.bool, device=DEV)
    if train is not None:
        rp, ci = train.rowptr.long(), train.colidx.long()
        lens = rp[q + 1] - rp[q]
        rows = torch.repeat_interleave(torch.arange(n, device=DEV), lens)
        offs = torch.arange(int(lens.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
        masked[rows, ci[torch.repeat_interleave(rp[q], lens) + offs]] = True
    return masked


def _expected(ops, Eu, Ei, q, train, kmax, check_rows=()):
    """([n, kmax] int32 ids, [n, kmax] float32 scores): candidates by (score desc, id asc), -1 / -inf behind the last candidate."""
    S = ops.scores(Eu, Ei, q)
    n, I = S.shape
    masked = _masked(q, train, I)
    order = torch.sort(S, dim=1, descending=True, stable=True).indices                       # ties keep ascending ids
    first = torch.sort(masked.gather(1, order).to(torch.uint8), dim=1, stable=True).indices    # candidates in front, order kept
    order = order.gather(1, first)
    n_cand = I - masked.sum(1)
    idx = torch.full((n, kmax), -1, dtype=torch.int32, device=DEV)
    sc = torch.full((n, kmax), float("-inf"), dtype=torch.float32, device=DEV)
    k = min(kmax, I)
    live = torch.arange(k, device=DEV)[None, :] < n_cand[:, None]
    idx[:, :k] = torch.where(live, order[:, :k].to(torch.int32), idx[:, :k])
    sc[:, :k] = torch.where(live, S.gather(1, order[:, :k]), sc[:, :k])
    for r in check_rows:                                           # the statement itself, in numpy
        s = S[r].cpu().numpy()
        ids = np.flatnonzero(~masked[r].cpu().numpy())
        want = ids[np.lexsort((ids, -s[ids]))][:kmax]
        assert idx[r, :len(want)].cpu().numpy().tolist() == want.tolist() and (idx[r, len(want):] == -1).all()
    return idx, sc


def _assert_lists(got, want, K, what):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == (wi.shape[0], K) and gs.shape == gi.shape, what
    same_i = torch.equal(gi, wi[:, :K])
    same_s = torch.equal(gs.view(torch.int32), ws[:, :K].contiguous().view(torch.int32))
    if not (same_i and same_s):
        bad = (gi != wi[:, :K]).nonzero()
        raise AssertionError("%s: %d ids differ (first %s), score bits equal: %s" % (what, bad.shape[0], bad[:3].tolist(), same_s))


@pytest.mark.parametrize("d", [64, 128])
def test_small_shape_every_cutoff_mode_and_mask(ops, d):
    rng = np.random.default_rng(640 + d)
    U, I = 211, 3000
    Eu = torch.tensor((rng.standard_normal((U, d)) * 0.4).astype(np.float32)).to(DEV)
    Ei = torch.tensor((rng.standard_normal((I, d)) * 0.4).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 60, duplicates=200)
    q = torch.tensor(np.concatenate([rng.permutation(U)[:180], rng.integers(0, U, 23)])).to(DEV)    # 203 queries: unsorted, users listed twice, not a multiple of 16
    for tr in (train, None):
        want = _expected(ops, Eu, Ei, q, tr, 1024, check_rows=(0, 7, 202))
        for K in KS_WIDE:
            for mode in (None, "exact", "prefilter"):
                _assert_lists(ops.score_topk(Eu, Ei, q, tr, K, mode=mode), want, K, "K = %d, mode %s, train %s" % (K, mode, tr is not None))
    # the Stage-1 export: no mask, int64 ids
    cand = ops.export_candidates(Eu, Ei, k=300, query_users=q)
    assert cand.dtype == torch.int64 and torch.equal(cand, want[0][:, :300].long())
    with pytest.raises(RuntimeError, match="1024"):
        ops.score_topk(Eu, Ei, q, train, 1025)


def test_netflix_shape_with_its_train_rows(ops):
    from llmrec_amd import synth
    sh = synth.NF_SHAPE
    rows, cols = synth.bipartite_edges(sh.n_users, sh.n_items, sh.n_train, seed=0)
    train = _csr(ops, rows, cols, sh.n_users, sh.n_items)
    g = torch.Generator(device=DEV); g.manual_seed(5)
    Eu = torch.randn(sh.n_users, 64, generator=g, device=DEV) * 0.2
    Ei = torch.randn(sh.n_items, 64, generator=g, device=DEV) * 0.2
    q = torch.arange(sh.n_users, device=DEV)
    want = _expected(ops, Eu, Ei, q, train, 1024, check_rows=(0, 13186))
    for K in KS_WIDE:
        for mode in (None, "exact", "prefilter"):
            _assert_lists(ops.score_topk(Eu, Ei, q, train, K, mode=mode), want, K, "netflix shape, K = %d, mode %s" % (K, mode))
    a = ops.score_topk(Eu, Ei, q, train, 1024)
    b = ops.score_topk(Eu, Ei, q, train, 1024)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))       # deterministic
    del want
    want = _expected(ops, Eu, Ei, q, None, 200)
    for K in (65, 200):
        _assert_lists(ops.score_topk(Eu, Ei, q, None, K), want, K, "netflix shape, no mask, K = %d" % K)


def test_first_columns_are_the_single_sweep_answer(ops):
    rng = np.random.default_rng(9)
    U, I, d = 333, 5000, 64
    Eu = torch.tensor((rng.standard_normal((U, d)) * 0.4).astype(np.float32)).to(DEV)
    Ei = torch.tensor((rng.standard_normal((I, d)) * 0.4).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 80)
    q = torch.tensor(rng.permutation(U)).to(DEV)
    i64, s64 = ops.score_topk(Eu, Ei, q, train, 64)
    i50, s50 = ops.score_topk(Eu, Ei, q, train, 50)
    for K in (65, 200):
        for mode in (None, "exact", "prefilter"):
            iw, sw = ops.score_topk(Eu, Ei, q, train, K, mode=mode)
            assert torch.equal(iw[:, :64], i64) and torch.equal(sw[:, :64].contiguous().view(torch.int32), s64.view(torch.int32)), (K, mode)
            assert torch.equal(iw[:, :50], i50) and torch.equal(sw[:, :50].contiguous().view(torch.int32), s50.view(torch.int32)), (K, mode)


@pytest.mark.parametrize("kind", ["all_equal", "integers", "zeros_and_signs", "near_identical_rows", "strictly_ascending"])
def test_adversarial_tables(ops, kind):
    rng = np.random.default_rng({"all_equal": 201, "integers": 205, "zeros_and_signs": 209, "near_identical_rows": 210, "strictly_ascending": 211}[kind])
    U, I, d = 100, 3000, 64
    if kind == "all_equal":                  # the list is the first K unmasked ids
        Eu = np.full((U, d), 0.5, dtype=np.float32); Ei = np.full((I, d), 0.25, dtype=np.float32)
    elif kind == "integers":                 # exact arithmetic in every order: ties everywhere, ranked by item id
        Ei = rng.integers(-2, 3, size=(I, d)).astype(np.float32); Eu = rng.integers(-2, 3, size=(U, d)).astype(np.float32)
    elif kind == "zeros_and_signs":          # both signs around exact zeros; a third of the items and a few users are all-zero rows
        Eu = (rng.standard_normal((U, d)) * 0.2).astype(np.float32); Eu[::9] = 0.0
        Ei = (rng.standard_normal((I, d)) * 0.2).astype(np.float32); Ei[::3] = 0.0; Ei[1::7] *= -0.0
    elif kind == "near_identical_rows":      # scores within ~1e-4 relative of one another
        base = rng.standard_normal(d).astype(np.float32)
        Ei = base[None, :] + (rng.standard_normal((I, d)) * 1e-4).astype(np.float32)
        Eu = np.abs(rng.standard_normal((U, d))).astype(np.float32)
    else:                                    # every item beats all items before it, for every user
        Eu = (np.abs(rng.standard_normal((U, d))) + 0.5).astype(np.float32)
        Ei = (np.full((I, d), 0.25) * (1.0 + np.arange(I)[:, None] * 1e-3)).astype(np.float32)
    Eu, Ei = torch.tensor(Eu).to(DEV), torch.tensor(Ei).to(DEV)
    train = _train_csr(ops, U, I, rng, 30)
    q = torch.arange(U, device=DEV)
    want = _expected(ops, Eu, Ei, q, train, 1024, check_rows=(0, 9, 99))
    for K in (100, 1024):
        for mode in (None, "exact", "prefilter"):
            _assert_lists(ops.score_topk(Eu, Ei, q, train, K, mode=mode), want, K, "%s, K = %d, mode %s" % (kind, K, mode))
    if kind == "all_equal":
        free = (~_masked(q, train, I)[3]).nonzero().flatten()[:1024]
        assert torch.equal(want[0][3].long(), free)


def test_exhausted_users_leave_empty_tails(ops):
    rng = np.random.default_rng(31)
    d = 64
    # 90 items, 60 of them train items: 30 candidates < K; user 5 has every item in its train row; user 6 none
    U, I = 40, 90
    rows, cols = [], []
    for u in range(U):
        c = np.arange(I) if u == 5 else (np.zeros(0, dtype=np.int64) if u == 6 else rng.choice(I, size=60, replace=False))
        rows.append(np.full(len(c), u)); cols.append(c)
    train = _csr(ops, np.concatenate(rows), np.concatenate(cols), U, I)
    Eu = torch.tensor(rng.standard_normal((U, d)).astype(np.float32)).to(DEV)
    Ei = torch.tensor(rng.standard_normal((I, d)).astype(np.float32)).to(DEV)
    q = torch.arange(U, device=DEV)
    want = _expected(ops, Eu, Ei, q, train, 1024, check_rows=(0, 5, 6))
    for K in (65, 100, 129, 1024):
        for mode in ("exact", "prefilter"):
            got = ops.score_topk(Eu, Ei, q, train, K, mode=mode)
            _assert_lists(got, want, K, "exhaustion, K = %d, mode %s" % (K, mode))
            assert (got[0][5] == -1).all() and torch.isneginf(got[1][5]).all()
            assert (got[0][0, 30:] == -1).all() and (got[0][0, :30] >= 0).all()
            assert (got[0][6, :min(K, I)] >= 0).all() and (got[0][6, I:] == -1).all()
    # fewer items than K, with and without a mask
    want = _expected(ops, Eu, Ei[:50].contiguous(), q, None, 200)
    _assert_lists(ops.score_topk(Eu, Ei[:50].contiguous(), q, None, 200), want, 200, "n_items < K")
    _assert_lists(ops.score_topk(Eu, Ei[:50].contiguous(), q, None, 65, mode="exact"), want, 65, "n_items < K, exact")


def test_a_capacity_that_is_too_small_is_detected_on_the_device(ops):
    """train_nnz below the sum of the queried train rows: nothing is written beyond the mask buffers, every list comes back empty."""
    from llmrec_amd import _lib
    rng = np.random.default_rng(41)
    U, I, d, K = 64, 2000, 64, 100
    Eu = torch.tensor(rng.standard_normal((U, d)).astype(np.float32)).to(DEV)
    Ei = torch.tensor(rng.standard_normal((I, d)).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 50)
    q = torch.arange(U, device=DEV)
    nnz = ops._wide_train_nnz(train, q)
    assert nnz == train.colidx.numel() > 100
    ws = ops.topk_workspace(U, I, DEV, d, K, nnz - 1)
    idx = torch.zeros(U, K, dtype=torch.int32, device=DEV); sc = torch.zeros(U, K, device=DEV)
    _lib.call("llmrec_score_topk_wide_f32", U, q.data_ptr(), Eu.data_ptr(), d, Ei.data_ptr(), d, I, d, train.rowptr.data_ptr(), train.colidx.data_ptr(),
              K, idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel(), 1, nnz - 1, None)
    torch.cuda.synchronize()
    assert (idx == -1).all() and torch.isneginf(sc).all()


def test_item_parts_beyond_131072_items(ops):
    g = torch.Generator(device=DEV); g.manual_seed(13)
    U, I, d, K = 300, 140_000, 64, 200
    Ei = torch.randn(I, d, generator=g, device=DEV) * 0.3
    Eu = torch.randn(U, d, generator=g, device=DEV) * 0.3
    rng = np.random.default_rng(13)
    train = _train_csr(ops, U, I, rng, 100)
    q = torch.arange(U, device=DEV)
    want = _expected(ops, Eu, Ei, q, train, K, check_rows=(0,))
    for mode in (None, "exact"):
        _assert_lists(ops.score_topk(Eu, Ei, q, train, K, mode=mode), want, K, "item parts, mode %s" % mode)


def _tree(v):
    v = v.copy()
    off = len(v) // 2
    while off > 0:
        v[:off] += v[off:2 * off]
        off //= 2
    return v[0]


def test_eval_sums_over_wide_lists(ops):
    from oracle import oracle
    rng = np.random.default_rng(77)
    U, I, d = 1300, 3000, 64
    Eu = torch.tensor((rng.standard_normal((U, d)) * 0.4).astype(np.float32)).to(DEV)
    Ei = torch.tensor((rng.standard_normal((I, d)) * 0.4).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 40)
    held_np = [np.sort(rng.choice(I, size=int(n), replace=False)) for n in rng.integers(0, 400, size=U)]
    held_np[3] = np.arange(I)                                       # every ranked item is a hit
    held = _csr(ops, np.repeat(np.arange(U), [len(h) for h in held_np]), np.concatenate(held_np), U, I)
    q = torch.tensor(rng.permutation(U)).to(DEV)
    idx, _ = ops.score_topk(Eu, Ei, q, train, 1024)
    lists, qs = idx.cpu().numpy(), q.cpu().numpy()

    def want(Ks, K):
        tot = {k: np.zeros(len(Ks)) for k in ("precision", "recall", "ndcg", "hit_ratio")}
        for row, u in zip(lists, qs):
            top = row[:K][row[:K] >= 0]
            pos = set(held_np[u].tolist())
            m = oracle.metrics_from_hits([1 if int(i) in pos else 0 for i in top], len(held_np[u]), Ks)
            for k in tot:
                tot[k] += m[k]
        return np.stack([tot["precision"], tot["recall"], tot["ndcg"], tot["hit_ratio"]])

    for Ks, K in (([10, 20, 50, 100, 200, 1024], 1024), ([10, 100, 129], 129), ([10, 20, 50, 100], 200)):
        got = ops.topk_eval_sums(idx[:, :K].contiguous(), q, held.rowptr, held.colidx, Ks).cpu().numpy()
        ref = want(Ks, K)
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("eval sums K = %d: max relative difference %.3e" % (K, rel.max()))
        assert rel.max() <= 1e-12, (K, rel)
        again = ops.topk_eval_sums(idx[:, :K].contiguous(), q, held.rowptr, held.colidx, Ks).cpu().numpy()
        assert np.array_equal(got, again)
    # lists of at most 128 columns keep the one-thread-per-user kernel and its bits: the per-user values of llmrec_topk_metrics (the same
    # arithmetic) added in that kernel's order - a pairwise tree over each block of 128 users, the blocks in order, a tree over 256 slots
    Ks = [10, 20, 50]
    i50 = idx[:, :50].contiguous()
    got = ops.topk_eval_sums(i50, q, held.rowptr, held.colidx, Ks).cpu().numpy()
    per = ops.topk_metrics(i50, ops.topk_hits(i50, q, held.rowptr, held.colidx), q, held.rowptr, Ks).cpu().numpy()      # [n, 4, 3]
    pad = np.zeros((-(-U // 128) * 128, 4, 3)); pad[:U] = per
    for m in range(4):
        for t in range(3):
            partial = np.array([_tree(pad[b * 128:(b + 1) * 128, m, t]) for b in range(len(pad) // 128)])
            slots = np.zeros(256)
            for b, p in enumerate(partial):
                slots[b % 256] += p
            assert got[m, t] == _tree(slots), (m, t)
    rel = np.abs(got - want(Ks, 50)) / np.maximum(np.abs(want(Ks, 50)), 1e-300)
    assert rel.max() <= 1e-12


# ---- the drop-in's Trainer.test with --Ks '[10,20,50,100]' ----
from tests._dropin import load_dropin, golden_argv          # noqa: E402
from tests.conftest import GoldenCase                       # noqa: E402


def _oracle_result(m, fused, users, Ks):
    """oracle.evaluate over the device's own score bits: (metrics, ranked lists)."""
    from oracle import oracle
    from llmrec_amd import ops as _ops
    dg = m.data_generator
    fn = lambda blk: _ops.scores(fused.E_u, fused.E_i, torch.tensor(list(blk), device=DEV)).cpu().numpy()
    return oracle.evaluate(fused.E_u.detach().cpu().numpy(), fused.E_i.detach().cpu().numpy(), users, dg.train_items, dg.test_set, Ks, scores_fn=fn)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("flag", ["part", "full"])
@pytest.mark.parametrize("kmax", [100, 200])
def test_trainer_test_at_cutoffs_above_64(monkeypatch, graph, flag, kmax):
    """Trainer.test on the golden tiny set (80 items: every list ends in an empty tail) against oracle.evaluate over the device's own score
    bits. The ranked lists are compared exactly. The averages are the same per-user doubles added in another order (fixed trees on the
    device, one after the other in the oracle), so they are held to the relative 1e-12 of the sums test instead of to the last bit.
    kmax = 200: lists of more than 128 columns, i.e. the wave-per-user evaluation sums inside the captured graph."""
    if not graph:
        monkeypatch.setenv("LLMREC_EVAL_GRAPH", "0")
    g = GoldenCase("nf_tiny")
    Ks = [10, 20, 50, kmax]
    m = load_dropin(golden_argv(g) + ["--Ks", str(Ks), "--test_flag", flag])
    m.set_seed(3)
    tr = m.Trainer(data_config={})
    fused = tr._fused_step()
    assert fused
    users = g.z["eval/users"].tolist()
    r1 = tr.test(users, is_val=False)
    assert len(fused._eval_graphs) == (1 if graph else 0)
    want, want_lists = _oracle_result(m, fused, users, Ks)
    for k in ("precision", "recall", "ndcg", "hit_ratio"):
        assert r1[k].shape == (4,)
        assert np.allclose(r1[k], want[k], rtol=1e-12, atol=0), (k, r1[k], want[k])
    r2 = tr.test(users, is_val=False)                              # the captured evaluation, replayed: the same bits
    for k in ("precision", "recall", "ndcg", "hit_ratio"):
        assert np.array_equal(r1[k], r2[k])
    from llmrec_amd import ops as _ops
    q = torch.tensor(users, device=DEV)
    if graph:
        idx, sc = fused._last_eval[1].clone(), fused._last_eval[2].clone()
        assert idx.shape[1] == kmax
        fused._last_eval[0].replay(); torch.cuda.synchronize()
        assert torch.equal(idx, fused._last_eval[1]) and torch.equal(sc.view(torch.int32), fused._last_eval[2].view(torch.int32))
        eager = _ops.score_topk(fused.E_u, fused.E_i, q, fused._last_eval[4], kmax)
        assert torch.equal(eager[0], idx) and torch.equal(eager[1].view(torch.int32), sc.view(torch.int32))
    else:                                                          # (the eager path returns no lists: the same call Trainer.test made)
        idx, _ = fused.eval_topk(q, m.data_generator.device_state(q.device)["train"], kmax, use_graph=False)
    got = idx.cpu().numpy()                                        # the device's lists are the oracle's lists, item for item
    assert len(want_lists) == len(users)
    for row, top in zip(got, want_lists):
        assert row[:len(top)].tolist() == [int(i) for i in top] and (row[len(top):] == -1).all()
    if flag == "full":                                             # the AUC does not depend on the cut-offs
        m3 = load_dropin(golden_argv(g) + ["--Ks", "[10, 20, 50]", "--test_flag", "full"])
        m3.set_seed(3)
        tr3 = m3.Trainer(data_config={})
        r3 = tr3.test(users, is_val=False)
        assert 0.0 < r1["auc"] < 1.0 and r1["auc"] == r3["auc"] == r2["auc"]
