"""GPU: recommending under an item allow-list - llmrec_item_filter_build / llmrec_score_topk_filtered_f32 (csrc/serve.hip) through
ops.ItemFilter / ops.score_topk_filtered, llmrec_amd.serve.Recommender and recommend.py. No tolerance anywhere: the expected list of a
user is the candidates (eligible items outside the train row) ordered by (score desc, item id asc) over the bits ops.scores returns -
two stable sorts on the device, as tests/test_gpu_topk_wide.py orders them -, and ids and score bits are compared with torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import _lib
from tests import _serve_ref as R
from tests._dropin import ROOT, golden_argv
from tests.conftest import GoldenCase

DEV = "cuda"
KS = (1, 20, 56, 64, 65, 130)
MODES = (None, "exact", "prefilter")
TILE = _lib.CONST["LLMREC_FILTER_TILE"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


def _csr(ops, rows, cols, U, I):
    rp, ci, _ = ops.csr_from_coo(torch.as_tensor(rows, dtype=torch.int64).to(DEV), torch.as_tensor(cols, dtype=torch.int64).to(DEV), None, U, I)
    return ops.Csr(U, I, rp, ci, None, None, None, ops.SpmmPlan())


def _train_csr(ops, U, I, rng, max_deg, duplicates=0, full_user=None):
    degs = rng.integers(0, max_deg + 1, size=U)
    rows = np.repeat(np.arange(U), degs)
    cols = np.concatenate([rng.choice(I, size=int(dg), replace=False) for dg in degs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    if duplicates and rows.size:                                   # llmrec_csr_build keeps repeated pairs: the compact mask must keep them too
        pick = rng.integers(0, rows.size, duplicates)
        rows, cols = np.concatenate([rows, rows[pick]]), np.concatenate([cols, cols[pick]])
    if full_user is not None:                                      # a train row that holds every item, so every eligible one under any mask
        keep = rows != full_user
        rows, cols = np.concatenate([rows[keep], np.full(I, full_user)]), np.concatenate([cols[keep], np.arange(I)])
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


def _expected(S, masked, kmax, check_rows=()):
    """([n, kmax] int32 ids, [n, kmax] float32 scores) from the score block S (left unchanged) and the [n, I] matrix of the pairs set
    aside (ineligible or train): candidates by (score desc, id asc), -1 / -inf behind the last candidate."""
    n, I = S.shape
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
    assert gi.shape == (wi.shape[0], K) and gs.shape == gi.shape and gi.dtype == torch.int32, what
    same_i = torch.equal(gi, wi[:, :K])
    same_s = torch.equal(gs.view(torch.int32), ws[:, :K].contiguous().view(torch.int32))
    if not (same_i and same_s):
        bad = (gi != wi[:, :K]).nonzero()
        raise AssertionError("%s: %d ids differ (first %s), score bits equal: %s" % (what, bad.shape[0], bad[:3].tolist(), same_s))


def _assert_empty(got, what=""):
    assert (got[0] == -1).all() and torch.isneginf(got[1]).all(), what


def _allow_masks(I, rng):
    half = (rng.random(I) < 0.5).astype(np.uint8)
    few = (rng.random(I) < 0.03).astype(np.uint8)
    block = np.zeros(I, np.uint8); block[1000:2000] = 1
    first = np.zeros(I, np.uint8); first[0] = 1
    last = np.zeros(I, np.uint8); last[I - 1] = 1
    odd_bytes = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=I)
    return {"all": np.ones(I, np.uint8), "none": np.zeros(I, np.uint8), "item 0": first, "item I-1": last, "half": half, "3 %": few,
            "block": block, "bytes 0/1/255": odd_bytes}


FULL_USER = 5


@pytest.mark.parametrize("d", [64, 128, 20])
def test_small_shape_every_mask_cutoff_and_mode(ops, d):
    rng = np.random.default_rng(900 + d)
    U, I = 211, 3000
    Eu = torch.tensor((rng.standard_normal((U, d)) * 0.4).astype(np.float32)).to(DEV)
    Ei = torch.tensor((rng.standard_normal((I, d)) * 0.4).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 60, duplicates=200, full_user=FULL_USER)
    qn = np.concatenate([rng.permutation(U)[:180], rng.integers(0, U, 23)])    # 203 queries: unsorted, users listed twice, not a multiple of 16
    qn[17] = qn[200] = FULL_USER
    q = torch.tensor(qn).to(DEV)
    S = ops.scores(Eu, Ei, q)                                      # once: every expected list below is cut from these bits
    seen = {True: _masked(q, train, I), False: _masked(q, None, I)}
    for name, allow_np in _allow_masks(I, rng).items():
        allow = torch.tensor(allow_np).to(DEV)
        filt = ops.ItemFilter(allow)
        assert filt.n_kept == int((allow_np != 0).sum()) == int(filt.n_kept_dev.item())
        for with_train in (True, False):
            tr = train if with_train else None
            want = _expected(S, seen[with_train] | (allow == 0)[None, :], max(KS), check_rows=(0, 17, 202))
            for K in KS:
                for mode in MODES:
                    what = "d = %d, allow %s, K = %d, mode %s, train %s" % (d, name, K, mode, with_train)
                    got = ops.score_topk_filtered(Eu, Ei, q, tr, K, filt, mode=mode)
                    _assert_lists(got, want, K, what)
                    if name == "all":                              # the unfiltered call's lists, bit for bit
                        ref = ops.score_topk(Eu, Ei, q, tr, K, mode=mode)
                        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), what
                    if name == "none":
                        _assert_empty(got, what)
                    if with_train:                                 # the user whose train row holds every eligible item
                        _assert_empty((got[0][[17, 200]], got[1][[17, 200]]), what)
            if name == "3 %":
                assert filt.n_kept < 130 and (want[0][:, 129] == -1).all() and (want[0][:, 0] >= 0).any()      # fewer candidates than K
    # filt=None forwards to score_topk
    a, b = ops.score_topk_filtered(Eu, Ei, q, train, 20, None), ops.score_topk(Eu, Ei, q, train, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    with pytest.raises(RuntimeError, match="1024"):
        ops.score_topk_filtered(Eu, Ei, q, train, 1025, filt)
    with pytest.raises(RuntimeError, match="covers"):
        ops.score_topk_filtered(Eu, Ei[:100].contiguous(), q, None, 20, filt)


def test_views_with_a_wider_leading_dimension(ops):
    """any ld >= d: column views of wider tables give the bits of their contiguous copies."""
    rng = np.random.default_rng(3)
    U, I, d = 50, 700, 24
    Eu_w = torch.tensor(rng.standard_normal((U, 40)).astype(np.float32)).to(DEV)
    Ei_w = torch.tensor(rng.standard_normal((I, 37)).astype(np.float32)).to(DEV)
    q = torch.tensor(rng.permutation(U)).to(DEV)
    filt = ops.ItemFilter(torch.tensor((rng.random(I) < 0.4).astype(np.uint8)).to(DEV))
    got = ops.score_topk_filtered(Eu_w[:, 3:3 + d], Ei_w[:, 5:5 + d], q, None, 70, filt)
    ref = ops.score_topk_filtered(Eu_w[:, 3:3 + d].contiguous(), Ei_w[:, 5:5 + d].contiguous(), q, None, 70, filt)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)) and (got[0][:, 0] >= 0).all()


def _scan_patterns(I, rng):
    rnd = lambda: (rng.random(I) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=I)
    empty_block = rnd(); empty_block[TILE:2 * TILE] = 0
    full_block = rnd(); full_block[2 * TILE:3 * TILE] = 1
    tail_only = np.zeros(I, np.uint8); tail_only[3 * TILE + np.array([0, 5, 36])] = 255
    both = rnd(); both[0:TILE] = 0; both[TILE:2 * TILE] = 7
    return {"a block empty": empty_block, "a block full": full_block, "only the ragged tail": tail_only, "first empty, second full": both,
            "all": np.ones(I, np.uint8), "none": np.zeros(I, np.uint8)}


def test_scan_over_several_blocks(ops):
    rng = np.random.default_rng(2048)
    I, d, n = 3 * TILE + 37, 16, 40
    Eu = torch.tensor(rng.standard_normal((64, d)).astype(np.float32)).to(DEV)
    Ei = torch.tensor(rng.standard_normal((I, d)).astype(np.float32)).to(DEV)
    train = _train_csr(ops, 64, I, rng, 30)
    q = torch.tensor(rng.integers(0, 64, n)).to(DEV)
    S = ops.scores(Eu, Ei, q)
    seen = _masked(q, train, I)
    for name, allow_np in _scan_patterns(I, rng).items():
        allow = torch.tensor(allow_np).to(DEV)
        filt = ops.ItemFilter(allow)
        new_id, old_id, n_kept = R.id_maps(allow_np)
        assert filt.n_kept == n_kept, name
        assert np.array_equal(filt.new_id.cpu().numpy(), new_id), name
        assert np.array_equal(filt.old_id.cpu().numpy()[:n_kept], old_id), name
        again = ops.ItemFilter(allow)                              # deterministic
        assert torch.equal(again.new_id, filt.new_id) and torch.equal(again.old_id[:n_kept], filt.old_id[:n_kept])
        want = _expected(S, seen | (allow == 0)[None, :], 70, check_rows=(0, 39))
        for K in (20, 70):
            _assert_lists(ops.score_topk_filtered(Eu, Ei, q, train, K, filt), want, K, "%s, K = %d" % (name, K))
    b = ops.ItemFilter(torch.tensor([True, False, True], device=DEV))      # a bool mask is its bytes
    assert b.new_id.tolist() == [0, -1, 1] and b.n_kept == 2


def _call(ops, Eu, Ei, q, train, K, filt, nnz, n_kept, ws, mode=1):
    n, d = q.numel(), Eu.shape[1]
    idx = torch.zeros(n, K, dtype=torch.int32, device=DEV)
    sc = torch.zeros(n, K, device=DEV)
    _lib.call("llmrec_score_topk_filtered_f32", n, q.data_ptr(), Eu.data_ptr(), d, Ei.data_ptr(), d, Ei.shape[0], d,
              train.rowptr.data_ptr() if train is not None else None, train.colidx.data_ptr() if train is not None else None,
              K, idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel(), mode, nnz, filt.new_id.data_ptr(), filt.old_id.data_ptr(),
              filt.n_kept_dev.data_ptr(), n_kept, None)
    torch.cuda.synchronize()
    return idx, sc


def _error_case(ops, seed=41):
    rng = np.random.default_rng(seed)
    U, I, d = 64, 2000, 64
    Eu = torch.tensor(rng.standard_normal((U, d)).astype(np.float32)).to(DEV)
    Ei = torch.tensor(rng.standard_normal((I, d)).astype(np.float32)).to(DEV)
    train = _train_csr(ops, U, I, rng, 50, duplicates=40)
    q = torch.tensor(np.concatenate([rng.permutation(U), rng.integers(0, U, 9)])).to(DEV)
    allow_np = (rng.random(I) < 0.4).astype(np.uint8)
    return Eu, Ei, train, q, allow_np, ops.ItemFilter(torch.tensor(allow_np).to(DEV))


@pytest.mark.parametrize("K", [20, 100])
def test_the_compact_mask_rows_on_the_device(ops, K):
    Eu, Ei, train, q, allow_np, filt = _error_case(ops)
    n, I, d = q.numel(), Ei.shape[0], Eu.shape[1]
    new_id, _, n_kept = R.id_maps(allow_np)
    want_rp, want_ci = R.mask_rows(train.rowptr.cpu().numpy(), train.colidx.cpu().numpy(), q.cpu().numpy(), new_id)
    nnz = ops._wide_train_nnz(train, q)
    assert 0 < len(want_ci) < nnz                                  # the filter drops entries, and keeps some
    assert any(np.any(np.diff(want_ci[a:b]) == 0) for a, b in zip(want_rp[:-1], want_rp[1:]))      # a duplicated pair survives
    for cap in (nnz, len(want_ci)):                                # the exact capacity is enough
        ws = ops.topk_filtered_workspace(n, I, n_kept, DEV, d, K, cap)
        ws.fill_(0xEE)
        got = _call(ops, Eu, Ei, q, train, K, filt, cap, n_kept, ws)
        off = _lib.query("llmrec_score_topk_filtered_mask_offset", n, I, n_kept, d, K, cap)
        rp = ws[off:off + 4 * (n + 1)].view(torch.int32).cpu().numpy()
        ci = ws[off + R.A(4 * (n + 1)):off + R.A(4 * (n + 1)) + 4 * len(want_ci)].view(torch.int32).cpu().numpy()
        assert np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci)
        assert all(np.all(np.diff(ci[a:b]) >= 0) for a, b in zip(rp[:-1], rp[1:]))                   # ascending rows
        want = _expected(ops.scores(Eu, Ei, q), _masked(q, train, I) | torch.tensor(allow_np == 0).to(DEV)[None, :], K)
        _assert_lists(got, want, K, "capacity %d" % cap)


@pytest.mark.parametrize("K", [20, 100])
def test_caller_errors_come_back_as_empty_lists(ops, K):
    Eu, Ei, train, q, allow_np, filt = _error_case(ops, seed=43)
    n, I, d = q.numel(), Ei.shape[0], Eu.shape[1]
    new_id, _, n_kept = R.id_maps(allow_np)
    _, want_ci = R.mask_rows(train.rowptr.cpu().numpy(), train.colidx.cpu().numpy(), q.cpu().numpy(), new_id)
    nnz = ops._wide_train_nnz(train, q)
    need = max(_lib.query("llmrec_score_topk_filtered_workspace_bytes", n, I, c, d, K, nnz) for c in (n_kept - 1, n_kept, n_kept + 1))
    assert need == _lib.query("llmrec_score_topk_filtered_workspace_bytes", n, I, n_kept + 1, d, K, nnz)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)          # sized for the larger count
    for mode in (0, 1):
        for tr in (train, None):
            for wrong in (n_kept - 1, n_kept + 1):
                _assert_empty(_call(ops, Eu, Ei, q, tr, K, filt, nnz, wrong, ws, mode), "n_kept %+d" % (wrong - n_kept))
            assert (_call(ops, Eu, Ei, q, tr, K, filt, nnz, n_kept, ws, mode)[0][:, 0] >= 0).all()      # the true count: lists
        # a mask that outgrows train_nnz
        small = ops.topk_filtered_workspace(n, I, n_kept, DEV, d, K, len(want_ci) - 1)
        _assert_empty(_call(ops, Eu, Ei, q, train, K, filt, len(want_ci) - 1, n_kept, small, mode), "train_nnz too small")
        _assert_empty(_call(ops, Eu, Ei, q, train, K, filt, 0, n_kept, ops.topk_filtered_workspace(n, I, n_kept, DEV, d, K, 0), mode), "train_nnz 0")
    # through ops: a caller's bound that is too small
    _assert_empty(ops.score_topk_filtered(Eu, Ei, q, train, K, filt, train_nnz=len(want_ci) - 1))
    # a filter without an eligible item: the host count 0 launches no sweep
    none = ops.ItemFilter(torch.zeros(I, dtype=torch.uint8, device=DEV))
    assert none.n_kept == 0
    _assert_empty(_call(ops, Eu, Ei, q, train, K, none, nnz, 0, torch.empty(16, dtype=torch.uint8, device=DEV)))


@pytest.mark.parametrize("K", [20, 100])
def test_one_capture_on_one_stream(ops, K):
    Eu, Ei, train, q, allow_np, filt = _error_case(ops, seed=47)
    n, I, d = q.numel(), Ei.shape[0], Eu.shape[1]
    nnz = ops._wide_train_nnz(train, q)
    ws = ops.topk_filtered_workspace(n, I, filt.n_kept, DEV, d, K, nnz)
    run = lambda: ops.score_topk_filtered(Eu, Ei, q, train, K, filt, train_nnz=nnz, ws=ws)
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
    assert torch.equal(out[0], first[0]) and torch.equal(out[1].view(torch.int32), first[1].view(torch.int32))
    Ei.copy_(torch.flip(Ei, dims=(0,)) * 1.5)                      # the table moves in place; the graph reads it at replay
    g.replay()
    torch.cuda.synchronize()
    eager = ops.score_topk_filtered(Eu, Ei, q, train, K, filt)
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1].view(torch.int32), eager[1].view(torch.int32))
    assert not torch.equal(out[0], first[0])
    want = _expected(ops.scores(Eu, Ei, q), _masked(q, train, I) | torch.tensor(allow_np == 0).to(DEV)[None, :], K)
    _assert_lists(out, want, K, "replay")


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end on tests/golden/nf_tiny (96 users x 80 items)
# ---------------------------------------------------------------------------------------------------------------------------------
FLAGS = ["--batch_size", "64", "--lr", "0.01"]
ENVS = {"graph": {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1"}, "modular": {"LLMREC_FUSED": "0", "LLMREC_GRAPH": "0"}}


def _trainer(monkeypatch, path, ckpt=None):
    from llmrec_amd import checkpoint as C
    from tests._step_env import fused_trainer
    g = GoldenCase("nf_tiny")
    for k in C.CHECKPOINT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if ckpt is not None:
        monkeypatch.setenv("LLMREC_CHECKPOINT", str(ckpt))
    b = fused_trainer(monkeypatch, golden_argv(g) + FLAGS + ["--epoch", "2"], ENVS[path], seed=g.args["seed"])
    b.m._progress = lambda it: it
    return b


def _train_and_reload(monkeypatch, path, tmp_path):
    """Two epochs with LLMREC_CHECKPOINT, then a FRESH trainer (nothing loaded yet) and the path of best.ckpt."""
    a = _trainer(monkeypatch, path, ckpt=tmp_path)
    a.trainer.train()
    del a
    best = str(tmp_path / "best.ckpt")
    if not os.path.exists(best):
        pytest.fail("the recall never rose above 0 in 2 epochs: no best.ckpt, this case shows nothing")
    return _trainer(monkeypatch, path), best


def _brute_force(ops, rec, q, train, allow, k):
    masked = _masked(q, train, rec.n_items)
    if allow is not None:
        masked = masked | (allow == 0)[None, :]
    return _expected(ops.scores(rec.E_u, rec.E_i, q), masked, k, check_rows=(0,))


@pytest.mark.parametrize("path", list(ENVS))
def test_recommend_from_a_checkpoint(ops, path, monkeypatch, tmp_path):
    from llmrec_amd.serve import Recommender
    f, best = _train_and_reload(monkeypatch, path, tmp_path)
    tr = f.trainer
    rec = Recommender.from_checkpoint(tr, best)
    users = list(f.m.data_generator.test_set.keys())
    st = f.m.data_generator.device_state(DEV)
    q = torch.tensor(users, dtype=torch.int64).to(DEV)
    n = len(users)
    assert (rec.n_users, rec.n_items) == (96, 80) and rec.train is st["train"]
    items, scores = rec.recommend(users, 50)
    assert items.dtype == torch.int64 and items.shape == (n, 50) and scores.dtype == torch.float32
    if path == "graph":
        from llmrec_amd.fused import FusedStep
        assert isinstance(tr._fused, FusedStep)
        assert rec.E_u.data_ptr() != tr._fused.E_u.data_ptr()      # clones
        idx, sc = tr._fused.eval_topk(q, st["train"], 50, use_graph=False)
        assert torch.equal(items, idx.long()) and torch.equal(scores.view(torch.int32), sc.view(torch.int32))
        ret = tr.test(users, is_val=False)
        Ks = eval(f.m.args.Ks)
        sums = ops.topk_eval_sums(items.to(torch.int32), q, st["test"][0], st["test"][1], Ks).cpu().numpy() / n
        for j, name in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            assert (sums[j] == np.asarray(ret[name])).all(), name
        assert ret["recall"][-1] > 0
    else:
        assert tr._fused is False
    want = _brute_force(ops, rec, q, st["train"], None, 50)
    assert torch.equal(items, want[0].long()) and torch.equal(scores.view(torch.int32), want[1].view(torch.int32))
    # the even item ids allowed
    even = list(range(0, 80, 2))
    allow = torch.zeros(80, dtype=torch.uint8, device=DEV); allow[::2] = 1
    got = rec.recommend(users, 50, allow_items=even)
    want = _brute_force(ops, rec, q, st["train"], allow, 50)
    assert torch.equal(got[0], want[0].long()) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    live = got[0] >= 0
    assert live.any() and not ((got[0] % 2 == 1) & live).any()
    assert not (_masked(q, st["train"], 80).gather(1, got[0].clamp(min=0)) & live).any()       # nothing from the train row
    # the same set as a deny list of the odd ids: the cached filter answers
    n_filters = len(rec._filters)
    again = rec.recommend(torch.tensor(users), 50, deny_items=np.arange(1, 80, 2))
    assert torch.equal(again[0], got[0]) and len(rec._filters) == n_filters == 1
    both = rec.recommend(users, 50, allow_items=list(range(40)), deny_items=even)                # allowed and not denied: the odd ids below 40
    allow2 = torch.zeros(80, dtype=torch.uint8, device=DEV); allow2[1:40:2] = 1
    assert torch.equal(both[0], _brute_force(ops, rec, q, st["train"], allow2, 50)[0].long())
    seen = rec.recommend(users, 50, allow_items=even, exclude_seen=False)
    assert torch.equal(seen[0], _brute_force(ops, rec, q, None, allow, 50)[0].long())
    # chunks bound the workspace, not the lists
    everyone = list(range(96)) + users[:7]
    for kw in (dict(), dict(allow_items=even)):
        whole = rec.recommend(everyone, 50, chunk=None, **kw)
        for chunk in (64, 16):
            part = rec.recommend(everyone, 50, chunk=chunk, **kw)
            assert torch.equal(part[0], whole[0]) and torch.equal(part[1].view(torch.int32), whole[1].view(torch.int32)), (chunk, kw)
    with pytest.raises(ValueError, match=r"\[0, 80\)"):
        rec.recommend(users, 10, allow_items=[80])
    with pytest.raises(ValueError, match=r"\[0, 96\)"):
        rec.recommend([96], 10)


def test_the_script_in_a_fresh_process(ops, monkeypatch, tmp_path):
    from llmrec_amd import checkpoint as C
    from llmrec_amd.serve import Recommender
    from llmrec_amd.step_options import ENV_SWITCHES, TRAINER_SWITCHES
    f, best = _train_and_reload(monkeypatch, "graph", tmp_path)
    rng = np.random.default_rng(1)
    users = rng.integers(0, 96, 70)
    allow = np.sort(rng.choice(80, size=45, replace=False))
    (tmp_path / "users.txt").write_text("".join("%d\n" % u for u in users))
    np.save(str(tmp_path / "allow.npy"), allow.astype(np.int64))
    out = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES + TRAINER_SWITCHES + tuple(C.CHECKPOINT_SWITCHES)}
    env.update(ENVS["graph"])
    argv = golden_argv(GoldenCase("nf_tiny")) + FLAGS + ["--epoch", "2"]
    cmd = [sys.executable, os.path.join(ROOT, "recommend.py"), "--checkpoint", best, "--users", str(tmp_path / "users.txt"), "--topk", "20",
           "--allow_items", str(tmp_path / "allow.npy"), "--out", out]
    r = subprocess.run(cmd + argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    rec = Recommender.from_checkpoint(f.trainer, best)
    items, scores = rec.recommend(users, 20, allow_items=allow)
    assert np.array_equal(z["users"], users) and z["items"].dtype == np.int64 and z["scores"].dtype == np.float32
    assert np.array_equal(z["items"], items.cpu().numpy()) and np.array_equal(z["scores"].view(np.uint32), scores.cpu().numpy().view(np.uint32))
    assert (z["items"][:, 0] >= 0).all() and np.isin(z["items"][z["items"] >= 0], allow).all()
    assert not os.path.exists(str(tmp_path / "logs"))              # (--debug: no log file)
    # a masking configuration is refused before anything is built
    r = subprocess.run(cmd + argv + ["--mask_rate", "0.1"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "masking round" in r.stderr
