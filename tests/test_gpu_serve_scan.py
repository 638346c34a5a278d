"""GPU: the second tile of block_exclusive_scan (csrc/compact.h), the one scan behind the row pointers of the serving pipeline
(csrc/serve.hip), of the wide call's rounds (csrc/topk_wide.hip) and behind the filter build. A tile is 1024 elements: the calls below
scan 1024, 1025 and 2 * 1024 + 37 queries, and 1026 block counts. No tolerance anywhere: mask rows against the numpy restatements of
tests/_serve_ref.py / tests/_exclude_ref.py, lists against the brute-force expectation cut from the bits of ops.scores."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import _lib
from tests import _exclude_ref as X
from tests import _serve_ref as R
from tests.test_gpu_serve import _assert_empty, _assert_lists, _csr, _expected, _masked

DEV = "cuda"
U, I, D = 64, 300, 16
SCAN_TILE = 1024                                                   # SCAN_THREADS of csrc/compact.h
N_QUERIES = (SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 37)         # a full single tile, the first element of a second, a ragged third
TILE = _lib.CONST["LLMREC_FILTER_TILE"]


def scan_case_numpy():
    """The host side of the case, numpy only: train pairs (about 10 per user, some repeated, user 0 without any), a filter that keeps about
    half of the items, and per number of queries the query list (users repeat) and the exclusion rows (0 - 5 entries, -1 padding and ids
    beyond the table among them)."""
    rng = np.random.default_rng(1024)
    degs = rng.integers(0, 21, size=U)
    degs[0] = 0
    rows = np.repeat(np.arange(U), degs)
    cols = np.concatenate([rng.choice(I, size=int(dg), replace=False) for dg in degs]).astype(np.int64)
    pick = rng.integers(0, rows.size, 60)
    rows, cols = np.concatenate([rows, rows[pick]]), np.concatenate([cols, cols[pick]])
    allow = (rng.random(I) < 0.5).astype(np.uint8)
    queries, excl = {}, {}
    for n in N_QUERIES:
        queries[n] = rng.integers(0, U, n)
        er = [rng.integers(-1, I + 5, size=int(k)) for k in rng.integers(0, 6, size=n)]
        er[n - 1] = np.array([-1, 7, I, 7, I + 4])                 # the last query of the last tile: padding, a repeat, two ids beyond the table
        excl[n] = er
    return rows, cols, allow, queries, excl


def _to_csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.concatenate(rows).astype(np.int32)


def _excluded_matrix(csr, n):
    rp, ci = torch.from_numpy(csr[0]).long().to(DEV), torch.from_numpy(csr[1]).long().to(DEV)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), rp[1:] - rp[:-1])
    ok = (ci >= 0) & (ci < I)
    m = torch.zeros(n, I, dtype=torch.bool, device=DEV)
    m[rows[ok], ci[ok]] = True
    return m


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


class Case:
    def __init__(self, ops):
        rng = np.random.default_rng(16)
        rows, cols, self.allow_np, self.queries, self.excl = scan_case_numpy()
        self.Eu = torch.tensor((rng.standard_normal((U, D)) * 0.4).astype(np.float32)).to(DEV)
        self.Ei = torch.tensor((rng.standard_normal((I, D)) * 0.4).astype(np.float32)).to(DEV)
        self.train = _csr(ops, rows, cols, U, I)
        self.trp, self.tci = self.train.rowptr.cpu().numpy(), self.train.colidx.cpu().numpy()
        self.filt = ops.ItemFilter(torch.tensor(self.allow_np).to(DEV))
        self.new_id = R.id_maps(self.allow_np)[0]
        self.banned = torch.tensor(self.allow_np == 0).to(DEV)[None, :]


@pytest.fixture(scope="module")
def case(ops):
    return Case(ops)


def _mask_in(ws, off, n, n_cols):
    rp = ws[off:off + 4 * (n + 1)].view(torch.int32).cpu().numpy()
    ci = ws[off + R.A(4 * (n + 1)):off + R.A(4 * (n + 1)) + 4 * n_cols].view(torch.int32).cpu().numpy()
    return rp, ci


@pytest.mark.parametrize("n", N_QUERIES)
def test_mask_rows_beyond_one_scan_tile(ops, case, n):
    c = case
    qn = c.queries[n]
    q = torch.tensor(qn).to(DEV)
    csr = _to_csr(c.excl[n])
    excl, ennz = (torch.from_numpy(csr[0]).to(DEV), torch.from_numpy(csr[1]).to(DEV)), len(csr[1])
    nnz = ops._wide_train_nnz(c.train, q)
    S = ops.scores(c.Eu, c.Ei, q)                                  # once: every expected list below is cut from these bits
    seen, gone = _masked(q, c.train, I), _excluded_matrix(csr, n)
    Ks = (20, 70) if n == N_QUERIES[-1] else (20,)                 # K = 70: two rounds of the wide call, whose tw_rowptr_kernel is the same scan

    # (a) the filtered entry under the filter
    want_rp, want_ci = R.mask_rows(c.trp, c.tci, qn, c.new_id)
    assert 0 < len(want_ci) < nnz                                  # the filter drops entries, and keeps some
    assert any(np.any(np.diff(want_ci[a:b]) == 0) for a, b in zip(want_rp[:-1], want_rp[1:]))      # a duplicated pair survives
    assert np.any(np.diff(want_rp) == 0) and want_rp[SCAN_TILE] > 0                                 # an empty mask row; a carry out of the first tile
    want = _expected(S, seen | c.banned, max(Ks), check_rows=(0, n - 1))
    for K in Ks:
        ws = ops.topk_filtered_workspace(n, I, c.filt.n_kept, DEV, D, K, nnz)
        ws.fill_(0xEE)
        got = ops.score_topk_filtered(c.Eu, c.Ei, q, c.train, K, c.filt, train_nnz=nnz, ws=ws)
        rp, ci = _mask_in(ws, _lib.query("llmrec_score_topk_filtered_mask_offset", n, I, c.filt.n_kept, D, K, nnz), n, len(want_ci))
        assert np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci), ("filtered", K)
        _assert_lists(got, want, K, "filtered, n = %d, K = %d" % (n, K))
    if n == N_QUERIES[-1]:                                         # a mask that outgrows train_nnz: the zeroing loop runs across the tiles too
        small = len(want_ci) - 1
        ws = ops.topk_filtered_workspace(n, I, c.filt.n_kept, DEV, D, 20, small)
        ws.fill_(0xEE)
        _assert_empty(ops.score_topk_filtered(c.Eu, c.Ei, q, c.train, 20, c.filt, train_nnz=small, ws=ws), "train_nnz too small")
        rp, _ = _mask_in(ws, _lib.query("llmrec_score_topk_filtered_mask_offset", n, I, c.filt.n_kept, D, 20, small), n, 0)
        assert not rp.any()

    # (b) the excluded entry without a filter, (c) under the filter
    for name, filt, new_id, banned in (("no filter", None, None, torch.zeros_like(c.banned)), ("filter", c.filt, c.new_id, c.banned)):
        kept = filt.n_kept if filt is not None else I
        want_rp, want_ci = X.merged_rows(c.trp, c.tci, qn, csr[0], csr[1], new_id, n_items=I)
        n_train = int(X.merged_rows(c.trp, c.tci, qn, None, None, new_id, n_items=I)[0][-1])
        assert n_train < len(want_ci) < n_train + ennz             # exclusion entries are merged, and some are dropped
        want = _expected(S, seen | banned | gone, max(Ks), check_rows=(0, n - 1))
        assert not torch.equal(want[0][:, :20], _expected(S, seen | banned, 20)[0])                  # the rows do something
        for K in Ks:
            ws = ops.topk_excluded_workspace(n, I, kept, DEV, D, K, nnz, ennz)
            ws.fill_(0xEE)
            got = ops.score_topk_excluded(c.Eu, c.Ei, q, c.train, K, excl, filt, train_nnz=nnz, ws=ws)
            rp, ci = _mask_in(ws, _lib.query("llmrec_score_topk_excluded_mask_offset", n, I, kept, D, K, nnz, ennz), n, len(want_ci))
            assert np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci), ("excluded", name, K)
            _assert_lists(got, want, K, "excluded, %s, n = %d, K = %d" % (name, n, K))


def filter_build_patterns():
    """{name: allow bytes} over 1026 blocks of LLMREC_FILTER_TILE items: the block counts fill one tile of the scan and two elements of the next"""
    n = SCAN_TILE * TILE + TILE + 5
    rng = np.random.default_rng(1026)
    random = (rng.random(n) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=n)
    late = np.zeros(n, np.uint8); late[SCAN_TILE * TILE:] = 1
    last = np.zeros(n, np.uint8); last[n - 5:] = 1
    return {"random 30 %, bytes 1/2/255": random, "the first 1024 blocks empty, the rest full": late, "only the last 5 items": last}


def test_filter_build_beyond_one_scan_tile_of_block_counts(ops):
    for name, allow_np in filter_build_patterns().items():
        assert -(-allow_np.size // TILE) == SCAN_TILE + 2
        allow = torch.tensor(allow_np).to(DEV)
        filt = ops.ItemFilter(allow)
        new_id, old_id, n_kept = R.id_maps(allow_np)
        assert filt.n_kept == n_kept == int(filt.n_kept_dev.item()) and n_kept > 0, name
        assert np.array_equal(filt.new_id.cpu().numpy(), new_id), name
        assert np.array_equal(filt.old_id.cpu().numpy()[:n_kept], old_id), name
        again = ops.ItemFilter(allow)                              # deterministic
        assert again.n_kept == n_kept and torch.equal(again.new_id, filt.new_id) and torch.equal(again.old_id[:n_kept], filt.old_id[:n_kept]), name
