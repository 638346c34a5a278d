"""The evaluation kernels at every width and table layout their entry points accept, against the contract itself.

llmrec_scores_f32, llmrec_score_topk_f32 / _mode_f32 (exact sweep with and without the workspace, bf16 prefilter and its fallback sweep),
llmrec_score_topk_wide_f32 and llmrec_score_auc_f32 are compared with tests/_eval_ref.py: scores are the bits of the k-ordered fp32 fma chain
(chain_scores, numpy), lists follow (score desc, item id asc) over the items outside the train row (rank) - for 1 <= d <= 128 including every
ragged width class (d % 4 != 0, d % 16 in {1, 15}, every chunk count of both sweeps, the 12-thread pack of (64, 96]) and for tables that
switch the kernels' vector path off through the stride or through the base address. Every table is a view inside a NaN-filled allocation
(_eval_ref.layouts): one element read outside the view poisons a score, one element written there fails Table.check().

Small on purpose: 45 users (three 16-user tiles, the last partial), 700 items (22 item tiles of 32, the last partial), 43 queries."""
import numpy as np
import pytest
import torch

from tests._auc_ref import auc_counts
from tests._eval_ref import chain_scores, layouts, rank

pytestmark = pytest.mark.gpu

DEV = "cuda"
U, I = 45, 700
W = [1, 3, 4, 15, 16, 17, 20, 31, 33, 50, 64, 65, 72, 96, 100, 127, 128]
LAYOUTS = ["contig", "padded", "odd_ld", "shifted"]

# ---- train rows and the query list (the same for every width) ----
_rng = np.random.default_rng(2024)
# four rows that leave K - 7 candidates for K = 20, 56, 64, 100; two dense rows (more than 48 items: the exact sweep's bitmaps); nine rows of at
# most 40 items around the 16-item staged window; 30 empty rows
_SIZES = {5: I - 13, 12: I - 49, 19: I - 57, 26: I - 93, 33: 60, 40: 200, 1: 1, 3: 15, 8: 16, 14: 17, 17: 33, 23: 40, 28: 7, 36: 25, 44: 3}
TRAIN = [sorted(_rng.choice(I, _SIZES.get(u, 0), replace=False).tolist()) for u in range(U)]
_DROPPED = [7, 21, 30]
# the last (partial) user tile holds light rows only (77 train items: the bf16 sweep walks them), the first two hold the dense rows (all 16 rows
# of such a tile as bitmaps); user 12 is listed twice; the table's first and last rows are queried
_TAIL = [44, 1, 8, 14, 23, 0, 2, 4, 6, 9, 10]
_FRONT = [u for u in range(U) if u not in _DROPPED and u not in _TAIL] + [12]
QUERY = [int(u) for u in _rng.permutation(_FRONT)] + [int(u) for u in _rng.permutation(_TAIL)]
assert len(QUERY) == 43 and len(set(QUERY)) == 42 and sum(len(TRAIN[u]) for u in QUERY[32:]) <= 192


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def train(ops):
    return _csr(ops, TRAIN, I)


def _csr(ops, rows, n_items):
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return ops.Csr(len(rows), n_items, torch.from_numpy(rp).to(DEV), torch.from_numpy(ci).to(DEV), None, None, None, ops.SpmmPlan())


# ---- tables and their references, computed once per (kind, d) and shared by every layout and entry ----
_CASES = {}


class _Case:
    def __init__(self, kind, d):
        rng = np.random.default_rng([d, {"normal": 0, "int": 1, "near": 2}[kind]])
        if kind == "int":                        # exact in any order: the ties are real and the id rule alone decides
            self.eu = rng.integers(-2, 3, (U, d)).astype(np.float32)
            self.ei = rng.integers(-1, 2, (I, d)).astype(np.float32)
        elif kind == "near":                     # near-identical item rows (tests/test_gpu_topk_prefilter.py): the bf16 bound cannot separate them
            base = rng.standard_normal(d).astype(np.float32)
            self.ei = base[None, :] + (rng.standard_normal((I, d)) * 1e-4).astype(np.float32)
            self.eu = np.abs(rng.standard_normal((U, d))).astype(np.float32)
        else:
            self.eu = (rng.standard_normal((U, d)) * 0.4).astype(np.float32)
            self.ei = (rng.standard_normal((I, d)) * 0.4).astype(np.float32)
        self.S = chain_scores(self.eu[QUERY], self.ei)             # [43, 700]
        self._rank = {}

    def rank(self, K):
        if K not in self._rank:
            both = [rank(self.S[r], TRAIN[u], K) for r, u in enumerate(QUERY)]
            self._rank[K] = (np.stack([b[0] for b in both]), np.stack([b[1] for b in both]))
        return self._rank[K]


def _case(kind, d):
    if (kind, d) not in _CASES:
        _CASES[(kind, d)] = _Case(kind, d)
    return _CASES[(kind, d)]


def _tables(case, layout):
    d = case.eu.shape[1]
    lu, li = ("shifted", "contig") if layout == "mixed" else (layout, layout)
    return layouts(d)[lu](case.eu, DEV), layouts(d)[li](case.ei, DEV)


def _q():
    return torch.tensor(QUERY, dtype=torch.int64, device=DEV)


def _assert_lists(idx, sc, case, K, what):
    want_i, want_s = case.rank(K)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert idx.shape == sc.shape == (len(QUERY), K)
    if not (np.array_equal(idx, want_i) and np.array_equal(sc, want_s)):
        r = int(np.flatnonzero((idx != want_i).any(1) | ~(sc == want_s).all(1))[0])
        c = int(np.flatnonzero((idx[r] != want_i[r]) | ~(sc[r] == want_s[r]))[0])
        raise AssertionError("%s K=%d: query %d (user %d, %d train items) column %d: got (%d, %r), want (%d, %r)"
                             % (what, K, r, QUERY[r], len(TRAIN[QUERY[r]]), c, idx[r, c], sc[r, c], want_i[r, c], want_s[r, c]))


def _done(*tables):
    torch.cuda.synchronize()
    for t in tables:
        t.check()


def _no_ws(ops, eu, ei, train, K):
    """llmrec_score_topk_f32: no workspace - one block per user tile, the item fragments straight from Ei (the non-packed instances)."""
    from llmrec_amd import _lib
    from llmrec_amd.ops import _ld, _p, _stream
    q = _q()
    idx = torch.full((q.numel(), K), -9, dtype=torch.int32, device=DEV)
    sc = torch.full((q.numel(), K), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("llmrec_score_topk_f32", q.numel(), _p(q), _p(eu.t), _ld(eu.t), _p(ei.t), _ld(ei.t), ei.t.shape[0], eu.t.shape[1],
              _p(train.rowptr), _p(train.colidx), K, _p(idx), _p(sc), _stream())
    return idx, sc


PARAMS = [("normal", d, lay) for d in W for lay in LAYOUTS + ["mixed"]] + [("int", d, lay) for d in (20, 50, 100) for lay in LAYOUTS]
_IDS = ["%s-d%d-%s" % p for p in PARAMS]


@pytest.mark.parametrize("kind,d,layout", PARAMS, ids=_IDS)
def test_scores_are_the_fma_chain(ops, kind, d, layout):
    """scores_kernel<DK>: the anchor of every other comparison of the suite (ops.scores is what the AUC and top-K tests take as the bits)."""
    case = _case(kind, d)
    eu, ei = _tables(case, layout)
    assert ops._rowmajor(eu.t).data_ptr() == eu.t.data_ptr() and ops._ld(eu.t) == eu.ld and ops._ld(ei.t) == ei.ld     # passed through, not copied
    S = ops.scores(eu.t, ei.t, _q())
    _done(eu, ei)
    assert np.array_equal(S.cpu().numpy(), case.S)


@pytest.mark.parametrize("kind,d,layout", PARAMS, ids=_IDS)
def test_exact_sweep_with_workspace(ops, train, kind, d, layout):
    """The packed sweep: score_topk_kernel<DK, true, true> for aligned tables of whole chunks, <DK, false, true> otherwise; the pack launch's tail."""
    case = _case(kind, d)
    eu, ei = _tables(case, layout)
    for K in (1, 20, 64):
        idx, sc = ops.score_topk(eu.t, ei.t, _q(), train, K, mode="exact")
        _done(eu, ei)
        _assert_lists(idx, sc, case, K, "exact, workspace")


@pytest.mark.parametrize("kind,d,layout", PARAMS, ids=_IDS)
def test_exact_sweep_without_workspace(ops, train, kind, d, layout):
    """llmrec_score_topk_f32: score_topk_kernel<DK, true, false> / <DK, false, false>, otherwise only the prefilter's fallback sweep."""
    case = _case(kind, d)
    eu, ei = _tables(case, layout)
    for K in (1, 20, 64):
        idx, sc = _no_ws(ops, eu, ei, train, K)
        _done(eu, ei)
        _assert_lists(idx, sc, case, K, "exact, no workspace")


@pytest.mark.parametrize("kind,d,layout", PARAMS, ids=_IDS)
def test_prefilter(ops, train, kind, d, layout):
    """bf16 sweep + exact re-ranking + verification, against the chain itself (not merely against the exact mode)."""
    case = _case(kind, d)
    eu, ei = _tables(case, layout)
    for K in (1, 20, 56):
        stats = {}
        idx, sc = ops.score_topk(eu.t, ei.t, _q(), train, K, mode="prefilter", stats=stats)
        _done(eu, ei)
        _assert_lists(idx, sc, case, K, "prefilter %s" % stats)


@pytest.mark.parametrize("layout", ["contig", "odd_ld"])
@pytest.mark.parametrize("d", W)
def test_prefilter_fallback_sweep_runs_at_every_width(ops, train, d, layout):
    """Near-identical item rows: more items within the bf16 bound of the K-th score than the 64-slot list has spare, so the verification
    fails and the second launch (the non-packed exact sweep at this width, only for flagged tiles) produces the lists. (Measured on an
    MI355X: all three user tiles are flagged at every width of W, in both layouts and at both K.)"""
    case = _case("near", d)
    eu, ei = _tables(case, layout)
    for K in (20, 56):
        stats = {}
        idx, sc = ops.score_topk(eu.t, ei.t, _q(), train, K, mode="prefilter", stats=stats)
        _done(eu, ei)
        _assert_lists(idx, sc, case, K, "prefilter, near-identical rows %s" % stats)
        assert stats["fallback_tiles"] > 0, (d, layout, K, stats)


@pytest.mark.parametrize("kind,d,layout", PARAMS, ids=_IDS)
def test_wide_rounds(ops, train, kind, d, layout):
    """K = 100: two passes over the gathered user rows ([n_query][d4] copy) in both modes; the first 64 columns are the K = 64 answer."""
    case = _case(kind, d)
    eu, ei = _tables(case, layout)
    i64, s64 = ops.score_topk(eu.t, ei.t, _q(), train, 64, mode="exact")
    for mode in ("exact", "prefilter"):
        idx, sc = ops.score_topk(eu.t, ei.t, _q(), train, 100, mode=mode)
        _done(eu, ei)
        _assert_lists(idx, sc, case, 100, "wide, %s" % mode)
        assert torch.equal(idx[:, :64], i64) and torch.equal(sc[:, :64].view(torch.int32), s64.view(torch.int32)), mode


@pytest.mark.parametrize("d", [1, 3, 17, 50, 127])
def test_wide_rounds_gather_the_user_rows_zero_padded(ops, train, d):
    """The rounds sweep a compact copy of the queried user rows: [n_query][d4] floats (d4 = d rounded up to 4) right behind the single-sweep
    workspace, as include/llmrec_hip.h lays the wide workspace out. Columns d .. d4 - 1 are zeros, never what follows the row in Eu.
    This pins the workspace's layout, not a result: the sweeps guard their user loads by d and never read those columns, so no list can
    show what the gather left there. A change of the layout documented in the header has to change this test with it."""
    from llmrec_amd import _lib
    from llmrec_amd.ops import _ld, _p, _stream
    case = _case("normal", d)
    eu, ei = _tables(case, "shifted")
    q = _q()
    n, K, nnz = q.numel(), 100, sum(len(TRAIN[u]) for u in QUERY)
    nbytes = _lib.query("llmrec_score_topk_wide_workspace_bytes", n, I, d, K, nnz)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFFFFFFFF is a NaN)
    idx = torch.empty(n, K, dtype=torch.int32, device=DEV)
    sc = torch.empty(n, K, dtype=torch.float32, device=DEV)
    _lib.call("llmrec_score_topk_wide_f32", n, _p(q), _p(eu.t), _ld(eu.t), _p(ei.t), _ld(ei.t), I, d, _p(train.rowptr), _p(train.colidx),
              K, _p(idx), _p(sc), _p(ws), nbytes, 0, nnz, _stream())
    _done(eu, ei)
    _assert_lists(idx, sc, case, K, "wide, own workspace")
    d4 = (d + 3) // 4 * 4
    off = (_lib.query("llmrec_score_topk_workspace_bytes", n, I, d) + 255) // 256 * 256
    rows = ws[off:off + 4 * n * d4].view(torch.float32).view(n, d4).cpu().numpy()
    want = np.zeros((n, d4), np.float32)
    want[:, :d] = case.eu[QUERY]
    assert np.array_equal(rows.view(np.int32), want.view(np.int32))


def test_left_over_user_tiles_at_a_ragged_width(ops):
    """4096 + 16 * 57 users: the user tiles beyond the last full round of one tile per compute unit are swept in item parts and merged
    (plan_split), here at d = 50 on tables with an odd leading dimension: equal to the workspace-free sweep for every user, bit for bit, and
    to the chain and the ranking rule for 64 of them."""
    from llmrec_amd import _lib
    from llmrec_amd.ops import _ld, _p, _stream
    n_users, n_items, d, K = 4096 + 16 * 57, 4200, 50, 50
    rng = np.random.default_rng(50)
    eu_h = (rng.standard_normal((n_users, d)) * 0.4).astype(np.float32)
    ei_h = (rng.standard_normal((n_items, d)) * 0.4).astype(np.float32)
    ei_h[::7] = ei_h[3]                                                    # exact ties across the item parts
    deg = rng.integers(0, 12, n_users)
    deg[n_users - 5] = n_items - 20                                        # fewer than K candidates in total
    deg[4100] = 100
    rows = [np.sort(rng.choice(n_items, int(g), replace=False)).tolist() for g in deg]
    tr = _csr(ops, rows, n_items)
    eu, ei = layouts(d)["odd_ld"](eu_h, DEV), layouts(d)["odd_ld"](ei_h, DEV)
    q = torch.arange(n_users, dtype=torch.int64, device=DEV)
    need = _lib.query("llmrec_score_topk_workspace_bytes", n_users, n_items, d)
    assert need > -(-n_items // 32) * 2 * -(-d // 16) * 64 * 16, "more than the packed item table"
    assert _lib.query("llmrec_score_topk_stats_offset", n_users, n_items) > 0, "these shapes leave user tiles over: the part lists precede the fragments"
    out = []
    for ws in (None, torch.empty(need, dtype=torch.uint8, device=DEV)):
        idx = torch.full((n_users, K), -9, dtype=torch.int32, device=DEV)
        sc = torch.full((n_users, K), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("llmrec_score_topk_ws_f32", n_users, _p(q), _p(eu.t), _ld(eu.t), _p(ei.t), _ld(ei.t), n_items, d, _p(tr.rowptr), _p(tr.colidx),
                  K, _p(idx), _p(sc), _p(ws), need if ws is not None else 0, _stream())
        _done(eu, ei)
        out.append((idx, sc))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
    special = [0, 4095, 4096, 4100, n_users - 5, n_users - 1]             # both sides of the split, the dense rows, the table's last row
    sample = special + [int(u) for u in rng.permutation(np.setdiff1d(np.arange(n_users), special))[:58]]
    S = chain_scores(eu_h[sample], ei_h)
    got_i, got_s = out[1][0].cpu().numpy(), out[1][1].cpu().numpy()
    for r, u in enumerate(sample):
        want_i, want_s = rank(S[r], rows[u], K)
        assert np.array_equal(got_i[u], want_i) and np.array_equal(got_s[u], want_s), u
    assert int((got_i[n_users - 5] >= 0).sum()) == 20


# ---- AUC: exact pair counts on tied scores, against the chain (not against ops.scores) ----
_AUC = {}


def _auc_case(d):
    if d not in _AUC:
        rng = np.random.default_rng(d)
        n_users, n_items = 24, 6007                                        # not a multiple of 64
        eu = rng.integers(-2, 3, (n_users, d)).astype(np.float32) / 2
        ei = rng.integers(-2, 3, (n_items, d)).astype(np.float32) / 4
        train_rows, held_rows = [], []
        sizes = [0, 1, 63, 64, 65, 500, 5000, 7, 3, 2]
        for u in range(n_users):
            tr = np.sort(rng.choice(n_items, int(rng.integers(0, 300)), replace=False))
            free = np.setdiff1d(np.arange(n_items), tr)
            h = rng.choice(free, min(sizes[u % len(sizes)], free.size), replace=False)
            h = np.concatenate([h, h[:3], tr[:2], [n_items, n_items + 5]])   # duplicates, train items, ids out of range
            if u == 10:
                tr, h = np.arange(n_items), np.arange(5)                      # every item in train
            if u == 11:
                h = free                                                       # |N| = 0
            train_rows.append(tr)
            held_rows.append(np.sort(h))
        q = list(range(n_users)) + [3, 6, 6]                                   # repeated query users
        S = chain_scores(eu[q], ei)
        want = [auc_counts(S[r], train_rows[u], held_rows[u], n_items) for r, u in enumerate(q)]
        _AUC[d] = (eu, ei, train_rows, held_rows, q, want, sizes)
    return _AUC[d]


@pytest.mark.parametrize("layout", ["padded", "odd_ld", "shifted"])
@pytest.mark.parametrize("d", [16, 48, 96, 128])
def test_auc_counts_on_tied_scores_equal_the_chains(ops, d, layout):
    eu_h, ei_h, train_rows, held_rows, q, want, sizes = _auc_case(d)
    eu, ei = layouts(d)[layout](eu_h, DEV), layouts(d)[layout](ei_h, DEV)
    tr, held = _csr(ops, train_rows, ei_h.shape[0]), _csr(ops, held_rows, ei_h.shape[0])
    auc, cnt = ops.score_auc(eu.t, ei.t, torch.tensor(q, dtype=torch.int64, device=DEV), (tr.rowptr, tr.colidx), (held.rowptr, held.colidx), counts=True)
    _done(eu, ei)
    auc, cnt = auc.cpu().numpy(), cnt.cpu().numpy()
    for r in range(len(q)):
        c2, n_p, n_n, a = want[r]
        assert cnt[r].tolist() == [c2, n_p, n_n] and auc[r] == a, (r, q[r], cnt[r], want[r], auc[r])
    assert cnt[10].tolist() == [0, 0, 0] and cnt[11, 2] == 0 and auc[11] == 0.0
    assert sorted(set(int(c) for c in cnt[:10, 1])) == sorted(sizes)          # every |P| of the list swept


def test_auc_refuses_a_ragged_width(ops):
    rng = np.random.default_rng(20)
    eu = torch.from_numpy(rng.standard_normal((8, 20)).astype(np.float32)).to(DEV)
    ei = torch.from_numpy(rng.standard_normal((100, 20)).astype(np.float32)).to(DEV)
    empty = _csr(ops, [[] for _ in range(8)], 100)
    held = _csr(ops, [[1, 2] for _ in range(8)], 100)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.score_auc(eu, ei, torch.arange(8, device=DEV), (empty.rowptr, empty.colidx), (held.rowptr, held.colidx))
    torch.cuda.synchronize()


# ---- d > 128 is refused before anything is launched ----
@pytest.mark.parametrize("d", [129, 144])
def test_widths_beyond_128_are_refused_before_the_first_launch(ops, train, d):
    from llmrec_amd import _lib
    from llmrec_amd.ops import _ld, _p, _stream
    rng = np.random.default_rng(d)
    eu = torch.from_numpy(rng.standard_normal((U, d)).astype(np.float32)).to(DEV)
    ei = torch.from_numpy(rng.standard_normal((I, d)).astype(np.float32)).to(DEV)
    q = _q()
    n = q.numel()
    nnz = sum(len(TRAIN[u]) for u in QUERY)
    nbytes = _lib.query("llmrec_score_topk_wide_workspace_bytes", n, I, d, 100, nnz)
    assert nbytes >= _lib.query("llmrec_score_topk_workspace_bytes", n, I, d) > 0
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    idx = torch.full((n, 100), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((n, 100), 123.0, dtype=torch.float32, device=DEV)
    S = torch.full((n, I), 123.0, dtype=torch.float32, device=DEV)
    tabs = (n, _p(q), _p(eu), _ld(eu), _p(ei), _ld(ei), I, d)
    csr = (_p(train.rowptr), _p(train.colidx))
    calls = [("llmrec_scores_f32",) + tabs + (_p(S), I, _stream()),
             ("llmrec_score_topk_f32",) + tabs + csr + (50, _p(idx), _p(sc), _stream()),
             ("llmrec_score_topk_ws_f32",) + tabs + csr + (50, _p(idx), _p(sc), _p(ws), nbytes, _stream()),
             ("llmrec_score_topk_mode_f32",) + tabs + csr + (50, _p(idx), _p(sc), _p(ws), nbytes, 0, _stream()),
             ("llmrec_score_topk_mode_f32",) + tabs + csr + (50, _p(idx), _p(sc), _p(ws), nbytes, 1, _stream()),
             ("llmrec_score_topk_wide_f32",) + tabs + csr + (100, _p(idx), _p(sc), _p(ws), nbytes, 0, nnz, _stream()),
             ("llmrec_score_topk_wide_f32",) + tabs + csr + (100, _p(idx), _p(sc), _p(ws), nbytes, 1, nnz, _stream())]
    for call in calls:
        with pytest.raises(RuntimeError, match="unsupported|> 128"):
            _lib.call(*call)
        assert _lib.load().llmrec_last_error().decode().endswith("d = %d > 128" % d), call[0]
    for mode in ("exact", "prefilter"):
        for K in (50, 100):
            with pytest.raises(RuntimeError):
                ops.score_topk(eu, ei, q, train, K, mode=mode)
    with pytest.raises(RuntimeError):
        ops.scores(eu, ei, q)
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all()), "a refused call wrote the workspace"
    assert bool((idx == -7).all()) and bool((sc == 123.0).all()) and bool((S == 123.0).all()), "a refused call wrote an output"
    for call in (("llmrec_scores_f32", n, _p(q), _p(eu), _ld(eu), _p(ei), _ld(ei), I, 0, _p(S), I, _stream()),
                 ("llmrec_score_topk_f32", n, _p(q), _p(eu), _ld(eu), _p(ei), _ld(ei), I, 0) + csr + (50, _p(idx), _p(sc), _stream())):
        with pytest.raises(RuntimeError):                                  # d = 0 is still a bad size
            _lib.call(*call)
