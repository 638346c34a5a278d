"""GPU: recommending with per-query exclusion lists - llmrec_score_topk_excluded_f32 (csrc/exclude.hip) through ops.score_topk_excluded,
llmrec_amd.serve.Recommender.recommend(exclude=...) and recommend.py --exclude. No tolerance anywhere: the expected list of a query is
the candidates (eligible items outside the train row of its user and outside its own exclusion row) ordered by (score desc, item id asc)
over the bits ops.scores returns - the two stable sorts of tests/test_gpu_serve.py -, and ids and score bits are compared with torch.equal.
The shapes are those of tests/test_gpu_serve.py: 211 users, 3000 items, 203 unsorted queries with users listed twice, train rows with
duplicates, one user whose train row holds every item."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import _lib
from tests import _exclude_ref as X
from tests import _serve_ref as R
from tests._dropin import ROOT, golden_argv
from tests.conftest import GoldenCase
from tests.test_gpu_serve import ENVS, FLAGS, FULL_USER, _assert_empty, _assert_lists, _expected, _masked, _train_and_reload, _train_csr

DEV = "cuda"
KS = (1, 20, 64, 65, 130)
MODES = (None, "exact", "prefilter")
U, I, N_QUERY = 211, 3000, 203
TWICE = 7                                                          # the user of queries 3 and 150, which carry different exclusion rows
KINDS = ("empty", "one id", "63 ids", "64 ids", "65 ids", "700 ids, unsorted, repeats", "every item", "sprinkled with -1 and I + 5", "the train row",
         "only ineligible ids")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


def _allow_masks(rng):
    return {"no filter": None, "all": np.ones(I, np.uint8), "none": np.zeros(I, np.uint8), "half": (rng.random(I) < 0.5).astype(np.uint8),
            "3 %": (rng.random(I) < 0.03).astype(np.uint8)}


def _excl_rows(rng, qn, train, allow_np):
    """One exclusion row per query, query i of kind KINDS[i % 10]: every kind many times in one call."""
    trp, tci = train.rowptr.cpu().numpy(), train.colidx.cpu().numpy()
    banned = np.flatnonzero(allow_np == 0) if allow_np is not None else np.zeros(0, np.int64)
    rows = []
    for i, u in enumerate(qn):
        kind = i % len(KINDS)
        if kind == 0:
            row = np.zeros(0, np.int64)
        elif kind in (1, 2, 3, 4):
            row = rng.choice(I, size=(1, 63, 64, 65)[kind - 1], replace=False)
        elif kind == 5:
            row = rng.integers(0, I, 700)
        elif kind == 6:
            row = rng.permutation(I)
        elif kind == 7:
            row = rng.integers(0, I, 40)
            row[rng.choice(40, 12, replace=False)] = np.tile([-1, I + 5, I], 4)
        elif kind == 8:
            row = tci[trp[u]:trp[u + 1]][::-1]
        else:                                                      # ineligible ids only; without a filter: ids that are no items
            row = rng.choice(banned, size=min(30, banned.size)) if banned.size else np.array([-1, I + 5, I, -7])
        rows.append(np.asarray(row, dtype=np.int64))
    return rows


def _to_csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return rp, ci


def _dev(csr):
    return torch.from_numpy(csr[0]).to(DEV), torch.from_numpy(csr[1]).to(DEV)


def _excluded_matrix(csr, n):
    """[n, I] bool: the pairs (query, item) an exclusion CSR names; entries that are no items are ignored."""
    rp, ci = torch.from_numpy(csr[0]).long().to(DEV), torch.from_numpy(csr[1]).long().to(DEV)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), rp[1:] - rp[:-1])
    ok = (ci >= 0) & (ci < I)
    m = torch.zeros(n, I, dtype=torch.bool, device=DEV)
    m[rows[ok], ci[ok]] = True
    return m


class Case:
    def __init__(self, ops, d, seed):
        rng = np.random.default_rng(seed)
        self.d = d
        self.Eu = torch.tensor((rng.standard_normal((U, d)) * 0.4).astype(np.float32)).to(DEV)
        self.Ei = torch.tensor((rng.standard_normal((I, d)) * 0.4).astype(np.float32)).to(DEV)
        self.train = _train_csr(ops, U, I, rng, 60, duplicates=200, full_user=FULL_USER)
        qn = np.concatenate([rng.permutation(U)[:180], rng.integers(0, U, 23)])      # unsorted, users listed twice, not a multiple of 16
        qn[17] = qn[200] = FULL_USER
        qn[3] = qn[150] = TWICE
        self.qn, self.q = qn, torch.tensor(qn).to(DEV)
        self.S = ops.scores(self.Eu, self.Ei, self.q)              # once: every expected list is cut from these bits
        self.seen = _masked(self.q, self.train, I)
        self.masks = _allow_masks(rng)

    def filt(self, ops, name):
        a = self.masks[name]
        return ops.ItemFilter(torch.tensor(a).to(DEV)) if a is not None else None

    def banned(self, name):
        a = self.masks[name]
        return torch.tensor(a == 0).to(DEV)[None, :] if a is not None else torch.zeros(1, I, dtype=torch.bool, device=DEV)


@pytest.fixture(scope="module")
def case64(ops):
    return Case(ops, 64, 1364)


@pytest.mark.parametrize("d", [64, 20])
def test_brute_force_every_row_kind_filter_cutoff_and_mode(ops, case64, d):
    c = case64 if d == 64 else Case(ops, d, 1300 + d)
    n = N_QUERY
    assert c.q.numel() == n
    for k, name in enumerate(c.masks):
        filt = c.filt(ops, name)
        rows = _excl_rows(np.random.default_rng(100 * d + k), c.qn, c.train, c.masks[name])
        assert not np.array_equal(rows[3], rows[150])              # the user listed twice carries two different rows
        csr = _to_csr(rows)
        excl = _dev(csr)
        want = _expected(c.S, c.seen | c.banned(name) | _excluded_matrix(csr, n), max(KS), check_rows=(0, 3, 5, 150, 202))
        if name in ("no filter", "half"):                          # the rows do something: lists differ from those without them
            plain = _expected(c.S, c.seen | c.banned(name), 20)
            assert not torch.equal(plain[0], want[0][:, :20])
        for K in KS:
            for mode in MODES:
                what = "d = %d, filter %s, K = %d, mode %s" % (d, name, K, mode)
                got = ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, excl, filt, mode=mode)
                _assert_lists(got, want, K, what)
                if name == "none":
                    _assert_empty(got, what)
                every = [i for i in range(n) if i % len(KINDS) == 6] + [17, 200]
                _assert_empty((got[0][every], got[1][every]), what)            # every item excluded, and the user who has seen every item
    with pytest.raises(RuntimeError, match="1024"):
        ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, 1025, excl, None)
    with pytest.raises(RuntimeError, match="covers"):
        ops.score_topk_excluded(c.Eu, c.Ei[:100].contiguous(), c.q, None, 20, excl, filt)
    with pytest.raises(RuntimeError, match="rowptr int32"):
        ops.score_topk_excluded(c.Eu, c.Ei, c.q, None, 20, (excl[0][:-1], excl[1]), None)


def _call(c, train, K, filt, nnz, excl, excl_nnz, ws, ws_bytes=None, mode=1, n_kept=None):
    n, d = c.q.numel(), c.d
    idx = torch.zeros(n, K, dtype=torch.int32, device=DEV)
    sc = torch.zeros(n, K, device=DEV)
    maps = (filt.new_id.data_ptr(), filt.old_id.data_ptr(), filt.n_kept_dev.data_ptr()) if filt is not None else (None, None, None)
    kept = n_kept if n_kept is not None else (filt.n_kept if filt is not None else I)
    _lib.call("llmrec_score_topk_excluded_f32", n, c.q.data_ptr(), c.Eu.data_ptr(), d, c.Ei.data_ptr(), d, I, d,
              train.rowptr.data_ptr() if train is not None else None, train.colidx.data_ptr() if train is not None else None,
              K, idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, mode, nnz,
              excl[0].data_ptr() if excl is not None else None, excl[1].data_ptr() if excl is not None and excl_nnz else None, excl_nnz,
              *maps, kept, None)
    torch.cuda.synchronize()
    return idx, sc


@pytest.mark.parametrize("K", [20, 100])
def test_the_merged_mask_rows_on_the_device(ops, case64, K):
    c = case64
    n, d = N_QUERY, c.d
    trp, tci = c.train.rowptr.cpu().numpy(), c.train.colidx.cpu().numpy()
    for name in ("no filter", "half", "all"):
        filt = c.filt(ops, name)
        rows = _excl_rows(np.random.default_rng(5), c.qn, c.train, c.masks[name])
        csr = _to_csr(rows)
        new_id = R.id_maps(c.masks[name])[0] if c.masks[name] is not None else None
        want_rp, want_ci = X.merged_rows(trp, tci, c.qn, csr[0], csr[1], new_id, n_items=I)
        kept = filt.n_kept if filt is not None else I
        n_train = int(X.merged_rows(trp, tci, c.qn, None, None, new_id, n_items=I)[0][-1])
        ennz = len(csr[1])
        assert any(np.any(np.diff(want_ci[a:b]) == 0) for a, b in zip(want_rp[:-1], want_rp[1:]))      # duplicates survive
        for cap in (ops._wide_train_nnz(c.train, c.q), n_train):                                          # the exact capacity is enough
            ws = ops.topk_excluded_workspace(n, I, kept, DEV, d, K, cap, ennz)
            ws.fill_(0xEE)
            got = _call(c, c.train, K, filt, cap, _dev(csr), ennz, ws)
            off = _lib.query("llmrec_score_topk_excluded_mask_offset", n, I, kept, d, K, cap, ennz)
            rp = ws[off:off + 4 * (n + 1)].view(torch.int32).cpu().numpy()
            ci = ws[off + R.A(4 * (n + 1)):off + R.A(4 * (n + 1)) + 4 * len(want_ci)].view(torch.int32).cpu().numpy()
            assert np.array_equal(rp, want_rp), (name, cap)
            assert np.array_equal(ci, want_ci), (name, cap)
            want = _expected(c.S, c.seen | c.banned(name) | _excluded_matrix(csr, n), K)
            _assert_lists(got, want, K, "%s, capacity %d" % (name, cap))


@pytest.mark.parametrize("K", [20, 100])
def test_identities(ops, case64, K):
    c = case64
    n = N_QUERY
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    empty = (torch.zeros(n + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    trp, tci = c.train.rowptr.cpu().numpy(), c.train.colidx.cpu().numpy()
    as_rows = _dev(_to_csr([tci[trp[u]:trp[u + 1]] for u in c.qn]))                  # the queried train rows as exclusion rows
    for name in ("no filter", "half"):
        filt = c.filt(ops, name)
        for mode in MODES:
            ref = ops.score_topk_filtered(c.Eu, c.Ei, c.q, c.train, K, filt, mode=mode)
            assert (ref[0][:, 0] >= 0).any()
            assert same(ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, empty, filt, mode=mode), ref), (name, mode)      # every row empty
            assert same(ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, None, filt, mode=mode), ref), (name, mode)       # forwards
            assert same(ops.score_topk_excluded(c.Eu, c.Ei, c.q, None, K, as_rows, filt, mode=mode), ref), (name, mode)       # train rows as lists
            if filt is None:
                assert same(ref, ops.score_topk(c.Eu, c.Ei, c.q, c.train, K, mode=mode))


def test_paging_equals_one_long_list(ops, case64):
    from llmrec_amd.serve import Recommender
    c = case64
    rec = Recommender(c.Eu, c.Ei, c.train)
    users = c.qn.tolist()
    allow = np.flatnonzero(c.masks["half"])
    for kw in (dict(), dict(allow_items=allow), dict(chunk=64), dict(allow_items=allow, exclude_seen=False)):
        whole = rec.recommend(users, 150, **{k: v for k, v in kw.items() if k != "chunk"})
        assert (whole[0][:, 149] >= 0).any() and (whole[0][17] == -1).all() == kw.get("exclude_seen", True)
        pages = [rec.recommend(users, 50, **kw)]
        for _ in range(2):
            shown = torch.cat([p[0] for p in pages], dim=1)        # int64 [n, 50 or 100], -1 behind the last candidate: the [n, m] form
            pages.append(rec.recommend(users, 50, exclude=shown, **kw))
        items, scores = torch.cat([p[0] for p in pages], dim=1), torch.cat([p[1] for p in pages], dim=1)
        assert items.dtype == torch.int64 and torch.equal(items, whole[0]), kw
        assert torch.equal(scores.view(torch.int32), whole[1].view(torch.int32)), kw
    # the other forms of the same lists
    shown = pages[0][0].cpu().numpy()
    want = rec.recommend(users, 50, exclude=pages[0][0], allow_items=allow, exclude_seen=False)
    by_user = {}
    for u, row in zip(users, shown):
        by_user.setdefault(u, row)                                 # (a user's pages are the same at every occurrence)
    csr = _to_csr([r[r >= 0] for r in shown])
    for form in (by_user, [r.tolist() for r in shown], (csr[0], csr[1]), torch.from_numpy(shown).to(DEV)):
        got = rec.recommend(users, 50, exclude=form, allow_items=allow, exclude_seen=False)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), type(form)
    with pytest.raises(ValueError, match=r"\[0, 3000\)"):
        rec.recommend(users, 10, exclude={users[0]: [I]})
    with pytest.raises(ValueError, match="rows"):
        rec.recommend(users, 10, exclude=shown[:-1])


GUARD = 4096


@pytest.mark.parametrize("K", [20, 100])
def test_capacity_errors_come_back_as_empty_lists(ops, case64, K):
    c = case64
    n, d = N_QUERY, c.d
    trp, tci = c.train.rowptr.cpu().numpy(), c.train.colidx.cpu().numpy()
    for name in ("no filter", "half"):
        filt = c.filt(ops, name)
        kept = filt.n_kept if filt is not None else I
        csr = _to_csr(_excl_rows(np.random.default_rng(9), c.qn, c.train, c.masks[name]))
        excl, ennz = _dev(csr), len(csr[1])
        new_id = R.id_maps(c.masks[name])[0] if c.masks[name] is not None else None
        n_train = int(X.merged_rows(trp, tci, c.qn, None, None, new_id, n_items=I)[0][-1])
        decreasing = csr[0].copy(); decreasing[40] = decreasing[41] + 1
        late = csr[0].copy(); late[0] = 1
        cases = {"excl_nnz one below the count": (n_train, excl, ennz - 1), "train_nnz one below the kept entries": (n_train - 1, excl, ennz),
                 "train_nnz 0": (0, excl, ennz), "a decreasing excl_rowptr": (n_train, (torch.from_numpy(decreasing).to(DEV), excl[1]), ennz),
                 "an excl_rowptr that starts at 1": (n_train, (torch.from_numpy(late).to(DEV), excl[1]), ennz)}
        for mode in (0, 1):
            for what, (cap, e, claimed) in cases.items():
                need = _lib.query("llmrec_score_topk_excluded_workspace_bytes", n, I, kept, d, K, cap, claimed)
                ws = torch.full((need + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
                got = _call(c, c.train, K, filt, cap, e, claimed, ws, ws_bytes=need, mode=mode)
                _assert_empty(got, "%s, %s" % (name, what))
                assert (ws[need:] == 0xEE).all(), "%s, %s: written behind the workspace" % (name, what)
            need = _lib.query("llmrec_score_topk_excluded_workspace_bytes", n, I, kept, d, K, n_train, ennz)
            ws = torch.full((need + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
            good = _call(c, c.train, K, filt, n_train, excl, ennz, ws, ws_bytes=need, mode=mode)      # the true counts: lists
            assert (good[0][:, 0] >= 0).any() and (ws[need:] == 0xEE).all()
        if filt is not None:                                       # the hand-shake of the filtered call
            need = max(_lib.query("llmrec_score_topk_excluded_workspace_bytes", n, I, k, d, K, n_train, ennz) for k in (kept - 1, kept, kept + 1))
            ws = torch.full((need + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
            for wrong in (kept - 1, kept + 1):
                _assert_empty(_call(c, c.train, K, filt, n_train, excl, ennz, ws, ws_bytes=need, n_kept=wrong), "n_kept %+d" % (wrong - kept))
            assert (ws[need:] == 0xEE).all()
    # through ops: the column count is the claimed count
    _assert_empty(ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, (excl[0], excl[1][:-1]), None))
    # a filter without an eligible item: the host count 0 launches no sweep and needs no workspace
    none = c.filt(ops, "none")
    assert none.n_kept == 0
    _assert_empty(_call(c, c.train, K, none, n_train, excl, ennz, torch.empty(16, dtype=torch.uint8, device=DEV)))


@pytest.mark.parametrize("K", [20, 100])
def test_one_capture_on_one_stream(ops, case64, K):
    c = case64
    n, d = N_QUERY, c.d
    rng = np.random.default_rng(77)
    nnz = ops._wide_train_nnz(c.train, c.q)
    for name in ("no filter", "half"):
        filt = c.filt(ops, name)
        kept = filt.n_kept if filt is not None else I
        rows = _excl_rows(rng, c.qn, c.train, c.masks[name])
        csr = _to_csr(rows)
        rp, ci = _dev(csr)
        ws = ops.topk_excluded_workspace(n, I, kept, DEV, d, K, nnz, ci.numel())
        run = lambda: ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, (rp, ci), filt, train_nnz=nnz, ws=ws)
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
        assert torch.equal(out[0], first[0]) and torch.equal(out[1].view(torch.int32), first[1].view(torch.int32)), name
        want = _expected(c.S, c.seen | c.banned(name) | _excluded_matrix(csr, n), K)
        _assert_lists(out, want, K, "%s, first replay" % name)
        # other lists in the same buffers: the rows move to other queries, the sizes stay
        perm = rng.permutation(n)
        again = _to_csr([rng.integers(0, I, len(rows[p])) if len(rows[p]) != I else rows[p] for p in perm])
        assert len(again[1]) == ci.numel()
        rp.copy_(torch.from_numpy(again[0])); ci.copy_(torch.from_numpy(again[1]))
        g.replay()
        torch.cuda.synchronize()
        eager = ops.score_topk_excluded(c.Eu, c.Ei, c.q, c.train, K, (rp, ci), filt)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1].view(torch.int32), eager[1].view(torch.int32)), name
        assert not torch.equal(out[0], first[0])
        want = _expected(c.S, c.seen | c.banned(name) | _excluded_matrix(again, n), K)
        _assert_lists(out, want, K, "%s, second replay" % name)


def test_the_script_in_a_fresh_process(ops, monkeypatch, tmp_path):
    """recommend.py --exclude on tests/golden/nf_tiny (96 users x 80 items) against Recommender.recommend(exclude=dict)."""
    from llmrec_amd import checkpoint as C
    from llmrec_amd.serve import Recommender
    from llmrec_amd.step_options import ENV_SWITCHES, TRAINER_SWITCHES
    f, best = _train_and_reload(monkeypatch, "graph", tmp_path)
    rng = np.random.default_rng(2)
    users = rng.integers(0, 96, 70)
    assert len(set(users.tolist())) < 70                           # users listed twice
    pairs = np.stack([rng.integers(0, 96, 900), rng.integers(0, 80, 900)], axis=1)      # with repeats, and users that are not listed
    (tmp_path / "users.txt").write_text("".join("%d\n" % u for u in users))
    (tmp_path / "pairs.txt").write_text("".join("%d %d\n" % (u, i) for u, i in pairs))
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES + TRAINER_SWITCHES + tuple(C.CHECKPOINT_SWITCHES)}
    env.update(ENVS["graph"])
    argv = golden_argv(GoldenCase("nf_tiny")) + FLAGS + ["--epoch", "2"]
    rec = Recommender.from_checkpoint(f.trainer, best)
    by_user = {}
    for u, i in pairs:
        if u in users:
            by_user.setdefault(int(u), []).append(int(i))
    items, scores = rec.recommend(users, 20, exclude=by_user)
    plain = rec.recommend(users, 20)
    assert not torch.equal(items, plain[0])
    for q, u in enumerate(users):
        assert not np.isin(items[q].cpu().numpy(), by_user.get(int(u), [])).any()
    for name in ("pairs.txt",):                                      # (the .npy reader: tests/test_exclude_ref_cpu.py)
        out = str(tmp_path / (name + ".npz"))
        cmd = [sys.executable, os.path.join(ROOT, "recommend.py"), "--checkpoint", best, "--users", str(tmp_path / "users.txt"), "--topk", "20",
               "--exclude", str(tmp_path / name), "--out", out]
        r = subprocess.run(cmd + argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        assert np.array_equal(z["users"], users) and z["items"].dtype == np.int64 and z["scores"].dtype == np.float32
        assert np.array_equal(z["items"], items.cpu().numpy()), name
        assert np.array_equal(z["scores"].view(np.uint32), scores.cpu().numpy().view(np.uint32)), name
