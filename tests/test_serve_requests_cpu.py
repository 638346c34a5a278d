"""CPU: the request logic of llmrec_amd.serve.Recommender and the argument lists of the four served ops wrappers, with no device.

Part A runs the real serve.py on CPU tensors: ops._need_gpu is a no-op, and ops.score_topk_excluded / score_topk_candidates /
score_topk_candidates_capped / fold_in_users / ItemFilter are stand-ins that implement their docstring contracts by brute force and record
every call. Whole requests - chunks, slices, the two quota rounds, dict-keyed lists for repeated users - are compared with an oracle that
computes the request in one go from the request's own Python lists, and the recorded call sequences with tables written out by hand.
All table entries are multiples of 1/2, so every score is exact in fp32 whatever the shape of the product that computed it.

Part B runs the real ops wrappers on CPU tensors with _lib.call / _lib.query recorded, and compares the entry name and the positional
arguments with the parameter order of include/llmrec_hip.h, written out here."""
import itertools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from llmrec_amd import _lib, ops, serve
from tests import _quota_ref as Q

U, I, D = 7, 30, 8
_rng = np.random.default_rng(20261021)
E_U = torch.from_numpy(_rng.integers(-3, 4, (U, D)).astype(np.float32) * 0.5)
E_I = torch.from_numpy(_rng.integers(-3, 4, (I, D)).astype(np.float32) * 0.5)
ID_ROWS = _rng.integers(-2, 3, (5, D)).astype(np.float32) * 0.5
TRAIN_ROWS = [[0, 4], [2, 29], [5, 6], [1, 7, 8], [3], [12, 13], []]                       # user 6: an empty row; user 1 holds the last item
TRAIN_RP = [0, 2, 4, 6, 9, 10, 12, 12]
USERS = [3, 0, 3, 6, 1]                                                                     # user 3 twice
HISTORIES = [[1, 7, 8], [4, 0, 4], [], [29, 2], [9]]                                        # one empty, one with a repeated id
ALLOW, DENY = list(range(0, I, 2)) + [1, 29, 29], [5, 20, 29]
EX_ROWS = [[29, 10, 11, 10], [1, 4], [29, 10, 11, 10], [], [0]]                             # rows 0 and 2 are user 3's: a dict can say them
CAND_ROWS = [[20, 1, 21, 7, 10, 20, 3], [22, 0, 4, 5, 13], [20, 1, 21, 7, 10, 20, 3], [], [5, 6, 2, 29, 14, 15, 16, 17, 9]]
GROUP = [i // 10 for i in range(I)]                                                        # three groups of ten ...
GROUP[1] = GROUP[3] = -1                                                                   # ... and two items of no group
CAPS = {"int": 2, "array": [1, 0, 3]}
CHUNKS, KS = (None, 2, 5, 64), (1, 4, 40)
CALLS = ("recommend", "recommend_new", "rank", "rank_new")


def _train():
    return ops.Csr(U, I, torch.tensor(TRAIN_RP, dtype=torch.int32), torch.tensor(sum(TRAIN_ROWS, []), dtype=torch.int32), None, None, None)


def _forms(rows, keys):
    """The per-query id lists `rows` in every container form exclusion_csr accepts; keys: the dict key of each query."""
    width = max(len(r) for r in rows)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return {"none": None,
            "dict": dict([(k, r) for k, r in zip(keys, rows) if r] + [(5, [2])]),          # (key 5 is no listed query: ignored)
            "csr": (rowptr, np.array(sum(rows, []), dtype=np.int64)),
            "array": np.array([r + [-1] * (width - len(r)) for r in rows]),
            "lists": [list(r) for r in rows]}


# ------------------------------------------------------------------------------------------------------------------------------------
# the stand-ins: the contracts of the ops docstrings on the CPU, every call recorded
# ------------------------------------------------------------------------------------------------------------------------------------
class FakeFilter:
    """ops.ItemFilter without a device: the flags, n_items and n_kept."""

    def __init__(self, allow):
        assert allow.dtype == torch.uint8 and allow.dim() == 1
        self.flags, self.n_items, self.n_kept = allow.clone(), allow.numel(), int((allow != 0).sum())


def _host(csr, n):
    """A device CSR over n queries as host lists, its form checked; None stays None."""
    if csr is None:
        return None
    rowptr, colidx = csr
    assert rowptr.dtype == torch.int32 and colidx.dtype == torch.int32 and rowptr.shape == (n + 1,) and colidx.dim() == 1
    assert rowptr[0] == 0 and colidx.numel() == rowptr[n] and bool((rowptr[1:] >= rowptr[:-1]).all())
    return rowptr.tolist(), colidx.tolist()


def _row(csr, r):
    return () if csr is None else csr[1][csr[0][r]:csr[0][r + 1]]


def _ranked(scores_row, keep, K, walk=None):
    """The K first ids of the set `keep` by (score descending, id ascending), under `walk` the greedy quota walk down that ranking; padded
    with -1 / -inf."""
    order = sorted(keep, key=lambda i: (-float(scores_row[i]), i))
    order = walk(order, K) if walk is not None else order[:K]
    ids = torch.full((K,), -1, dtype=torch.int64)
    sc = torch.full((K,), -np.inf, dtype=torch.float32)
    ids[:len(order)], sc[:len(order)] = torch.tensor(order, dtype=torch.int64), scores_row[order]
    return ids, sc


def _walk(group, cap, n_groups):
    g, caps = Q.group_and_cap(group, n_groups, cap)
    return lambda order, K: Q.greedy(order, g, caps, K)


def _stand_ins(log):
    def ranking(Eu, Ei, q, train, K, cand, excl, filt, walk=None):
        n, n_items = q.numel(), Ei.shape[0]
        assert q.dtype == torch.int64 and Eu.dtype == Ei.dtype == torch.float32 and (filt is None or filt.n_items == n_items)
        S = Eu[q] @ Ei.T
        eligible = set(range(n_items)) if filt is None else set(filt.flags.nonzero().reshape(-1).tolist())
        t = _host((train.rowptr, train.colidx), train.n_rows) if train is not None else None
        idx, sc = torch.empty(n, K, dtype=torch.int32), torch.empty(n, K, dtype=torch.float32)
        for r in range(n):
            keep = (eligible if cand is None else eligible & set(_row(cand, r))) - set(_row(t, int(q[r]))) - set(_row(excl, r))
            idx[r], sc[r] = _ranked(S[r], keep, K, walk)
        return idx, sc

    def score_topk_excluded(Eu, Ei, query_users, train, K, exclude, filt=None, mode=None, train_nnz=None, ws=None):
        e = _host(exclude, query_users.numel())
        log.append(("excluded", query_users.tolist(), K, e, train is not None, filt is not None))
        return ranking(Eu, Ei, query_users, train, K, None, e, filt)

    def score_topk_candidates(Eu, Ei, query_users, train, K, candidates, exclude=None, filt=None, ws=None):
        c, e = _host(candidates, query_users.numel()), _host(exclude, query_users.numel())
        log.append(("candidates", query_users.tolist(), K, c, e, train is not None, filt is not None))
        return ranking(Eu, Ei, query_users, train, K, c, e, filt)

    def score_topk_candidates_capped(Eu, Ei, query_users, train, K, candidates, item_group, cap, exclude=None, filt=None, ws=None, n_groups=None):
        c, e = _host(candidates, query_users.numel()), _host(exclude, query_users.numel())
        assert item_group.dtype == torch.int32 and item_group.shape == (Ei.shape[0],) and 1 <= K <= 1024
        if isinstance(cap, torch.Tensor):
            assert cap.dtype == torch.int32 and (n_groups is None or n_groups == cap.numel())
            cap, n_groups = cap.tolist(), cap.numel()
        elif n_groups is None:
            n_groups = max(int(item_group.max()) + 1, 1)
        log.append(("capped", query_users.tolist(), K, c, e, train is not None, filt is not None, cap, n_groups))
        return ranking(Eu, Ei, query_users, train, K, c, e, filt, _walk(item_group.tolist(), cap, n_groups))

    def fold_in_users(tables, rowptr, colidx, row_scale=None, id_rows=None, out=None, ws=None):
        rp, ci = _host((rowptr, colidx), rowptr.numel() - 1)
        log.append(("fold_in", (rp, ci), None if id_rows is None else id_rows.tolist()))
        rows = [sorted({i for i in ci[a:b] if 0 <= i < tables.n_items}) for a, b in zip(rp[:-1], rp[1:])]
        return _fold(tables.E_i, rows, id_rows)

    return score_topk_excluded, score_topk_candidates, score_topk_candidates_capped, fold_in_users


def _fold(E_i, rows, id_rows):
    """The stand-in's embedding of new users: the id row plus the sum of the E_i rows of the history SET (exact: halves)."""
    E = torch.zeros(len(rows), E_i.shape[1]) if id_rows is None else torch.as_tensor(id_rows, dtype=torch.float32).clone()
    for r, h in enumerate(rows):
        E[r] += E_i[sorted(set(h))].sum(0)
    return E


@pytest.fixture
def served(monkeypatch):
    """(make, log): make(E_u, E_i) a Recommender over CPU tables behind the stand-ins, log the calls they saw."""
    log = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops, "ItemFilter", FakeFilter)
    for f in _stand_ins(log):
        monkeypatch.setattr(ops, f.__name__, f)
    return (lambda E_u=E_U, E_i=E_I: serve.Recommender(E_u, E_i, _train(), fold_in=SimpleNamespace(n_items=I, d=D, E_i=E_i))), log


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle: one whole request from its own Python lists - no CSR, no chunk, no round, no candidate trick
# ------------------------------------------------------------------------------------------------------------------------------------
def _oracle(E_q, E_i, gone, k, allow=None, deny=None, cand=None, cap=None, overfetch=2):
    """(items int64 [n, k], scores float32 [n, k], queries a first round of min(1024, overfetch * k) would leave unsettled). E_q: one
    embedding per query; gone: per query, everything to leave out; cand: per query, the candidate ids, or None = the catalogue."""
    S = E_q @ E_i.T
    eligible = (set(range(I)) if allow is None else set(allow)) - set(deny or ())
    walk = _walk(GROUP, cap, 3) if cap is not None else None
    K1 = min(1024, overfetch * k)
    ids, sc, unsettled = torch.empty(len(gone), k, dtype=torch.int64), torch.empty(len(gone), k, dtype=torch.float32), 0
    for r in range(len(gone)):
        keep = (eligible if cand is None else eligible & set(cand[r])) - set(gone[r])
        ids[r], sc[r] = _ranked(S[r], keep, k, walk)
        if walk is not None:
            prefix, _ = _ranked(S[r], keep, K1)
            unsettled += int(len(walk([i for i in prefix.tolist() if i >= 0], k)) < k and len(keep) >= K1)
    return ids, sc, unsettled


def _request(rec, call, k, seen=True, excl="none", cand="lists", id_rows=False, **kw):
    """One request through the public call `call`, and the oracle's answer to it. seen: exclude_seen / exclude_history; excl, cand: the
    container form of EX_ROWS / CAND_ROWS; kw: allow_items, deny_items, chunk, overfetch, per_group (with group_of = GROUP)."""
    new, ranks = call.endswith("_new"), call.startswith("rank")
    keys = range(len(USERS)) if new else USERS
    args = dict(kw, exclude=_forms(EX_ROWS, keys)[excl], **{"exclude_history" if new else "exclude_seen": seen})
    if "per_group" in kw:
        args["group_of"] = GROUP
    if new and id_rows:
        args["id_rows"] = ID_ROWS
    head = ([HISTORIES] if new else [USERS]) + ([_forms(CAND_ROWS, keys)[cand]] if ranks else [])
    got = getattr(rec, call)(*head, k, **args)
    E_q = _fold(rec.E_i, HISTORIES, ID_ROWS if id_rows else None) if new else rec.E_u[USERS]
    own = HISTORIES if new else [TRAIN_ROWS[u] for u in USERS]
    gone = [(own[r] if seen else []) + (EX_ROWS[r] if excl != "none" else []) for r in range(len(USERS))]
    want = _oracle(E_q, rec.E_i, gone, k, kw.get("allow_items"), kw.get("deny_items"), CAND_ROWS if ranks else None, kw.get("per_group"),
                   kw.get("overfetch", 2))
    return got, want


def _same(got, want, what):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == got[1].shape == want[0].shape, what
    assert torch.equal(got[0], want[0]), (what, got[0], want[0])
    assert torch.equal(got[1], want[1]), (what, got[1], want[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# Part A
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
def test_whole_requests_equal_the_brute_force_oracle(served, call):
    make, log = served
    rec = make()
    filters = [{}, {"allow_items": ALLOW}, {"deny_items": DENY}, {"allow_items": ALLOW, "deny_items": DENY}]
    padded = False
    for chunk, k, form in itertools.product(CHUNKS, KS, ("none", "dict", "csr", "array", "lists")):
        what = (call, chunk, k, form)
        got, want = _request(rec, call, k, excl=form, cand=form if form != "none" else "lists", chunk=chunk, **filters[3])
        _same(got, want, what)
        padded = padded or bool((got[0] < 0).any())
    for f, seen, chunk, id_rows in itertools.product(filters, (True, False), CHUNKS, (False, True) if call.endswith("_new") else (False,)):
        got, want = _request(rec, call, 4, seen=seen, excl="dict", cand="dict", id_rows=id_rows, chunk=chunk, **f)
        _same(got, want, (call, f, seen, chunk, id_rows))
    assert padded and not hasattr(rec, "last_quota")                        # k = 40 > n_items pads; last_quota is set under quotas only
    ranking_ops = {e[0] for e in log} - {"fold_in"}
    assert ranking_ops == ({"candidates"} if call.startswith("rank") else {"excluded"})


@pytest.mark.parametrize("call", CALLS)
def test_no_queries_give_empty_lists(served, call):
    make, log = served
    rec = make()
    head = [[]] * (2 if call.startswith("rank") else 1)                     # no users / no histories, and no candidate lists
    for kw in ({}, {"group_of": GROUP, "per_group": 2}, {"deny_items": DENY, "exclude": {}, "chunk": 2}):
        items, scores = getattr(rec, call)(*head, 4, **kw)
        assert items.dtype == torch.int64 and scores.dtype == torch.float32 and items.shape == scores.shape == (0, 4)
    assert log == []
    if not call.startswith("rank"):
        assert rec.last_quota == {"queries": 0, "round2": 0}


@pytest.mark.parametrize("pairs", (None, I))
@pytest.mark.parametrize("call", CALLS)
def test_quota_lists_do_not_depend_on_overfetch_or_chunk(served, monkeypatch, call, pairs):
    make, log = served
    rec = make()
    if pairs is not None:
        monkeypatch.setattr(serve, "ROUND2_PAIRS", pairs)                   # round 2 goes one query per call
    sweeps, new = call.startswith("recommend"), call.endswith("_new")
    second_round = most = 0
    for cap, k in itertools.product(CAPS.values(), KS):
        first = None
        for overfetch, chunk in itertools.product((1, 2, 8) if sweeps else (None,), CHUNKS):
            del log[:]
            kw = {"overfetch": overfetch} if sweeps else {}
            got, want = _request(rec, call, k, excl="dict", cand="array", chunk=chunk, deny_items=DENY, per_group=cap, **kw)
            what = (call, cap, k, overfetch, chunk)
            _same(got, want, what)
            first = first or got
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), what
            if sweeps:
                assert rec.last_quota == {"queries": len(USERS), "round2": want[2]}, what
                capped = [e for e in log if e[0] == "capped"]
                whole = [e for e in capped if e[3][1] == list(range(I)) * len(e[1])]        # round 2: the catalogue as every candidate row
                assert all(e[4] is not None and e[5:7] == (not new, True) for e in whole), what           # with exclusion rows, train, filter
                assert all(e[4:7] == (None, False, False) for e in capped if e not in whole), what        # round 1: the fetched rows alone
                assert sum(len(e[1]) for e in whole) == want[2] and (pairs is None or all(len(e[1]) == 1 for e in whole)), what
                second_round, most = second_round + len(whole), max(most, len(whole))
            else:
                assert {e[0] for e in log} - {"fold_in"} == {"capped"}, what
    if sweeps:
        assert second_round > 0 and (pairs is None or most > 1)             # round 2 happened, with pairs patched in several calls


RANGE = list(range(I))


def test_call_sequence_recommend(served):
    make, log = served
    make().recommend(USERS, 4, deny_items=[5], exclude={3: [10, 11]}, chunk=2)
    assert log == [("excluded", [3, 0], 4, ([0, 2, 2], [10, 11]), True, True),
                   ("excluded", [3, 6], 4, ([0, 2, 2], [10, 11]), True, True),
                   ("excluded", [1], 4, ([0, 0], []), True, True)]
    del log[:]
    make().recommend(USERS, 4, exclude_seen=False, chunk=None)
    assert log == [("excluded", USERS, 4, None, False, False)]


def test_call_sequence_recommend_new(served):
    make, log = served
    make().recommend_new(HISTORIES, 4, deny_items=[5], exclude={0: [10, 11]}, chunk=2)
    assert log == [("fold_in", ([0, 3, 5], [1, 7, 8, 0, 4]), None),                        # histories sorted, repeats collapsed
                   ("excluded", [0, 1], 4, ([0, 5, 7], [1, 7, 8, 10, 11, 0, 4]), False, True),    # the history in front of the exclusion row
                   ("fold_in", ([0, 0, 2], [2, 29]), None),
                   ("excluded", [0, 1], 4, ([0, 0, 2], [2, 29]), False, True),
                   ("fold_in", ([0, 1], [9]), None),
                   ("excluded", [0], 4, ([0, 1], [9]), False, True)]
    del log[:]
    make().recommend_new(HISTORIES, 4, exclude_history=False, id_rows=ID_ROWS, chunk=3)
    assert log == [("fold_in", ([0, 3, 5, 5], [1, 7, 8, 0, 4]), ID_ROWS[:3].tolist()), ("excluded", [0, 1, 2], 4, None, False, False),
                   ("fold_in", ([0, 2, 3], [2, 29, 9]), ID_ROWS[3:].tolist()), ("excluded", [0, 1], 4, None, False, False)]


def test_call_sequence_rank_and_rank_new(served):
    make, log = served
    cands = {3: [20, 1, 21], 0: [22], 1: [5, -1, 6]}                        # user 6 has no key: an empty row; -1 is padding
    make().rank(USERS, cands, 2, exclude={3: [21]}, chunk=2)
    plain = [("candidates", [3, 0], 2, ([0, 3, 4], [20, 1, 21, 22]), ([0, 1, 1], [21]), True, False),
             ("candidates", [3, 6], 2, ([0, 3, 3], [20, 1, 21]), ([0, 1, 1], [21]), True, False),
             ("candidates", [1], 2, ([0, 2], [5, 6]), ([0, 0], []), True, False)]
    assert log == plain
    del log[:]
    make().rank(USERS, cands, 2, exclude={3: [21]}, chunk=2, group_of=GROUP, per_group=1)
    assert log == [("capped",) + e[1:] + (1, 3) for e in plain]            # the capped op exactly when a quota is given, the same slices
    del log[:]
    make().rank_new(HISTORIES, [[20, 1, 21], [22], [3], [], [5, 6]], 2, chunk=2, allow_items=ALLOW, group_of=GROUP, per_group=[1, 0, 2])
    assert log == [("fold_in", ([0, 3, 5], [1, 7, 8, 0, 4]), None),
                   ("capped", [0, 1], 2, ([0, 3, 4], [20, 1, 21, 22]), ([0, 3, 5], [1, 7, 8, 0, 4]), False, True, [1, 0, 2], 3),
                   ("fold_in", ([0, 0, 2], [2, 29]), None),
                   ("capped", [0, 1], 2, ([0, 1, 1], [3]), ([0, 0, 2], [2, 29]), False, True, [1, 0, 2], 3),
                   ("fold_in", ([0, 1], [9]), None),
                   ("capped", [0], 2, ([0, 2], [5, 6]), ([0, 1], [9]), False, True, [1, 0, 2], 3)]
    del log[:]
    make().rank_new(HISTORIES, [[20, 1, 21], [22], [3], [], [5, 6]], 2, chunk=None, exclude_history=False)
    assert log == [("fold_in", ([0, 3, 5, 5, 7, 8], [1, 7, 8, 0, 4, 2, 29, 9]), None),
                   ("candidates", [0, 1, 2, 3, 4], 2, ([0, 3, 4, 5, 5, 7], [20, 1, 21, 22, 3, 5, 6]), None, False, False)]


def test_call_sequence_recommend_under_a_quota(served, monkeypatch):
    """Tables under which every user ranks the items by ascending id (score of item i: (30 - i) / 2), so that the fetched rows and the
    unsettled queries can be written down: k = 3, one item per group, items 1 and 3 of no group, overfetch = 1 -> K1 = 3."""
    make, log = served
    monkeypatch.setattr(serve, "ROUND2_PAIRS", I)
    E_u, E_i = torch.zeros(U, D), torch.zeros(I, D)
    E_u[:, 0], E_i[:, 0] = 1.0, torch.arange(I, 0, -1) * 0.5
    rec = make(E_u, E_i)
    items, scores = rec.recommend(USERS, 3, deny_items=[5], exclude={3: [10, 11]}, chunk=2, group_of=GROUP, per_group=1, overfetch=1)
    gone3 = ([0, 2], [10, 11])
    assert log == [("excluded", [3, 0], 3, ([0, 2, 2], [10, 11]), True, True),
                   ("capped", [3, 0], 3, ([0, 3, 6], [0, 2, 3, 1, 2, 3]), None, False, False, 1, 3),        # user 3: [0, 3, -], user 0: [1, 2, 3]
                   ("capped", [3], 3, ([0, I], RANGE), gone3, True, True, 1, 3),
                   ("excluded", [3, 6], 3, ([0, 2, 2], [10, 11]), True, True),
                   ("capped", [3, 6], 3, ([0, 3, 6], [0, 2, 3, 0, 1, 2]), None, False, False, 1, 3),        # user 3: [0, 3, -], user 6: [0, 1, -]
                   ("capped", [3], 3, ([0, I], RANGE), gone3, True, True, 1, 3),
                   ("capped", [6], 3, ([0, I], RANGE), ([0, 0], []), True, True, 1, 3),
                   ("excluded", [1], 3, ([0, 0], []), True, True),
                   ("capped", [1], 3, ([0, 3], [0, 1, 3]), None, False, False, 1, 3)]                      # user 1: [0, 1, 3], settled
    assert items.tolist() == [[0, 3, 12], [1, 2, 3], [0, 3, 12], [0, 1, 3], [0, 1, 3]]
    assert scores.tolist() == [[(I - i) * 0.5 for i in row] for row in items.tolist()]
    assert rec.last_quota == {"queries": 5, "round2": 3}
    del log[:]
    rec.recommend_new(HISTORIES[:2], 3, group_of=GROUP, per_group=1, overfetch=1)            # one chunk; histories {1, 7, 8} and {0, 4}
    assert log == [("fold_in", ([0, 3, 5], [1, 7, 8, 0, 4]), None),
                   ("excluded", [0, 1], 3, ([0, 3, 5], [1, 7, 8, 0, 4]), False, False),
                   ("capped", [0, 1], 3, ([0, 3, 6], [0, 2, 3, 1, 2, 3]), None, False, False, 1, 3),        # [0, 3, -] and [1, 2, 3]
                   ("capped", [0], 3, ([0, I], RANGE), ([0, 3], [1, 7, 8]), False, False, 1, 3)]
    assert rec.last_quota == {"queries": 2, "round2": 1}


def test_the_messages_of_bad_requests(served):
    make, _ = served
    rec = make()
    plain = serve.Recommender(E_U, E_I, _train())
    fold = "Recommender: built without fold_in=True - Recommender.from_trainer / from_checkpoint(..., fold_in=True) " \
           "build the item-side tables that new users are embedded from"
    cands = "candidates: a dict, a (rowptr, colidx) tuple, an [n, m] array or a sequence of n id sequences expected"
    for call, args, kw in (("recommend_new", ([[1]], 0), {"id_rows": np.zeros((3, 1))}), ("rank_new", ([[1]], None, 0), {}), ("embed_new", ([[1]],), {})):
        with pytest.raises(RuntimeError, match=re.escape(fold)):            # a missing fold_in comes before anything else
            getattr(plain, call)(*args, **kw)
    for call, args, kw, message in (
            ("recommend", ([0, U], 4), {}, "users: ids must lie in [0, %d); got 0 .. %d" % (U, U)),
            ("rank", ([0.5], [[1]], 4), {}, "users: integer ids expected, got float64"),
            ("rank", (USERS, None, 4), {}, cands),
            ("rank_new", (HISTORIES, None, 4), {}, cands),
            ("recommend", (USERS, 0), {"group_of": GROUP, "per_group": 1}, "k = 0: under quotas 1 <= k <= 1024"),
            ("recommend_new", (HISTORIES, 1025), {"group_of": GROUP, "per_group": 1}, "k = 1025: under quotas 1 <= k <= 1024"),
            ("recommend", (USERS, 4), {"group_of": GROUP, "per_group": 1, "overfetch": 0}, "overfetch: an integer >= 1 expected, got 0"),
            ("recommend_new", (HISTORIES, 4), {"group_of": GROUP, "per_group": 1, "overfetch": 1.5}, "overfetch: an integer >= 1 expected, got 1.5"),
            ("recommend_new", (HISTORIES, 4), {"id_rows": np.zeros((5, D + 1))}, "id_rows: [n, %d] expected, got (5, %d)" % (D, D + 1)),
            ("rank_new", (HISTORIES, CAND_ROWS, 4), {"id_rows": np.zeros(D)}, "id_rows: [n, %d] expected, got (%d,)" % (D, D))):
        with pytest.raises(ValueError, match=re.escape(message)):
            getattr(rec, call)(*args, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# Part B: what the four wrappers hand the library
# ------------------------------------------------------------------------------------------------------------------------------------
WS_BYTES = 4096                                                             # what every recorded workspace query answers


class Ptr:
    """An expected pointer argument: the address of `tensor`."""

    def __init__(self, tensor):
        self.tensor = tensor


@pytest.fixture
def library(monkeypatch):
    """The calls and the size queries the wrappers make, recorded: [(entry, args)]."""
    calls, queries = [], []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_lib, "query", lambda name, *args: queries.append((name, args)) or WS_BYTES)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.delenv("LLMREC_TOPK_MODE", raising=False)
    return calls, queries


def _handed(calls, entry, expected):
    """The one recorded call is `entry` with `expected` as its positional arguments: scalars by value, a Ptr by the tensor it addresses,
    None where the header allows NULL, ... for a pointer to memory the wrapper allocated itself."""
    (name, args), = calls
    del calls[:]
    assert name == entry and len(args) == len(expected), (name, len(args), len(expected))
    for pos, (got, want) in enumerate(zip(args, expected)):
        if want is ...:
            assert got.value, (entry, pos)
        elif isinstance(want, Ptr):
            assert got is not None and got.value == want.tensor.data_ptr(), (entry, pos)
        else:
            assert got is None if want is None else (got is not None and not hasattr(got, "value") and got == want), (entry, pos, got, want)


def _tables():
    q = torch.tensor([3, 0, 3], dtype=torch.int64)
    filt = SimpleNamespace(n_items=I, n_kept=11, new_id=torch.zeros(I, dtype=torch.int32), old_id=torch.zeros(I, dtype=torch.int32),
                           n_kept_dev=torch.zeros(1, dtype=torch.int32))
    return q, _train(), filt


def _csr(rowptr, colidx):
    return torch.tensor(rowptr, dtype=torch.int32), torch.tensor(colidx, dtype=torch.int32)


PREFILTER, EXACT = ops.TOPK_MODES["prefilter"], ops.TOPK_MODES["exact"]
QUEUED_TRAIN_NNZ = 3 + 2 + 3                                                # the train rows of users 3, 0, 3


def test_the_sweep_wrappers_hand_the_library_the_header_s_arguments(library):
    calls, queries = library
    q, train, filt = _tables()
    n, K = q.numel(), 4
    head = lambda: (n, Ptr(q), Ptr(E_U), D, Ptr(E_I), D, I, D)              # n_query, query_users, Eu, ldu, Ei, ldi, n_items, d
    maps = lambda f: (Ptr(f.new_id), Ptr(f.old_id), Ptr(f.n_kept_dev), f.n_kept) if f is not None else (None, None, None, I)
    for tr, mode, nnz, own_ws in ((train, None, None, False), (None, "exact", None, True), (train, None, 50, True), (None, None, 50, False)):
        ws = torch.empty(64, dtype=torch.uint8) if own_ws else None
        want_nnz = 0 if tr is None else (QUEUED_TRAIN_NNZ if nnz is None else nnz)
        del queries[:]
        idx, sc = ops.score_topk_filtered(E_U, E_I, q, tr, K, filt, mode=mode, train_nnz=nnz, ws=ws)
        assert idx.shape == sc.shape == (n, K) and idx.dtype == torch.int32 and sc.dtype == torch.float32
        # ... train_rowptr, train_colidx, K, out_idx, out_score, workspace, workspace_bytes, mode, train_nnz, new_id, old_id, n_kept_dev, n_kept, stream
        _handed(calls, "llmrec_score_topk_filtered_f32", head() + (
            Ptr(tr.rowptr) if tr else None, Ptr(tr.colidx) if tr else None, K, Ptr(idx), Ptr(sc), Ptr(ws) if own_ws else ..., 64 if own_ws else WS_BYTES,
            EXACT if mode else PREFILTER, want_nnz) + maps(filt) + (0,))
        assert queries == ([] if own_ws else [("llmrec_score_topk_filtered_workspace_bytes", (n, I, filt.n_kept, D, K, want_nnz))])
        for f, (rowptr, colidx) in itertools.product((filt, None), (_csr([0, 2, 2, 3], [10, 11, -1]), _csr([0, 0, 0, 0], []))):
            del queries[:]
            idx, sc = ops.score_topk_excluded(E_U, E_I, q, tr, K, (rowptr, colidx), f, mode=mode, train_nnz=nnz, ws=ws)
            nz = colidx.numel()
            # ... mode, train_nnz, excl_rowptr, excl_colidx, excl_nnz, new_id, old_id, n_kept_dev, n_kept, stream
            _handed(calls, "llmrec_score_topk_excluded_f32", head() + (
                Ptr(tr.rowptr) if tr else None, Ptr(tr.colidx) if tr else None, K, Ptr(idx), Ptr(sc), Ptr(ws) if own_ws else ...,
                64 if own_ws else WS_BYTES, EXACT if mode else PREFILTER, want_nnz, Ptr(rowptr), Ptr(colidx) if nz else None, nz) + maps(f) + (0,))
            kept = f.n_kept if f is not None else I
            assert queries == ([] if own_ws else [("llmrec_score_topk_excluded_workspace_bytes", (n, I, kept, D, K, want_nnz, nz))])
    idx, sc = ops.score_topk_excluded(E_U, E_I, q, train, K, None, filt, train_nnz=7)      # no lists: the filtered entry
    _handed(calls, "llmrec_score_topk_filtered_f32", head() + (Ptr(train.rowptr), Ptr(train.colidx), K, Ptr(idx), Ptr(sc), ..., WS_BYTES, PREFILTER, 7)
            + maps(filt) + (0,))


def test_the_candidate_wrappers_hand_the_library_the_header_s_arguments(library):
    calls, queries = library
    q, train, filt = _tables()
    n, K = q.numel(), 4
    group = torch.tensor(GROUP, dtype=torch.int32)
    caps = torch.tensor([1, 0, 3, 2], dtype=torch.int32)
    head = lambda: (n, Ptr(q), Ptr(E_U), D, Ptr(E_I), D, I, D)
    cands = (_csr([0, 3, 4, 6], [20, 1, 21, 22, 5, 6]), _csr([0, 0, 0, 0], []))
    excls = (None, _csr([0, 1, 1, 2], [21, 40]), _csr([0, 0, 0, 0], []))
    for tr, f, cand, excl, own_ws in itertools.product((train, None), (filt, None), cands, excls, (False, True)):
        ws = torch.empty(64, dtype=torch.uint8) if own_ws else None
        cn, en = cand[1].numel(), excl[1].numel() if excl is not None else 0
        # ... train_rowptr, train_colidx, K, out_idx, out_score, workspace, workspace_bytes, cand_rowptr, cand_colidx, cand_nnz, excl_rowptr,
        # excl_colidx, excl_nnz, new_id, [item_group, n_groups, group_cap, cap,] stream
        middle = lambda idx, sc: (Ptr(tr.rowptr) if tr else None, Ptr(tr.colidx) if tr else None, K, Ptr(idx), Ptr(sc), Ptr(ws) if own_ws else ...,
                                  64 if own_ws else WS_BYTES, Ptr(cand[0]), Ptr(cand[1]) if cn else None, cn,
                                  Ptr(excl[0]) if excl is not None else None, Ptr(excl[1]) if en else None, en, Ptr(f.new_id) if f else None)
        sized = [] if own_ws else [("llmrec_score_topk_candidates_workspace_bytes", (n, K, cn, en))]
        del queries[:]
        idx, sc = ops.score_topk_candidates(E_U, E_I, q, tr, K, cand, excl, f, ws=ws)
        assert idx.shape == sc.shape == (n, K) and idx.dtype == torch.int32 and sc.dtype == torch.float32
        _handed(calls, "llmrec_score_topk_candidates_f32", head() + middle(idx, sc) + (0,))
        assert queries == sized
        for cap, n_groups, tail in ((2, 3, (3, None, 2)), (2, None, (3, None, 2)), (1, 7, (7, None, 1)), (caps, None, (4, Ptr(caps), 0)),
                                    (caps, 4, (4, Ptr(caps), 0))):
            del queries[:]
            idx, sc = ops.score_topk_candidates_capped(E_U, E_I, q, tr, K, cand, group, cap, excl, f, ws=ws, n_groups=n_groups)
            assert idx.shape == sc.shape == (n, K) and idx.dtype == torch.int32 and sc.dtype == torch.float32
            _handed(calls, "llmrec_score_topk_candidates_capped_f32", head() + middle(idx, sc) + (Ptr(group),) + tail + (0,))
            assert queries == sized
    idx, sc = ops.score_topk_candidates(E_U, E_I, q, None, 2000, cands[0])                  # any K: the uncapped entry has no limit
    assert idx.shape == (n, 2000) and calls.pop()[0] == "llmrec_score_topk_candidates_f32"


def test_the_wrappers_refuse_what_they_refused(library):
    calls, _ = library
    q, train, filt = _tables()
    group = torch.tensor(GROUP, dtype=torch.int32)
    good = _csr([0, 1, 1, 2], [21, 22])
    small = SimpleNamespace(n_items=I - 1, n_kept=3, new_id=None, old_id=None, n_kept_dev=None)
    short, long_ = _csr([0, 1, 2], [21, 22]), (good[0].to(torch.int64), good[1])
    wide = "%s: K = 1025 exceeds LLMREC_TOPK_WIDE_MAX = 1024"
    size = "%%s: the filter covers %d items, the table has %d" % (I - 1, I)
    csr = "%s: %s = (rowptr int32 [4], colidx int32 [nnz]) expected, got %s %s and torch.int32 (2,)"
    capped = lambda *a, **kw: ops.score_topk_candidates_capped(*a[:6], group, 2, *a[6:], n_groups=3, **kw)
    for message, call in (
            (wide % "score_topk_filtered", lambda: ops.score_topk_filtered(E_U, E_I, q, train, 1025, filt)),
            (wide % "score_topk_excluded", lambda: ops.score_topk_excluded(E_U, E_I, q, train, 1025, good, filt)),
            (wide % "score_topk_excluded", lambda: ops.score_topk_excluded(E_U, E_I, q, train, 1025, good)),
            (wide % "score_topk_candidates_capped", lambda: capped(E_U, E_I, q, train, 1025, good)),
            (size % "score_topk_filtered", lambda: ops.score_topk_filtered(E_U, E_I, q, train, 4, small)),
            (size % "score_topk_excluded", lambda: ops.score_topk_excluded(E_U, E_I, q, train, 4, good, small)),
            (size % "score_topk_candidates", lambda: ops.score_topk_candidates(E_U, E_I, q, train, 4, good, None, small)),
            (size % "score_topk_candidates_capped", lambda: capped(E_U, E_I, q, train, 4, good, None, small)),
            (csr % ("score_topk_excluded", "exclude", "torch.int32", "(3,)"), lambda: ops.score_topk_excluded(E_U, E_I, q, train, 4, short)),
            (csr % ("score_topk_excluded", "exclude", "torch.int64", "(4,)"), lambda: ops.score_topk_excluded(E_U, E_I, q, train, 4, long_, filt)),
            (csr % ("score_topk_candidates", "candidates", "torch.int32", "(3,)"), lambda: ops.score_topk_candidates(E_U, E_I, q, train, 4, short)),
            (csr % ("score_topk_candidates", "exclude", "torch.int64", "(4,)"), lambda: ops.score_topk_candidates(E_U, E_I, q, train, 4, good, long_)),
            (csr % ("score_topk_candidates_capped", "candidates", "torch.int64", "(4,)"), lambda: capped(E_U, E_I, q, train, 4, long_)),
            (csr % ("score_topk_candidates_capped", "exclude", "torch.int32", "(3,)"), lambda: capped(E_U, E_I, q, train, 4, good, short)),
            ("score_topk_candidates_capped: item_group int32 [%d] expected, got torch.int32 (%d,)" % (I, I - 1),
             lambda: ops.score_topk_candidates_capped(E_U, E_I, q, train, 4, good, group[:-1], 2)),
            ("score_topk_candidates_capped: an integer cap >= 1 or an int32 tensor [n_groups] expected, got 0",
             lambda: ops.score_topk_candidates_capped(E_U, E_I, q, train, 4, good, group, 0)),
            ("score_topk_candidates_capped: cap = int32 [n_groups >= 1] expected, got torch.int32 (3,) (n_groups = 4)",
             lambda: ops.score_topk_candidates_capped(E_U, E_I, q, train, 4, good, group, torch.ones(3, dtype=torch.int32), n_groups=4))):
        with pytest.raises(RuntimeError, match=re.escape(message)):
            call()
    assert calls == []
