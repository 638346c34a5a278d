"""GPU tests of the full-rank AUC (llmrec_score_auc_f32 / ops.score_auc; --test_flag full): exact pair counts against the numpy contract of
tests/_auc_ref.py on the kernel's own score bits, determinism and graph replay, the drop-in's Trainer.test with --test_flag full on the fused
and on the modular path (without sklearn too), and a generous time bound that shows the work stays on the device."""
import sys

import numpy as np
import pytest
import torch

from llmrec_amd import ops
from llmrec_amd.fused import _capture_without_gc
from tests._auc_ref import auc_counts

pytestmark = pytest.mark.gpu


def _csr(rows, n_users):
    rp = np.zeros(n_users + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in rows]).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()


def _check(Eu, Ei, q, train_rows, held_rows, exact, tol=1e-12, check_users=None):
    n_users, n_items = Eu.shape[0], Ei.shape[0]
    train, held = _csr(train_rows, n_users), _csr(held_rows, n_users)
    qt = torch.tensor(q, dtype=torch.int64, device="cuda")
    auc, cnt = ops.score_auc(Eu, Ei, qt, train, held, counts=True)
    auc, cnt = auc.cpu().numpy(), cnt.cpu().numpy()
    rows = range(len(q)) if check_users is None else check_users
    sel = torch.tensor([q[r] for r in rows], dtype=torch.int64, device="cuda")
    S = ops.scores(Eu, Ei, sel).cpu().numpy()
    for j, r in enumerate(rows):
        c2, n_p, n_n, a = auc_counts(S[j], train_rows[q[r]], held_rows[q[r]], n_items)
        assert (int(cnt[r, 1]), int(cnt[r, 2])) == (n_p, n_n), (r, cnt[r], n_p, n_n)
        if exact:
            assert int(cnt[r, 0]) == c2 and auc[r] == a, (r, cnt[r], c2, auc[r], a)
        else:
            assert abs(auc[r] - a) <= tol, (r, auc[r], a)
    return auc, cnt


@pytest.mark.parametrize("d,ld", [(16, 16), (64, 80), (128, 128)])
def test_exact_counts_on_tied_integer_scores(d, ld):
    rng = np.random.default_rng(d)
    n_users, n_items = 24, 6007                                        # not a multiple of 64
    Eu = torch.from_numpy(rng.integers(-2, 3, (n_users, ld)).astype(np.float32) / 2).cuda()[:, :d]
    Ei = torch.from_numpy(rng.integers(-2, 3, (n_items, ld)).astype(np.float32) / 4).cuda()[:, :d]
    assert Eu.stride(0) == ld and Ei.stride(0) == ld
    train_rows, held_rows = [], []
    sizes = [0, 1, 63, 64, 65, 500, 5000, 7, 3, 2]
    for u in range(n_users):
        tr = np.sort(rng.choice(n_items, int(rng.integers(0, 300)), replace=False))
        k = sizes[u % len(sizes)]
        free = np.setdiff1d(np.arange(n_items), tr)
        h = rng.choice(free, min(k, free.size), replace=False)
        h = np.concatenate([h, h[:3], tr[:2], [n_items, n_items + 5]])   # duplicates, train items, ids out of range
        if u == 10:
            tr, h = np.arange(n_items), np.arange(5)                      # every item in train
        if u == 11:
            h = free                                                       # |N| = 0
        train_rows.append(tr)
        held_rows.append(h)
    q = list(range(n_users)) + [3, 6, 6]                               # repeated query users
    auc, cnt = _check(Eu, Ei, q, train_rows, held_rows, exact=True)
    assert cnt[10].tolist() == [0, 0, 0] and auc[10] == 0.0
    assert cnt[11, 2] == 0 and auc[11] == 0.0
    assert sorted(set(int(c) for c in cnt[:10, 1])) == sorted(sizes)  # every |P| of the list swept


def _random_case(rng, n_users, n_items, d, n_query, train_deg=30, held_deg=4):
    Eu = torch.from_numpy(rng.standard_normal((n_users, d)).astype(np.float32) * 0.3).cuda()
    Ei = torch.from_numpy(rng.standard_normal((n_items, d)).astype(np.float32) * 0.3).cuda()
    train_rows = [np.sort(rng.choice(n_items, int(rng.integers(0, 2 * train_deg)), replace=False)) for _ in range(n_users)]
    held_rows = [rng.integers(0, n_items, int(rng.integers(0, 2 * held_deg))) for _ in range(n_users)]
    q = rng.choice(n_users, n_query, replace=False).tolist()
    return Eu, Ei, train_rows, held_rows, q


@pytest.mark.parametrize("n_users,n_items,d,n_query", [(300, 1000, 32, 200), (2000, 9999, 64, 2000), (13187, 17366, 64, 13187),
                                                        (400, 270001, 64, 64)])
def test_random_tables_match_numpy(n_users, n_items, d, n_query):
    rng = np.random.default_rng(n_items)
    Eu, Ei, train_rows, held_rows, q = _random_case(rng, n_users, n_items, d, n_query)
    check = None if n_query <= 2000 else sorted(rng.choice(n_query, 1500, replace=False).tolist())
    _check(Eu, Ei, q, train_rows, held_rows, exact=False, check_users=check)


def test_non_finite_scores_zero_the_user_unless_in_train():
    rng = np.random.default_rng(5)
    Eu, Ei, train_rows, held_rows, q = _random_case(rng, 64, 3000, 64, 64)
    Ei[17, 3] = float("nan")
    Ei[29, 0] = float("inf")
    train_rows[0] = np.union1d(train_rows[0], [17, 29])              # user 0: both non-finite items masked
    held_rows[0] = np.setdiff1d(np.arange(100), train_rows[0])[:5]
    auc, cnt = _check(Eu, Ei, list(range(64)), train_rows, held_rows, exact=True)
    assert auc[0] > 0.0 and all(auc[u] == 0.0 for u in range(1, 64) if 17 not in train_rows[u] and 29 not in train_rows[u])


def test_deterministic_and_graph_replay_gives_identical_bits():
    rng = np.random.default_rng(11)
    Eu, Ei, train_rows, held_rows, q = _random_case(rng, 3000, 12000, 64, 3000)
    train, held = _csr(train_rows, 3000), _csr(held_rows, 3000)
    qt = torch.tensor(q, dtype=torch.int64, device="cuda")
    s1, s2, s3 = (torch.zeros(1, dtype=torch.float64).pin_memory() for _ in range(3))
    a1, c1 = ops.score_auc(Eu, Ei, qt, train, held, counts=True, out=s1)
    a2, c2 = ops.score_auc(Eu, Ei, qt, train, held, counts=True, out=s2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(c1, c2) and s1[0].item() == s2[0].item()
    a3 = torch.empty_like(a1)
    ws = ops.auc_workspace(qt.numel(), Ei.shape[0], Eu.device, 64)
    ops.score_auc(Eu, Ei, qt, train, held, out=s3, ws=ws)             # warm-up outside the capture
    torch.cuda.synchronize()
    s3.zero_()
    g = torch.cuda.CUDAGraph()
    with _capture_without_gc(g, False):
        a3.copy_(ops.score_auc(Eu, Ei, qt, train, held, out=s3, ws=ws))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a1, a3) and s3[0].item() == s1[0].item()
    assert s1[0].item() == pytest.approx(a1.sum().item(), rel=1e-12)


def test_netflix_shape_runs_on_the_device_in_milliseconds():
    rng = np.random.default_rng(3)
    Eu, Ei, train_rows, held_rows, q = _random_case(rng, 13187, 17366, 64, 13187)
    train, held = _csr(train_rows, 13187), _csr(held_rows, 13187)
    qt = torch.tensor(q, dtype=torch.int64, device="cuda")
    ws = ops.auc_workspace(qt.numel(), Ei.shape[0], Eu.device, 64)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    for _ in range(3):
        ops.score_auc(Eu, Ei, qt, train, held, out=out, ws=ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        ops.score_auc(Eu, Ei, qt, train, held, out=out, ws=ws)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    assert ms <= 20.0, ms


# ---- the drop-in's Trainer.test with --test_flag full ----
from tests._dropin import load_dropin, golden_argv          # noqa: E402
from tests.conftest import GoldenCase                       # noqa: E402


def _expected_auc(m, E_u, E_i, users, is_val=False):
    dg = m.data_generator
    S = ops.scores(E_u, E_i, torch.tensor(users, device="cuda")).cpu().numpy()
    held = dg.val_set if is_val else dg.test_set
    return float(np.mean([auc_counts(S[r], dg.train_items.get(u, []), held.get(u, []), dg.n_items)[3] for r, u in enumerate(users)]))


def test_trainer_full_fused_path_is_one_graph_and_needs_no_sklearn(monkeypatch):
    g = GoldenCase("nf_tiny")
    m = load_dropin(golden_argv(g) + ["--test_flag", "full"])
    m.set_seed(3)
    tr = m.Trainer(data_config={})
    fused = tr._fused_step()
    assert fused
    users = g.z["eval/users"].tolist()
    r1 = tr.test(users, is_val=False)
    n_graphs = len(fused._eval_graphs)
    graph = fused._last_eval[0]
    monkeypatch.setitem(sys.modules, "sklearn", None)
    monkeypatch.setitem(sys.modules, "sklearn.metrics", None)
    r2 = tr.test(users, is_val=False)
    assert len(fused._eval_graphs) == n_graphs == 1 and fused._last_eval[0] is graph      # the captured evaluation is replayed
    want = _expected_auc(m, fused.E_u, fused.E_i, users)
    assert 0.0 < want < 1.0
    assert abs(r1["auc"] - want) <= 1e-12 and r2["auc"] == r1["auc"]
    for k in ("precision", "recall", "ndcg", "hit_ratio"):
        assert np.array_equal(r1[k], r2[k])


def test_trainer_full_modular_path_matches_numpy(monkeypatch):
    g = GoldenCase("nf_tiny")
    m = load_dropin(golden_argv(g) + ["--test_flag", "full", "--mask", "True", "--mask_rate", "0.25"])
    m.set_seed(3)
    tr = m.Trainer(data_config={})
    assert tr._fused_step() is False
    users = g.z["eval/users"].tolist()
    monkeypatch.setitem(sys.modules, "sklearn", None)
    monkeypatch.setitem(sys.modules, "sklearn.metrics", None)
    seen, orig = [], m.test_full_on_device
    def recording(ua, ia, *a, **k):                                   # (the masked forward draws its own mask: keep the tables it scored)
        seen.append((ua.detach().clone(), ia.detach().clone()))
        return orig(ua, ia, *a, **k)
    monkeypatch.setattr(m, "test_full_on_device", recording)
    monkeypatch.setattr(m, "test_torch", None)                        # (full never reaches the host loop)
    res = tr.test(users, is_val=False)
    assert len(seen) == 1
    want = _expected_auc(m, seen[0][0], seen[0][1], users)
    assert 0.0 < want < 1.0 and abs(res["auc"] - want) <= 1e-12


def test_trainer_full_fused_eager_path_matches_numpy(monkeypatch):
    monkeypatch.setenv("LLMREC_EVAL_GRAPH", "0")
    g = GoldenCase("nf_tiny")
    m = load_dropin(golden_argv(g) + ["--test_flag", "full"])
    m.set_seed(3)
    tr = m.Trainer(data_config={})
    fused = tr._fused_step()
    assert fused
    users = g.z["eval/users"].tolist()
    monkeypatch.setitem(sys.modules, "sklearn", None)
    monkeypatch.setitem(sys.modules, "sklearn.metrics", None)
    monkeypatch.setattr(m, "test_torch", None)                        # (full never reaches the host loop)
    res = tr.test(users, is_val=False)
    assert len(fused._eval_graphs) == 0
    want = _expected_auc(m, fused.E_u, fused.E_i, users)
    assert 0.0 < want < 1.0 and abs(res["auc"] - want) <= 1e-12
