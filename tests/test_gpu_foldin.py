"""GPU: fold-in of users who are not rows of the graph - llmrec_fold_in_users_f32 (csrc/foldin.hip) through ops.FoldInTables /
ops.fold_in_users, Recommender.embed_new / recommend_new and recommend.py --histories.

The kernel is held to the float64 restatement of tests/_foldin_ref.py ELEMENT BY ELEMENT, under the bound that module derives from the
kernel's order of operations. Which row length takes which path of the kernel (R.PATH): 0, 1, 2, 63, 64, 65 are rows of one segment,
summed and finished by one block of fi_gather_kernel (0: no entry; 1, 2: waves without an entry; 63, 64, 65: runs of 16 / 16 / 17 per
wave, the last run ragged); 257, 3000, 5000 are rows of 2, 12 and 20 segments, each summed by a block of its own and finished by
fi_finish_long_kernel (257: a second segment of one entry; 3000: every item once, a ragged last segment; 5000: repeats). Every length
occurs 22 or 23 times in the one call of 203 rows. d = 64, 128, 20 take the float4 loads when T is aligned and the scalar loads through
a misaligned view; d = 7 always takes the scalar loads.
Everything else is exact: torch.equal."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _foldin_ref as R
from tests._dropin import ROOT, golden_argv
from tests.conftest import GoldenCase
from tests.test_gpu_serve import ENVS, FLAGS, _expected, _train_and_reload

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(ops, c, T=None):
    return ops.FoldInTables(_dev(c.T) if T is None else T, c.L, c.n_attr, c.d, *R.RATES)


def _view(a, pad, off):
    """`a` [rows, w] as a column view at column `off` of a table pad columns wider (filled with a value nothing may read into a result)"""
    wide = torch.full((a.shape[0], a.shape[1] + pad), 12345.0, device=DEV)
    wide[:, off:off + a.shape[1]] = a
    return wide[:, off:off + a.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the fp64 reference, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L,n_attr", R.cases())
def test_kernel_against_fp64_element_by_element(ops, d, L, n_attr):
    c = R.case(d, L, n_attr)
    assert {R.PATH[len(h)] for h in c.rows} == {"one", "long"}
    rp, ci, w, ids = _dev(c.rowptr), _dev(c.colidx), _dev(c.w), _dev(c.id_rows)
    tables = _tables(ops, c)
    worst = {}
    base, sums = None, R.gathered(c.T, c.rows)
    for name, id_rows in (("id_rows", c.id_rows), ("no id_rows", None)):
        ref, bound = R.reference(c.T, c.rows, c.w, id_rows, L, n_attr, d, R.RATES, sums)
        got = ops.fold_in_users(tables, rp, ci, row_scale=w, id_rows=ids if id_rows is not None else None)
        assert got.shape == (R.N_ROWS, d) and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref) / bound
        worst[name] = float(err.max())
        if id_rows is not None:
            base, base_ref, base_bound = got, ref, bound
    # T, id_rows and out as column views of wider tables: an aligned view (float4 loads where d % 4 == 0) and a misaligned one (scalar loads)
    for name, pad, off in (("view +4", 8, 4), ("view +1", 3, 1)):
        out = _view(torch.zeros(R.N_ROWS, d, device=DEV), pad, off)
        got = ops.fold_in_users(_tables(ops, c, _view(tables.T, pad, off)), rp, ci, row_scale=w, id_rows=_view(ids, pad, off), out=out)
        assert got.data_ptr() == out.data_ptr() and got.stride(0) == d + pad
        worst[name] = float((np.abs(got.cpu().numpy().astype(np.float64) - base_ref) / base_bound).max())
        assert torch.equal(got, base), name                        # the same sums through either family of loads
        assert (out._base[:, :off] == 12345.0).all() and (out._base[:, off + d:] == 12345.0).all(), name      # nothing written beside the view
    print("fold-in %s: worst |device - fp64| / bound: %s" % (c.name, {k: round(v, 3) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    # row_scale=None: from the row lengths on the device, the bits of the definition's expression
    lens = np.diff(c.rowptr)
    auto = ops.fold_in_users(tables, rp, ci, id_rows=ids)
    plain = ops.fold_in_users(tables, rp, ci, row_scale=_dev(R.row_scale(lens)), id_rows=ids)
    assert torch.equal(ops.fold_in_row_scale(rp), _dev(R.row_scale(lens))) and torch.equal(auto, plain)


def test_rows_the_definition_singles_out(ops):
    """an empty history: zero sums and a uniform softmax row; entries that add nothing add nothing; a repeat counts twice"""
    c = R.case(64, 2, 5)
    tables = _tables(ops, c)
    one = lambda h, w, ids=None: ops.fold_in_users(tables, _dev(np.array([0, len(h)], np.int32)), _dev(np.asarray(h, np.int32)),
                                                    row_scale=_dev(np.array([w], np.float32)), id_rows=ids)
    ids = _dev(c.id_rows[:1])
    empty = one([], 1e4, ids)
    third = np.float32(1.0) / np.float32(3.0)
    assert torch.equal(empty, (ids + torch.full((1, 64), 1.0 / 64, device=DEV)) * float(third))
    h = c.rows[R.SPRINKLED_ROW]
    clean = h[(h >= 0) & (h < R.N_ITEMS)]
    assert torch.equal(one([-1, 3000, 3005, -7], 0.5), one([], 0.5)) and len(clean) == 60
    ref, bound = R.reference(c.T, [clean], np.array([0.125], np.float32), None, 2, 5, 64, R.RATES)
    assert (np.abs(one(h, 0.125).cpu().numpy() - ref) <= bound).all()
    twice = R.reference(c.T, [np.array([7, 9, 7])], np.array([0.5], np.float32), None, 2, 5, 64, R.RATES)
    assert (np.abs(one([7, 9, 7], 0.5).cpu().numpy() - twice[0]) <= twice[1]).all()
    assert not (np.abs(one([7, 9], 0.5).cpu().numpy() - twice[0]) <= twice[1]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. independence and reproducibility
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L,n_attr", [(64, 2, 5), (7, 1, 0)])
def test_a_row_does_not_depend_on_its_call(ops, d, L, n_attr):
    c = R.case(d, L, n_attr)
    tables = _tables(ops, c)
    w, ids = _dev(c.w), _dev(c.id_rows)
    whole = ops.fold_in_users(tables, _dev(c.rowptr), _dev(c.colidx), row_scale=w, id_rows=ids)
    again = ops.fold_in_users(tables, _dev(c.rowptr), _dev(c.colidx), row_scale=w, id_rows=ids)
    assert torch.equal(whole, again)                               # two runs
    rev = c.rows[::-1]
    rp = np.concatenate([[0], np.cumsum([len(h) for h in rev])]).astype(np.int32)
    flipped = ops.fold_in_users(tables, _dev(rp), _dev(np.concatenate(rev).astype(np.int32)), row_scale=w.flip(0).contiguous(),
                                id_rows=ids.flip(0).contiguous())
    assert torch.equal(flipped.flip(0), whole)                     # the rows in reversed order
    singly = torch.cat([ops.fold_in_users(tables, _dev(np.array([0, len(h)], np.int32)), _dev(h), row_scale=w[r:r + 1], id_rows=ids[r:r + 1])
                        for r, h in enumerate(c.rows)])
    assert torch.equal(singly, whole)                              # one at a time


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_capture_on_one_stream(ops):
    c = R.case(64, 2, 5)
    tables = _tables(ops, c)
    rp, ci, w, ids = _dev(c.rowptr), _dev(c.colidx), _dev(c.w), _dev(c.id_rows)
    ws = ops.fold_in_workspace(R.N_ROWS, ci.numel(), tables, DEV)
    out = torch.zeros(R.N_ROWS, 64, device=DEV)
    run = lambda: ops.fold_in_users(tables, rp, ci, row_scale=w, id_rows=ids, out=out, ws=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        out.zero_()
        ws.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    tables.T.mul_(0.5)                                             # the table moves in place; the graph reads it at replay
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, eager) and torch.equal(out, ops.fold_in_users(tables, rp, ci, row_scale=w, id_rows=ids))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. recommend_new is exact
# ---------------------------------------------------------------------------------------------------------------------------------
def _synthetic_recommender(ops, fold_in=True):
    from llmrec_amd.serve import Recommender
    c = R.case(64, 2, 5)
    rng = np.random.default_rng(64)
    E_i = _dev((rng.standard_normal((R.N_ITEMS, 64)) * 0.4).astype(np.float32))
    E_u = _dev((rng.standard_normal((5, 64)) * 0.4).astype(np.float32))
    return Recommender(E_u, E_i, None, _tables(ops, c) if fold_in else None), rng


def _brute_force(ops, rec, histories, set_aside, allow, k, id_rows=None):
    """the statement itself: candidates = eligible items minus the rows of `set_aside`, by (score desc, id asc) over the bits of ops.scores"""
    E_new = rec.embed_new(histories, id_rows)
    n = E_new.shape[0]
    masked = torch.zeros(n, rec.n_items, dtype=torch.bool, device=DEV)
    for q, h in enumerate(set_aside):
        h = np.asarray(h, dtype=np.int64)
        masked[q, _dev(h[h >= 0])] = True
    if allow is not None:
        masked |= (allow == 0)[None, :]
    return _expected(ops.scores(E_new, rec.E_i, torch.arange(n, device=DEV)), masked, k, check_rows=(0,))


def _same(got, want, k):
    assert got[0].dtype == torch.int64 and got[0].shape == (want[0].shape[0], k) and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0][:, :k].long()) and torch.equal(got[1].view(torch.int32), want[1][:, :k].contiguous().view(torch.int32))


def test_recommend_new_is_exact(ops):
    rec, rng = _synthetic_recommender(ops)
    I = R.N_ITEMS
    hist = [rng.choice(I, size=int(n), replace=False) for n in (1, 5, 20, 200, 0, 64, 257, 1000)] + [np.arange(I)]      # the last holds every item
    n = len(hist)
    allow_np = np.flatnonzero(rng.random(I) < 0.03)
    allow = torch.zeros(I, dtype=torch.uint8, device=DEV)
    allow[_dev(allow_np)] = 1
    extra = [rng.choice(I, size=30, replace=False) for _ in range(n)]
    both = [np.concatenate([h, e]) for h, e in zip(hist, extra)]
    none = [np.zeros(0, np.int64)] * n
    ids = (rng.standard_normal((n, 64)) * 0.1).astype(np.float32)
    for k in (1, 20, 65):
        _same(rec.recommend_new(hist, k), _brute_force(ops, rec, hist, hist, None, k), k)
        got = rec.recommend_new(hist, k, allow_items=allow_np)
        _same(got, _brute_force(ops, rec, hist, hist, allow, k), k)
        live = got[0] >= 0
        assert np.isin(got[0][live].cpu().numpy(), allow_np).all() and (got[0][-1] == -1).all() and torch.isneginf(got[1][-1]).all()
        _same(rec.recommend_new(hist, k, exclude_history=False), _brute_force(ops, rec, hist, none, None, k), k)
        _same(rec.recommend_new(hist, k, exclude=extra), _brute_force(ops, rec, hist, both, None, k), k)
        _same(rec.recommend_new(hist, k, exclude=extra, exclude_history=False, deny_items=allow_np),
              _brute_force(ops, rec, hist, extra, 1 - allow, k), k)
        _same(rec.recommend_new(hist, k, id_rows=ids), _brute_force(ops, rec, hist, hist, None, k, ids), k)
    assert len(allow_np) > 65 and (rec.recommend_new(hist, 65)[0][:-1] >= 0).all()
    assert (rec.recommend_new(hist, 20)[0][-1] == -1).all()       # a history holding every item: nothing is left
    # an unsorted history with repeats and padding gives the bits of its sorted unique form
    messy = [np.concatenate([h[::-1], h[:3], [-1]]) for h in hist]
    assert torch.equal(rec.embed_new(messy), rec.embed_new([np.sort(h) for h in hist]))
    a, b = rec.recommend_new(messy, 20), rec.recommend_new(hist, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    # chunks bound the workspace, not the lists; every container form names the same users
    c = rec.recommend_new(hist, 20, chunk=4, exclude=extra)
    w = rec.recommend_new(hist, 20, chunk=None, exclude=extra)
    assert torch.equal(c[0], w[0]) and torch.equal(c[1].view(torch.int32), w[1].view(torch.int32))
    as_dict = rec.recommend_new({q: h for q, h in enumerate(hist)}, 20)
    assert torch.equal(as_dict[0], b[0])
    # the embedding is the kernel's, under the definition's row scale
    rp = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int32)
    direct = ops.fold_in_users(rec.fold_in, _dev(rp), _dev(np.concatenate([np.sort(h) for h in hist]).astype(np.int32)))
    assert torch.equal(rec.embed_new(hist), direct)
    with pytest.raises(ValueError, match=r"\[0, 3000\)"):
        rec.recommend_new([[3000]], 5)
    with pytest.raises(ValueError, match="rows"):
        rec.recommend_new(hist, 5, id_rows=ids[:3])
    with pytest.raises(ValueError, match="rows"):
        rec.recommend_new(hist, 5, exclude=extra[:3])
    bare, _ = _synthetic_recommender(ops, fold_in=False)
    for call in (lambda: bare.recommend_new(hist, 5), lambda: bare.embed_new(hist)):
        with pytest.raises(RuntimeError, match="fold_in=True"):
            call()
    assert rec.recommend_new([], 5)[0].shape == (0, 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. and 6. on the tiny drop-in trainer tests/test_gpu_serve.py trains and reloads (tests/golden/nf_tiny: 96 users x 80 items)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(tmp_path_factory):
    """served(path): the reloaded trainer of one route with its fold-in Recommender, built once for the module"""
    from llmrec_amd.serve import Recommender
    mp, made = pytest.MonkeyPatch(), {}

    def get(path):
        if path not in made:
            tmp = tmp_path_factory.mktemp("foldin_" + path)
            f, best = _train_and_reload(mp, path, tmp)
            made[path] = SimpleNamespace(f=f, best=best, tmp=tmp, rec=Recommender.from_checkpoint(f.trainer, best, fold_in=True))
        return made[path]

    yield get
    mp.undo()


@pytest.mark.parametrize("path", list(ENVS))
def test_an_existing_user_folds_in_to_its_own_row(ops, served, path):
    """the fold-in of user u's own train row with id_row = user_id_embedding.weight[u] is the forward's E_u[u] up to fp32 summation order
    (and, on the fused route under pre-propagation, (A F) W^T against A (F W^T)): relative error 1e-4, the parity tolerance of the bench's
    gate. Measured maxima: profiles/experiments/serve_foldin.md."""
    s = served(path)
    rec, tr = s.rec, s.f.trainer
    assert (rec.n_users, rec.n_items) == (96, 80) and rec.fold_in is not None and rec.iu.n_rows == 80
    assert (tr._fused is False) == (path == "modular")
    train = s.f.m.data_generator.device_state(DEV)["train"]
    got = ops.fold_in_users(rec.fold_in, train.rowptr, train.colidx, id_rows=tr.model_mm.user_id_embedding.weight.detach())
    rel = float((got - rec.E_u).abs().max() / rec.E_u.abs().max())
    print("fold-in of the train rows against E_u, route %s: max |a - b| / max |b| = %.3g" % (path, rel))
    assert rel <= 1e-4
    # through the Recommender: the same rows as histories (sorted unique: a train row is that already)
    rp, ci = train.rowptr.cpu().numpy(), train.colidx.cpu().numpy()
    assert torch.equal(rec.embed_new((rp, ci), id_rows=tr.model_mm.user_id_embedding.weight.detach()), got)
    # without its id row a user is a different one
    assert float((rec.embed_new((rp, ci)) - rec.E_u).abs().max() / rec.E_u.abs().max()) > 1e-3


def test_the_script_in_a_fresh_process(ops, served):
    from llmrec_amd import checkpoint as C
    from llmrec_amd.step_options import ENV_SWITCHES, TRAINER_SWITCHES
    s = served("graph")
    tmp, rec = s.tmp, s.rec
    rng = np.random.default_rng(6)
    hist = {0: rng.choice(80, 5, replace=False), 1: rng.choice(80, 30, replace=False), 3: np.array([7, 7, 2]), 4: np.arange(80)}     # row 2: empty
    (tmp / "hist.txt").write_text("".join("%d %d\n" % (q, i) for q, h in hist.items() for i in h))
    allow = np.sort(rng.choice(80, size=45, replace=False))
    np.save(str(tmp / "allow.npy"), allow.astype(np.int64))
    users = rng.integers(0, 96, 70)
    (tmp / "users.txt").write_text("".join("%d\n" % u for u in users))
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES + TRAINER_SWITCHES + tuple(C.CHECKPOINT_SWITCHES)}
    env.update(ENVS["graph"])
    argv = golden_argv(GoldenCase("nf_tiny")) + FLAGS + ["--epoch", "2"]
    head = [sys.executable, os.path.join(ROOT, "recommend.py"), "--checkpoint", s.best, "--topk", "20", "--allow_items", str(tmp / "allow.npy")]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    r = subprocess.run(head + ["--histories", str(tmp / "hist.txt"), "--out", str(tmp / "new.npz")] + argv, cwd=str(tmp), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(str(tmp / "new.npz"))
    items, scores = rec.recommend_new([hist.get(q, ()) for q in range(5)], 20, allow_items=allow)
    assert sorted(z.files) == ["items", "rows", "scores"] and np.array_equal(z["rows"], np.arange(5)) and z["items"].dtype == np.int64
    assert np.array_equal(z["items"], items.cpu().numpy()) and np.array_equal(bits(z["scores"]), bits(scores.cpu().numpy()))
    assert (z["items"][:4, 0] >= 0).all() and (z["items"][4] == -1).all() and not np.isin(z["items"][1], hist[1]).any()

    # --users: the file of before
    r = subprocess.run(head + ["--users", str(tmp / "users.txt"), "--out", str(tmp / "old.npz")] + argv, cwd=str(tmp), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(str(tmp / "old.npz"))
    items, scores = rec.recommend(users, 20, allow_items=allow)
    assert sorted(z.files) == ["items", "scores", "users"] and np.array_equal(z["users"], users)
    assert np.array_equal(z["items"], items.cpu().numpy()) and np.array_equal(bits(z["scores"]), bits(scores.cpu().numpy()))
