"""llmrec_bpr_prune_fwd_wide_f32 on the GPU: the multi-block selection against (a) the capped entry points, bit for bit, wherever both
exist, (b) the numpy restatement of the selection (tests/_select_ref.py) beyond LLMREC_BPR_MAX_B on crafted lists, bit for bit, and
(c) oracle.bpr_loss in float64 through ops.bpr_prune, forward and backward, within the bounds of tests/test_gpu_ops.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from tests import _select_ref as S

DEV = "cuda"
U, I, D = 300, 500, 64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


_TABLES = {}


def tables(d=D):
    """the 300 x d / 500 x d tables, made once per width and never written"""
    if d not in _TABLES:
        rng = np.random.default_rng(1000 + d)
        _TABLES[d] = (torch.tensor((rng.standard_normal((U, d)) * 0.3).astype(np.float32)),
                      torch.tensor((rng.standard_normal((I, d)) * 0.3).astype(np.float32)))
    return _TABLES[d]


def batch(B, seed=0):
    rng = np.random.default_rng(seed + B)
    return tuple(torch.tensor(rng.integers(0, n, size=B)) for n in (U, I, I))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """bit-equal, NaN counting as equal to NaN (k = 0: the empty mean)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))


def capped(ops, Eu, Ei, idx, remember, n_valid=None):
    B = idx[0].numel()
    out = torch.zeros(2, device=DEV); saved = torch.zeros(ops.bpr_saved_floats(B), device=DEV)
    ops._lib.call("llmrec_bpr_prune_fwd_f32", ops._p(Eu), ops._ld(Eu), ops._p(Ei), ops._ld(Ei), Eu.shape[1], *(ops._p(x) for x in idx), B,
                  ops._p(n_valid), float(remember), 1e-5, 64.0, ops._p(out), ops._p(saved), ops._stream())
    return out, saved


def sharded(ops, name, Eu, Ei, idx, remember, global_m, offset, scores_only, saved=None, n_valid=None, ws=None, out=None):
    """one call of llmrec_bpr_prune_fwd_sharded_f32 or llmrec_bpr_prune_fwd_wide_f32 (same leading arguments)"""
    B = idx[0].numel()
    out = torch.zeros(2, device=DEV) if out is None else out
    saved = torch.zeros(ops.bpr_saved_floats(B), device=DEV) if saved is None else saved
    args = [ops._p(Eu), ops._ld(Eu), ops._p(Ei), ops._ld(Ei), Eu.shape[1], *(ops._p(x) for x in idx), B, float(remember), 1e-5, 64.0,
            ops._p(global_m), 0 if global_m is None else global_m.numel(), int(offset), int(scores_only), ops._p(out), ops._p(saved)]
    if name == "wide":
        if ws is None and not scores_only:
            ws = ops.bpr_wide_workspace(B if global_m is None else global_m.numel(), DEV)
            ws.fill_(0xA5)                                             # the entry point initialises what it reads
        ops._lib.call("llmrec_bpr_prune_fwd_wide_f32", *args, ops._p(n_valid), ops._p(ws), 0 if ws is None else ws.numel(), ops._stream())
    else:
        ops._lib.call("llmrec_bpr_prune_fwd_sharded_f32", *args, ops._stream())
    return out, saved


# --------------------------------------------------------------------------------------------
# 1. the same bits where both paths exist
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remember", [0.29, 1.0])
@pytest.mark.parametrize("B", [35, 1126, 4096])
def test_wide_equals_the_capped_forward_bit_for_bit(ops, B, remember):
    Eu, Ei = (t.to(DEV) for t in tables())
    idx = tuple(x.to(DEV) for x in batch(B))
    o0, s0 = capped(ops, Eu, Ei, idx, remember)
    o1, s1 = sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 0)
    assert torch.equal(bits(o0), bits(o1)) and torch.equal(bits(s0), bits(s1))
    assert int((s1[:B] != 0).sum()) == S.k_of(remember, B)


@pytest.mark.parametrize("remember", [0.29, 1.0])
def test_wide_equals_the_capped_two_pass_form_bit_for_bit(ops, remember):
    Eu, Ei = (t.to(DEV) for t in tables())
    B, W = 1000, 3
    idx = tuple(x.to(DEV) for x in batch(W * B, seed=5))
    got = {}
    for name in ("sharded", "wide"):
        s1 = [sharded(ops, name, Eu, Ei, tuple(x[r * B:(r + 1) * B] for x in idx), remember, None, 0, 1)[1] for r in range(W)]
        global_m = torch.cat([s[B + 4:2 * B + 4] for s in s1]).contiguous()
        got[name] = [sharded(ops, name, Eu, Ei, tuple(x[r * B:(r + 1) * B] for x in idx), remember, global_m, r * B, 0, saved=s1[r])
                     for r in range(W)]
    for (o0, s0), (o1, s1) in zip(got["sharded"], got["wide"]):
        assert torch.equal(bits(o0), bits(o1)) and torch.equal(bits(s0), bits(s1))
    assert sum(int((s[:B] != 0).sum()) for _, s in got["wide"]) == S.k_of(remember, W * B)


# --------------------------------------------------------------------------------------------
# 2. the selection is exact beyond the cap (crafted lists)
# --------------------------------------------------------------------------------------------
def crafted(name, B):
    """(list, remember)"""
    rng = np.random.default_rng(B + len(name))
    rnd = (-5.0 * rng.random(B)).astype(np.float32)
    if name == "random":
        return rnd, 0.29
    if name == "all_equal":                                            # keep = the first k indices; the tie group spans every block
        return np.full(B, -0.7, dtype=np.float32), 0.29
    if name == "tie_group_at_threshold":                               # 500 below, 3000 equal, the rest above; k = 2000: r = 1500, strictly inside
        m = np.concatenate([-6.0 - rng.random(500), np.full(3000, -1.0), -0.5 * rng.random(B - 3500)]).astype(np.float32)
        assert S.k_of(2000.5 / B, B) == 2000
        return m[rng.permutation(B)], 2000.5 / B
    if name == "last_digit_only":                                      # equal in their top 24 bits
        return (np.uint32(0xBFC00000) | rng.integers(0, 256, size=B).astype(np.uint32)).view(np.float32), 0.29
    if name == "top_digit_only":                                       # every top byte that leaves a finite normal number, both signs, one tail
        top = rng.choice(np.r_[0x00:0x7F, 0x80:0xFF], size=B).astype(np.uint32)
        return ((top << np.uint32(24)) | np.uint32(0x00B45678)).view(np.float32), 0.5
    if name == "zeros_and_inf":
        m = rng.choice(np.array([-0.0, 0.0], dtype=np.float32), size=B)
        m[rng.choice(B, size=5, replace=False)] = -np.inf
        return m, 0.5
    if name == "k_0":
        return rnd, 1e-5
    if name == "k_all":
        return rnd, 1.0
    if name == "k_1":
        return rnd, 1.5 / B
    if name == "k_all_but_one":
        return rnd, (B - 0.5) / B
    raise KeyError(name)


VECTORS = ["random", "all_equal", "tie_group_at_threshold", "last_digit_only", "top_digit_only", "zeros_and_inf", "k_0", "k_all", "k_1",
           "k_all_but_one"]
_PASS1 = {}


def pass1(ops, B):
    """pass 1 of the wide entry at B (once per size): the saved block with the real scores, kept on the host"""
    if B not in _PASS1:
        Eu, Ei = (t.to(DEV) for t in tables())
        idx = tuple(x.to(DEV) for x in batch(B, seed=9))
        _PASS1[B] = (idx, sharded(ops, "wide", Eu, Ei, idx, 0.5, None, 0, 1)[1].cpu())
    return _PASS1[B]


@pytest.mark.parametrize("name", VECTORS)
@pytest.mark.parametrize("B", [4097, 8200])
def test_selection_is_exact_beyond_the_cap(ops, B, name):
    Eu, Ei = (t.to(DEV) for t in tables())
    idx, s1 = pass1(ops, B)
    m, remember = crafted(name, B)
    k = S.k_of(remember, B)
    assert {"k_0": 0, "k_all": B, "k_1": 1, "k_all_but_one": B - 1}.get(name, k) == k and (0 < k < B or name in ("k_0", "k_all"))
    saved = s1.clone()
    saved[B + 4:2 * B + 4] = torch.from_numpy(m)
    sg = saved[2 * B + 4:3 * B + 4].numpy().copy()
    global_m = torch.from_numpy(m).to(DEV)
    out, saved = sharded(ops, "wide", Eu, Ei, idx, remember, global_m, 0, 0, saved=saved.to(DEV))
    out, saved = out.cpu().numpy(), saved.cpu().numpy()
    keep, coef, kept_m, share = S.expected(m, sg, remember)
    assert int(keep.sum()) == k
    assert np.array_equal(saved[:B] != 0, keep)                          # (sg = sigmoid(-x) > 0: a kept coefficient is never zero)
    assert same_bits(saved[:B], coef)
    assert same_bits(saved[2 * B + 4:3 * B + 4], kept_m)
    assert same_bits(out[:1], np.array([share])), (out[0], share)
    assert saved[B + 3] == np.float32(k)


# --------------------------------------------------------------------------------------------
# 3. offsets: two ranks of one global list
# --------------------------------------------------------------------------------------------
def test_two_ranks_select_disjoint_shares_of_one_global_list(ops):
    Eu, Ei = (t.to(DEV) for t in tables())
    B, W, remember = 4100, 2, 0.29
    rng = np.random.default_rng(3)
    m = np.round(-4.0 * rng.random(W * B), 2).astype(np.float32)        # two decimals: hundreds of ties across the two ranks
    k = S.k_of(remember, W * B)
    want = S.keep_mask(m, remember)
    global_m = torch.from_numpy(m).to(DEV)
    keeps, shares = [], []
    for r in range(W):
        idx = tuple(x.to(DEV) for x in batch(B, seed=20 + r))
        _, saved = sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 1)
        saved[B + 4:2 * B + 4] = global_m[r * B:(r + 1) * B]
        out, saved = sharded(ops, "wide", Eu, Ei, idx, remember, global_m, r * B, 0, saved=saved)
        keeps.append((saved[:B] != 0).cpu().numpy()); shares.append(float(out[0]))
    got = np.concatenate(keeps)
    assert int(got.sum()) == k and np.array_equal(got, want)
    mean = -m[want].astype(np.float64).sum() / k
    assert abs(sum(shares) - mean) < 2e-6 * abs(mean)


def _select_as_ranks(ops, m, sizes, remember):
    """the list m cut into ranks of the given sizes, each selected by pass 2 at its offset: (union keep mask, the shares of out2[0])"""
    Eu, Ei = (t.to(DEV) for t in tables())
    global_m = torch.from_numpy(m).to(DEV)
    keeps, shares, off = [], [], 0
    for r, B in enumerate(sizes):
        idx = tuple(x.to(DEV) for x in batch(B, seed=30 + r))
        _, saved = sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 1)
        saved[B + 4:2 * B + 4] = global_m[off:off + B]
        out, saved = sharded(ops, "wide", Eu, Ei, idx, remember, global_m, off, 0, saved=saved)
        keeps.append((saved[:B] != 0).cpu().numpy()); shares.append(float(out[0]))
        off += B
    assert off == len(m)
    return np.concatenate(keeps), shares


def _tie_lists(sizes):
    """(name, list, k): tie groups whose r-th member lies a few entries behind a rank boundary - a boundary that is no multiple of the
    selection's 8 entries per thread, so one thread's entries belong to two ranks"""
    Bg, bounds = sum(sizes), np.cumsum(sizes)[:-1]
    rng = np.random.default_rng(Bg)
    for bd in bounds:
        assert bd % 8 != 0
        for extra in (1, 2, 5):
            yield "all_equal", np.full(Bg, -0.7, dtype=np.float32), int(bd) + extra
            m = np.full(Bg, -0.5, dtype=np.float32)
            m[bd - 1500:bd + 1500] = -1.0                                # 1500 equals in front of the boundary, 1500 behind it
            free = np.setdiff1d(np.arange(Bg), np.arange(bd - 1500, bd + 1500))
            m[rng.choice(free, size=500, replace=False)] = (-6.0 - rng.random(500)).astype(np.float32)
            yield "tie_group_across_boundary", m, 500 + 1500 + extra
    m, remember = crafted("tie_group_at_threshold", Bg)                  # the permuted group: r wherever it falls
    yield "tie_group_at_threshold", m, S.k_of(remember, Bg)


@pytest.mark.parametrize("sizes", [(4100, 4100), (4099, 4097, 4101)])
def test_ties_at_the_threshold_across_rank_boundaries(ops, sizes):
    """Among the equals at the threshold exactly the r of lowest GLOBAL index are kept, also where the r-th lies just behind a rank
    boundary: the union of the ranks' keep masks is the reference's and has exactly k members."""
    Bg = sum(sizes)
    for name, m, k in _tie_lists(sizes):
        remember = (k + 0.5) / Bg
        assert S.k_of(remember, Bg) == k
        want = S.keep_mask(m, remember)
        got, shares = _select_as_ranks(ops, m, sizes, remember)
        assert int(got.sum()) == k and np.array_equal(got, want), (name, k, int(got.sum()), np.flatnonzero(got != want)[:8])
        mean = -m[want].astype(np.float64).sum() / k
        assert abs(sum(shares) - mean) < 2e-6 * abs(mean), (name, k)


# --------------------------------------------------------------------------------------------
# 4. the batch count on the device
# --------------------------------------------------------------------------------------------
def test_device_batch_count(ops):
    Eu, Ei = (t.to(DEV) for t in tables())
    cap, B, remember = 6000, 4500, 0.29
    idx = tuple(x.to(DEV) for x in batch(cap, seed=40))
    nv = torch.tensor([B], dtype=torch.int32, device=DEV)
    saved = torch.full((ops.bpr_saved_floats(cap),), 7.0, device=DEV)   # stale values where the padding's zeros belong
    o1, s1 = sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 0, saved=saved, n_valid=nv)
    o0, s0 = sharded(ops, "wide", Eu, Ei, tuple(x[:B] for x in idx), remember, None, 0, 0)
    assert torch.equal(bits(o0), bits(o1))
    assert torch.equal(bits(s0[:B]), bits(s1[:B])) and torch.equal(bits(s0[B:B + 4]), bits(s1[cap:cap + 4]))
    assert torch.equal(bits(s0[2 * B + 4:3 * B + 4]), bits(s1[2 * cap + 4:2 * cap + 4 + B]))
    assert int((s1[:B] != 0).sum()) == S.k_of(remember, B)
    assert not s1[B:cap].any() and not s1[2 * cap + 4 + B:3 * cap + 4].any()


# --------------------------------------------------------------------------------------------
# 5. ops.bpr_prune, forward and backward
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,d", [(4097, 64), (8200, 64), (4097, 128), (8200, 128)])
def test_bpr_prune_forward_backward_beyond_the_cap(ops, B, d):
    """Against oracle.bpr_loss in float64, with the bounds of tests/test_gpu_ops.py::test_bpr_prune_forward_backward (2e-6 relative on
    both values, 2e-5 rel_err on both gradients). The batch draws from 300 users and 500 items: every destination row is hit dozens
    of times."""
    drop = 0.71
    Eu, Ei = tables(d)
    users, pos, neg = batch(B, seed=60 + d)
    a = Eu.double().requires_grad_(True); b = Ei.double().requires_grad_(True)
    mf, emb = O.bpr_loss(a[users], b[pos], b[neg], O.Config(batch_size=1024, decay=1e-5, prune_loss_drop_rate=drop))
    (0.7 * mf + 1.3 * emb).backward()
    mf, emb = mf.detach(), emb.detach()

    def run():
        Eug = Eu.to(DEV).requires_grad_(True); Eig = Ei.to(DEV).requires_grad_(True)
        out = ops.bpr_prune(Eug, Eig, users.to(DEV), pos.to(DEV), neg.to(DEV), drop, 1e-5, 1024)
        (0.7 * out[0] + 1.3 * out[1]).backward()
        return out.detach().cpu(), Eug.grad.cpu(), Eig.grad.cpu()

    def rel_err(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)

    out, gu, gi = run()
    figures = (abs(float(out[0]) - float(mf)) / abs(float(mf)), abs(float(out[1]) - float(emb)) / abs(float(emb)),
               rel_err(gu, a.grad), rel_err(gi, b.grad))
    print("bpr_prune wide B=%d d=%d: mf %.3g emb %.3g dEu %.3g dEi %.3g" % ((B, d) + figures))
    assert figures[0] < 2e-6 and figures[1] < 2e-6
    assert figures[2] < 2e-5 and figures[3] < 2e-5
    out2, gu2, gi2 = run()
    assert torch.equal(out, out2) and torch.equal(gu, gu2) and torch.equal(gi, gi2)


# --------------------------------------------------------------------------------------------
# 6. graph capture
# --------------------------------------------------------------------------------------------
def test_wide_forward_replays_from_a_captured_graph(ops):
    Eu, Ei = (t.to(DEV) for t in tables())
    cap, remember = 5000, 0.29
    idx = tuple(x.to(DEV) for x in batch(cap, seed=80))
    nv = torch.tensor([cap], dtype=torch.int32, device=DEV)
    out = torch.zeros(2, device=DEV); saved = torch.zeros(ops.bpr_saved_floats(cap), device=DEV)
    ws = ops.bpr_wide_workspace(cap, DEV)
    call = lambda: sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 0, saved=saved, n_valid=nv, ws=ws, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for n in (4200, 4999):
        nv.fill_(n); saved.zero_(); out.zero_()
        g.replay()
        torch.cuda.synchronize()
        o1, s1 = out.clone(), saved.clone()
        o0, s0 = sharded(ops, "wide", Eu, Ei, idx, remember, None, 0, 0, n_valid=nv)
        assert torch.equal(bits(o0), bits(o1)) and torch.equal(bits(s0), bits(s1))
        assert int((s1[:cap] != 0).sum()) == S.k_of(remember, n)
