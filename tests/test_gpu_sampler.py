"""The device BPR sampler (llmrec_sample_bpr, llmrec_sample_batch: csrc/bpr.hip) against its numpy restatement tests/_sampler_ref.py,
BIT FOR BIT: the contract is integer, so every comparison is torch.equal - users, positives, negatives, n_valid, the step counter, the
zero padding and the untouched tail of the buffers. tests/test_sampler_ref_cpu.py shows that the restatement's generator is
Philox4x32-10 and that the design it states draws uniformly; this file shows that the kernels ARE that design, at the shapes where
they could go wrong: the sizes where the Feistel domain grows, 64-bit seeds and steps, rows of length 1 / 2 / I - 3 / I - 1 / I, the
strided loop beyond 1024 slots, the multi-chunk compaction of the augmented triples, slices that start mid-wavefront, graph replay."""
import numpy as np
import pytest
import torch

from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS_STEPS = [(2022, 0), (2022, 1), (0, 0), (2 ** 32 + 5, 3), (2 ** 63 + 12345, 2 ** 32 + 7), (2 ** 64 - 1, 2 ** 64 - 2)]
SENTINEL, TAIL = -7, 9


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


class Graph:
    """Train rows (sorted, per user; users not listed have none) as numpy CSR for the restatement and as an ops.Csr for the kernels."""

    def __init__(self, ops, n_users, n_items, rows):
        self.U, self.I = n_users, n_items
        degs = np.zeros(n_users, dtype=np.int64)
        for u, r in rows.items():
            degs[u] = len(r)
        self.rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
        self.colidx = np.concatenate([np.asarray(rows[u], dtype=np.int64) for u in sorted(rows)] + [np.zeros(0, dtype=np.int64)])
        self.table = R.edge_table(self.rowptr, self.colidx, n_items)
        self.csr = ops.Csr(n_users, n_items, torch.tensor(self.rowptr, dtype=torch.int32, device=DEV),
                           torch.tensor(self.colidx, dtype=torch.int32, device=DEV), None, None, None)


def random_graph(ops, rng, n_users, n_items, users, max_deg=12):
    return Graph(ops, n_users, n_items, {int(u): np.sort(rng.choice(n_items, size=int(rng.integers(1, max_deg)), replace=False)) for u in users})


def signed64(x):
    """A 64-bit word as the int64 a torch tensor holds."""
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >= 2 ** 63 else x


def assert_bpr_equals_restatement(ops, g, exist, seed, step, B):
    got = ops.sample_bpr(seed, step, torch.tensor(exist, dtype=torch.int64, device=DEV), g.I, g.csr, B)
    want = R.sample_bpr(seed, step, exist, g.I, g.rowptr, g.colidx, B, table=g.table)
    for name, a, b in zip(("users", "pos", "neg"), got, want):
        assert torch.equal(a.cpu(), torch.from_numpy(b)), (name, len(exist), B, seed, step)
    return want


def run_batch(ops, g, exist, seed, step, B_global, begin, B, n_aug, aug_pos=None, aug_neg=None):
    """One llmrec_sample_batch launch into sentinel-filled buffers of B + n_aug + TAIL entries, compared with the restatement in full.
    Returns the restatement's (users, pos, neg, n_valid)."""
    step_dev = torch.tensor([signed64(step)], dtype=torch.int64, device=DEV)
    u, p, n = (torch.full((B + n_aug + TAIL,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
    nv = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    ap = torch.tensor(aug_pos, dtype=torch.int64, device=DEV) if aug_pos is not None else None
    an = torch.tensor(aug_neg, dtype=torch.int64, device=DEV) if aug_neg is not None else None
    ops.sample_batch(seed, step_dev, torch.tensor(exist, dtype=torch.int64, device=DEV), g.I, g.csr, B_global, begin, B, n_aug, ap, an, u, p, n, nv)
    wu, wp, wn, w_valid, w_step = R.sample_batch(seed, step, exist, g.I, g.rowptr, g.colidx, B_global, begin, B, n_aug, aug_pos, aug_neg)
    what = (len(exist), seed, step, B_global, begin, B, n_aug)
    assert int(nv) == w_valid, ("n_valid", int(nv), w_valid) + what
    assert int(step_dev) == signed64(w_step), ("step counter",) + what
    tail = torch.full((TAIL,), SENTINEL, dtype=torch.int64)
    for name, a, b in zip(("users", "pos", "neg"), (u, p, n), (wu, wp, wn)):
        a = a.cpu()
        assert torch.equal(a[:B], torch.from_numpy(b[:B])), (name, "slice") + what
        assert torch.equal(a[B:w_valid], torch.from_numpy(b[B:w_valid])), (name, "augmented") + what
        assert not a[w_valid:B + n_aug].any() and not b[w_valid:].any(), (name, "padding") + what
        assert torch.equal(a[B + n_aug:], tail), (name, "tail overwritten") + what
    return wu, wp, wn, w_valid


def aug_pairs(rng, g, lo=-3, hi=None):
    hi = int(1.3 * g.I) if hi is None else hi
    return rng.integers(lo, hi, size=g.U), rng.integers(lo, hi, size=g.U)


# ------------------------------------------------------------------------------------------
# llmrec_sample_bpr
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_exist", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1024, 1025, 13187])
def test_sample_bpr_equals_restatement(ops, n_exist):
    """Every size where keyed_perm's domain changes (4^h and 4^h + 1), n_exist = 1, 2, 3, B == n_exist exactly, B = 1, and B > n_exist
    (with replacement) for the small lists; exist_users = every third user id, so a slot is never its own id."""
    rng = np.random.default_rng(n_exist)
    exist = np.arange(1, 3 * n_exist, 3)
    g = random_graph(ops, rng, 3 * n_exist, 211, exist)
    Bs = {1, min(n_exist, 1024)}
    if n_exist <= 4096:
        Bs.add(n_exist)
    if n_exist <= 17:
        Bs |= {n_exist + 1, 300}
    for B in sorted(Bs):
        for seed, step in SEEDS_STEPS:
            u, p, q = assert_bpr_equals_restatement(ops, g, exist, seed, step, B)
            if B <= n_exist:
                assert len(set(u.tolist())) == B
            assert set(u.tolist()) <= set(exist.tolist())


def test_upper_words_of_seed_and_step_reach_the_stream(ops):
    rng = np.random.default_rng(5)
    exist = np.arange(0, 1400, 2)
    g = random_graph(ops, rng, 1400, 300, exist)
    ex = torch.tensor(exist, dtype=torch.int64, device=DEV)
    base = [t.cpu() for t in ops.sample_bpr(5, 3, ex, g.I, g.csr, 256)]
    for seed, step in ((5 + 2 ** 32, 3), (5 + 2 ** 63, 3), (5, 3 + 2 ** 32), (5, 3 + 2 ** 63)):
        other = [t.cpu() for t in ops.sample_bpr(seed, step, ex, g.I, g.csr, 256)]
        for a, b in zip(base, other):                          # users, positives and negatives each depend on the upper words
            assert not torch.equal(a, b), (seed, step)
        assert_bpr_equals_restatement(ops, g, exist, seed, step, 256)
    # with replacement too (the other user branch)
    a = ops.sample_bpr(5, 3, ex[:40], g.I, g.csr, 256)[0]
    for seed, step in ((5 + 2 ** 32, 3), (5, 3 + 2 ** 32)):
        assert not torch.equal(a, ops.sample_bpr(seed, step, ex[:40], g.I, g.csr, 256)[0])
        assert_bpr_equals_restatement(ops, g, exist[:40], seed, step, 256)


def test_rows_of_length_1_2_and_nearly_all_items(ops):
    """Rows of length 1, 2, I - 3 and I - 1 beside ordinary ones: the positive at both ends of the row, the negative by heavy rejection
    (the restatement confirms that a slot looked at more than 4 candidates, i.e. the kernel crossed a Philox refill)."""
    rng = np.random.default_rng(17)
    I = 300
    rows = {u: np.sort(rng.choice(I, size=d, replace=False)) for u, d in ((2, 1), (4, 2), (6, I - 3), (8, I - 1), (10, 20), (12, 37))}
    rows[14] = np.array([0, I - 1])                            # both ends of the item range are train items ...
    rows[16] = np.arange(1, I - 1)                             # ... or the only free ones
    g = Graph(ops, 20, I, rows)
    exist = np.array(sorted(rows))
    for B in (8, 512):                                         # without / with replacement
        for seed, step in SEEDS_STEPS:
            u, p, q = assert_bpr_equals_restatement(ops, g, exist, seed, step, B)
            tries = R.sample_bpr(seed, step, exist, I, g.rowptr, g.colidx, B, return_tries=True, table=g.table)[3]
            assert tries.max() < R.MAX_TRIES
            if B == 512:                                       # ~64 draws per user: refills crossed; every item of the short rows / of the small complements shows up
                assert tries[u == 8].max() > 4 and tries[u == 6].max() > 4
                assert set(p[u == 4].tolist()) == set(rows[4].tolist()) and set(q[u == 6].tolist()) == set(range(I)) - set(rows[6].tolist())
                assert set(q[u == 16].tolist()) == {0, I - 1} and set(p[u == 14].tolist()) == {0, I - 1}


def test_a_row_that_covers_every_item_ends_after_4096_candidates(ops):
    """The reference's loop would never end; the kernel's is bounded (`tries < 4096`, whatever n_items is) and returns the restatement's
    4096th candidate, the same one every time."""
    I = 40
    rng = np.random.default_rng(3)
    g = Graph(ops, 6, I, {1: np.arange(I), 3: np.sort(rng.choice(I, size=7, replace=False)), 5: np.arange(I)})
    exist = np.array([1, 3, 5])
    for B in (3, 64):
        u, p, q = assert_bpr_equals_restatement(ops, g, exist, 2022, B, B)
        tries = R.sample_bpr(2022, B, exist, I, g.rowptr, g.colidx, B, return_tries=True, table=g.table)[3]
        assert (tries[u != 3] == R.MAX_TRIES).all() and (tries[u == 3] < 100).all()
    one = Graph(ops, 4, 1, {0: [0], 2: [0]})                  # one item, in every row: the same case
    for B in (2, 33):
        u, p, q = assert_bpr_equals_restatement(ops, one, np.array([0, 2]), 9, 1, B)
        assert not p.any() and not q.any()


# ------------------------------------------------------------------------------------------
# llmrec_sample_batch
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(ops):
    rng = np.random.default_rng(4096)
    exist = np.arange(1, 10001, 2)                             # 5000 users with train items
    return random_graph(ops, rng, 10001, 500, exist), exist


@pytest.mark.parametrize("B", [1, 96, 1000, 1024, 1025, 2048, 4096])
def test_sample_batch_equals_restatement(ops, big, B):
    """The single block strides over B > 1024 slots, and over n_aug > 1024 draws in chunks whose kept counts carry over (n_aug = 1024: one
    full chunk; 1025, 2048: a second; 2500, 4096: a third and more). Pair ids in [-3, 1.3 I): negative, valid and too-large ids all occur."""
    g, exist = big
    rng = np.random.default_rng(B)
    ap, an = aug_pairs(rng, g)
    n_augs = sorted({a for a in (0, 1, 31, B) if a <= B} | ({1024, 1025, 2500} if B == 4096 else set()))
    for i, n_aug in enumerate(n_augs):
        seed, step = SEEDS_STEPS[(i + B) % len(SEEDS_STEPS)]
        wu, wp, wn, nv = run_batch(ops, g, exist, seed, step, B, 0, B, n_aug, ap, an)
        if n_aug >= 31:
            assert B < nv < B + n_aug                          # some pairs kept, some dropped
        if n_aug == B and B >= 96:                             # every user of the slice was drawn: pairs with an id below zero were
            below = set(wu[:B][(ap[wu[:B]] < 0) | (an[wu[:B]] < 0)].tolist())   # among them, and none of them was kept
            assert below and not below & set(wu[B:nv].tolist())


@pytest.mark.parametrize("B,n_aug", [(96, 31), (1025, 1025), (4096, 2500)])
def test_sample_batch_all_pairs_valid_and_no_pair_valid(ops, big, B, n_aug):
    g, exist = big
    rng = np.random.default_rng(B + n_aug)
    ap, an = aug_pairs(rng, g, 0, g.I)
    assert run_batch(ops, g, exist, 2022, 4, B, 0, B, n_aug, ap, an)[3] == B + n_aug
    for ap, an in (aug_pairs(rng, g, g.I, 2 * g.I), aug_pairs(rng, g, -5, 0), (ap, np.full(g.U, -1)), (np.full(g.U, g.I), an)):
        assert run_batch(ops, g, exist, 2022, 4, B, 0, B, n_aug, ap, an)[3] == B   # n_valid == B, all padding zero (checked in run_batch)


def test_sample_batch_with_replacement(ops, big):
    g, exist = big
    ap, an = aug_pairs(np.random.default_rng(1), g)
    run_batch(ops, g, exist[:50], 77, 2, 96, 0, 96, 31, ap, an)      # B > n_exist: users repeat, the augmented draws are distinct SLOTS
    run_batch(ops, g, exist[:1], 77, 2, 1100, 0, 1100, 1100, ap, an)


@pytest.mark.parametrize("cuts", [[96], [96, 96], [96, 96, 96], [96] * 8, [1100, 1100, 1100], [100, 37, 119]], ids=lambda c: "x".join(map(str, c)))
def test_ranks_slices_tile_the_global_batch(ops, big, cuts):
    """The same (seed, step) gives the same global batch whatever the number of ranks, also for slices that start and end inside a
    wavefront (100 | 37 | 119 of 256); each slice's augmented users come from that slice."""
    g, exist = big
    ap, an = aug_pairs(np.random.default_rng(len(cuts)), g)
    B_global = sum(cuts)
    for seed, step in ((2 ** 63 + 12345, 2 ** 32 + 7), (2022, 6)):
        whole = R.sample_bpr(seed, step, exist, g.I, g.rowptr, g.colidx, B_global, table=g.table)
        assert len(set(whole[0].tolist())) == B_global
        begin, parts = 0, []
        for B in cuts:
            n_aug = B // 3
            wu, wp, wn, nv = run_batch(ops, g, exist, seed, step, B_global, begin, B, n_aug, ap, an)   # == the device's buffers (run_batch)
            parts.append((wu[:B], wp[:B], wn[:B]))
            assert set(wu[B:nv].tolist()) <= set(wu[:B].tolist()) and len(set(wu[B:nv].tolist())) == nv - B
            begin += B
        for k in range(3):
            assert np.array_equal(np.concatenate([part[k] for part in parts]), whole[k])


def test_graph_replay_advances_the_64_bit_counter(ops, big):
    """One captured launch (a single-branch graph, as the fused step's) replayed 5 times from counter 2^32 - 2: every replay equals the
    restatement at its step, the counter crosses 2^32 inside the replays and ends at 2^32 + 3."""
    from llmrec_amd.fused import _capture_without_gc
    g, exist = big
    B, n_aug, seed, first = 1500, 1200, 2 ** 32 + 5, 2 ** 32 - 2
    ap, an = aug_pairs(np.random.default_rng(2), g)
    ex = torch.tensor(exist, dtype=torch.int64, device=DEV)
    apd, and_ = torch.tensor(ap, device=DEV), torch.tensor(an, device=DEV)
    step_dev = torch.tensor([first], dtype=torch.int64, device=DEV)
    u, p, n = (torch.full((B + n_aug + TAIL,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.sample_batch(seed, step_dev, ex, g.I, g.csr, B, 0, B, n_aug, apd, and_, u, p, n, nv)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capture_without_gc(graph, False):
        ops.sample_batch(seed, step_dev, ex, g.I, g.csr, B, 0, B, n_aug, apd, and_, u, p, n, nv)
    step_dev.fill_(first)
    for k in range(5):
        graph.replay()
        torch.cuda.synchronize()
        wu, wp, wn, w_valid, w_step = R.sample_batch(seed, first + k, exist, g.I, g.rowptr, g.colidx, B, 0, B, n_aug, ap, an)
        assert int(step_dev) == w_step == first + k + 1 and int(nv) == w_valid
        for name, a, b in zip(("users", "pos", "neg"), (u, p, n), (wu, wp, wn)):
            assert torch.equal(a.cpu()[:B + n_aug], torch.from_numpy(b)), (name, k)
            assert (a.cpu()[B + n_aug:] == SENTINEL).all()
    assert int(step_dev) == 2 ** 32 + 3


def test_netflix_shape_twenty_steps_through_the_batcher(ops):
    """13 187 users x 17 366 items, B = 1024 and the augmented share engine.DeviceBatcher computes for the default rate: 20 consecutive
    steps of the batcher (device counter) equal the restatement."""
    from llmrec_amd import engine, synth
    U, I, B, seed = 13187, 17366, 1024, 2022
    r, c = synth.bipartite_edges(U, I, 68933, seed=7, max_deg=400)
    ux, begin = np.unique(r, return_index=True)               # (rows, cols) come sorted by (row, col)
    rows = {int(u): c[s:e] for u, s, e in zip(ux, begin, np.append(begin[1:], r.size))}
    g = Graph(ops, U, I, rows)
    exist = np.array(sorted(rows))
    assert exist.size == U
    ap, an = aug_pairs(np.random.default_rng(9), g)
    batcher = engine.DeviceBatcher(g.csr, torch.tensor(exist, device=DEV), I, B, torch.tensor(ap, device=DEV), torch.tensor(an, device=DEV),
                                   engine.Hyper().aug_sample_rate, seed)
    assert batcher.n_aug == 102
    for step in range(20):
        u, p, n, nv = batcher.next()
        wu, wp, wn, w_valid, w_step = R.sample_batch(seed, step, exist, I, g.rowptr, g.colidx, B, 0, B, batcher.n_aug, ap, an)
        assert int(nv) == w_valid and int(batcher.step_dev) == w_step == step + 1
        for a, b in zip((u, p, n), (wu, wp, wn)):
            assert torch.equal(a.cpu()[:w_valid], torch.from_numpy(b[:w_valid])) and not a.cpu()[w_valid:].any()
