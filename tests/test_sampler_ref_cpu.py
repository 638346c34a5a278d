"""CPU tests of tests/_sampler_ref.py, the numpy restatement the device sampler is pinned to (tests/test_gpu_sampler.py): the generator is
Philox4x32-10, the keyed permutation is a bijection, and the design the restatement states draws users, positives and negatives uniformly.
Everything here is a function of fixed seeds: a test passes for good or fails for good."""
import ctypes
import os

import numpy as np
import pytest

from tests import _sampler_ref as R

BIG_SEED, BIG_STEP = 2 ** 63 + 12345, 2 ** 32 + 7


def test_restatement_is_independent_of_the_package():
    imports = [ln.strip() for ln in open(R.__file__) if ln.strip().startswith(("import ", "from "))]
    assert imports == ["import numpy as np"], imports


def test_philox_known_answers():
    """The three philox4x32-10 vectors of Random123's kat_vectors (counter, key -> output): all-zero, all-ones, and the digits of pi.
    The restatement was written from the four published constants alone (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, ten rounds) and
    reproduced all twelve words at its first run."""
    kat = [
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in kat:
        got = " ".join("%08x" % int(w) for w in R.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key)
    # vectorised over the counter: element i of a batched call is the scalar call
    c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    o = R.philox4x32_10(c0, 7, 8, 9, 10, 11)
    for i in range(3):
        assert [int(w[i]) for w in o] == [int(w) for w in R.philox4x32_10(int(c0[i]), 7, 8, 9, 10, 11)]


PERM_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 13187, 65536, 65537]


@pytest.mark.parametrize("seed,step", [(2022, 0), (0, 0), (BIG_SEED, BIG_STEP)])
def test_keyed_perm_is_a_bijection(seed, step):
    for n in PERM_SIZES:
        img = R.keyed_perm(np.arange(n), n, seed, step)
        assert img.dtype == np.uint64 and np.array_equal(np.sort(img), np.arange(n, dtype=np.uint64)), n


def test_keyed_perm_domain_sizes_and_key_sensitivity():
    assert [R.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 256, 257, 1024, 1025, 4096, 4097, 65536, 65537)] == [1, 1, 1, 2, 2, 3, 4, 5, 5, 6, 6, 7, 8, 9]
    for n in (257, 4097, 13187):
        base = R.keyed_perm(np.arange(n), n, 2022, 0)
        for seed, step in ((2022, 1), (2022, 2 ** 32), (2022 + 2 ** 32, 0), (2022 + 2 ** 63, 0), (2023, 0)):
            assert not np.array_equal(base, R.keyed_perm(np.arange(n), n, seed, step)), (n, seed, step)
    # one step per point == one call per step
    steps = np.array([0, 1, 2 ** 32, 2 ** 64 - 1], dtype=np.uint64)
    x = np.array([5, 5, 5, 5])
    assert R.keyed_perm(x, 1000, 9, steps).tolist() == [int(R.keyed_perm([5], 1000, 9, int(t))[0]) for t in steps]


def _graph():
    """400 users x 300 items, degrees in [1, 60), and the four rows where an off-by-one shows: length 1, 2, I - 3, I - 1."""
    rng = np.random.default_rng(2022)
    U, I = 400, 300
    degs = rng.integers(1, 60, size=U)
    special = {11: 1, 123: 2, 200: I - 3, 399: I - 1}
    for u, d in special.items():
        degs[u] = d
    rows = [np.sort(rng.choice(I, size=int(d), replace=False)) for d in degs]
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    return U, I, rows, rowptr, np.concatenate(rows).astype(np.int64), sorted(special) + [0, 77]


def _chi2(obs, expected):
    obs = np.asarray(obs, dtype=np.float64)
    return float(((obs - expected) ** 2 / expected).sum())


def test_sampler_design_is_uniform():
    """Pearson chi-square of the restatement's draws against the uniform expectation, each below the 1 - 1e-6 quantile of its degrees of
    freedom (scipy.stats.chi2.isf(1e-6, dof): a derived bound - a correct sampler exceeds one of them with probability 1e-6).
    Seed 2022, steps 0 .. 31999, B = 100 of 400 users: every user is drawn ~8000 times, so the largest tracked table (299 cells) expects
    ~26.7 draws per cell. The step count comes from the "every cell is drawn" check: with an expectation >= 24 (asserted) a given cell stays
    empty with probability <= e^-24 = 3.8e-11, ~1800 tracked cells together < 1e-7.

    Statistic / bound, as the restatement yields them (the test prints them; `pytest -s`):
        users, all slots               (399 dof)  280.64 / 547.95   (drawn without replacement within a step: conservative)
        user of slot 0                 (399 dof)  420.52 / 547.95
        user of slot B - 1             (399 dof)  405.12 / 547.95
        user  11, row of   1:  positive always the one item          negative (298 dof)  304.05 / 428.75
        user 123, row of   2:  positive (  1 dof)    2.85 /  23.93   negative (297 dof)  317.15 / 427.56
        user 200, row of 297:  positive (296 dof)  280.58 / 426.36   negative (  2 dof)    2.05 /  27.63
        user 399, row of 299:  positive (298 dof)  293.53 / 428.75   negative always the one free item
        user   0, row of  42:  positive ( 41 dof)   38.82 /  99.17   negative (257 dof)  265.08 / 379.50
        user  77, row of  59:  positive ( 58 dof)   55.14 / 124.23   negative (240 dof)  225.01 / 358.88
    Every item of every tracked row, and of its complement, is drawn at least once (the check that catches an off-by-one at either end)."""
    from scipy.stats import chi2
    U, I, rows, rowptr, colidx, tracked = _graph()
    B, n_steps = 100, 32000
    users, pos, neg = R.sample_bpr_steps(2022, range(n_steps), np.arange(U), I, rowptr, colidx, B)
    assert users.shape == (n_steps, B)
    # every batch: distinct users, the positive in the row, the negative outside it
    assert (np.sort(users, axis=1)[:, 1:] != np.sort(users, axis=1)[:, :-1]).all()
    table = R.edge_table(rowptr, colidx, I)
    assert np.isin(users * I + pos, table).all() and not np.isin(users * I + neg, table).any()
    assert neg.min() >= 0 and neg.max() < I

    def check(name, obs, dof_cells):
        obs = np.asarray(obs)
        assert obs.size == dof_cells
        expected = obs.sum() / dof_cells
        assert expected >= 24, (name, expected)
        assert obs.min() >= 1, (name, "a cell was never drawn", int(obs.argmin()))
        if dof_cells > 1:
            stat, bound = _chi2(obs, expected), float(chi2.isf(1e-6, dof_cells - 1))
            print("%-28s dof %3d  chi2 %8.2f  bound %8.2f" % (name, dof_cells - 1, stat, bound))
            assert stat < bound, (name, stat, bound)

    check("users, all slots", np.bincount(users.ravel(), minlength=U), U)
    check("user of slot 0", np.bincount(users[:, 0], minlength=U), U)
    check("user of slot B - 1", np.bincount(users[:, B - 1], minlength=U), U)
    for u in tracked:
        at = users == u
        row = rows[u]
        comp = np.setdiff1d(np.arange(I), row)
        p_counts = np.bincount(pos[at], minlength=I)
        n_counts = np.bincount(neg[at], minlength=I)
        assert p_counts[comp].sum() == 0 and n_counts[row].sum() == 0
        check("positive of user %d (row %d)" % (u, row.size), p_counts[row], row.size)
        check("negative of user %d (row %d)" % (u, row.size), n_counts[comp], comp.size)


def test_rejection_gives_up_after_4096_candidates_and_crosses_refills():
    """A row that covers every item: the reference's loop would spin for ever; the contract is the 4096th candidate. A row that covers
    all items but three needs ~I / 3 candidates: the draw crosses many 4-word refills and still ends on a free item."""
    I = 40
    rowptr = np.array([0, I, 2 * I - 3], dtype=np.int64)
    colidx = np.concatenate([np.arange(I), np.arange(3, I)]).astype(np.int64)
    u, p, q, tries = R.sample_bpr(2022, 0, [0, 1], I, rowptr, colidx, 64, return_tries=True)        # B > n_exist: with replacement
    assert set(u.tolist()) == {0, 1}
    assert (tries[u == 0] == R.MAX_TRIES).all() and (tries[u == 1] < R.MAX_TRIES).all() and tries[u == 1].max() > 4
    assert set(q[u == 1].tolist()) <= {0, 1, 2}
    # the 4096th candidate: word 3 of refill 1023
    b = np.flatnonzero(u == 0)
    last = R.philox4x32_10(b, 0x55AA0003 + 1023, 0, 0, 2022, 0)[3]
    assert np.array_equal(q[u == 0], (last.astype(np.uint64) * np.uint64(I)) >> np.uint64(32))
    # one item, in the row: the same case
    u1, p1, q1, t1 = R.sample_bpr(3, 9, [0], 1, [0, 1], [0], 5, return_tries=True)
    assert u1.tolist() == [0] * 5 and p1.tolist() == [0] * 5 and q1.tolist() == [0] * 5 and (t1 == R.MAX_TRIES).all()


def test_sample_batch_slices_tile_the_global_batch_and_compact_the_pairs():
    U, I, rows, rowptr, colidx, _ = _graph()
    rng = np.random.default_rng(1)
    exist = np.arange(0, U, 2)
    ap, an = rng.integers(-3, int(1.3 * I), size=U), rng.integers(-3, int(1.3 * I), size=U)
    whole = R.sample_bpr(BIG_SEED, BIG_STEP, exist, I, rowptr, colidx, 128)
    begin = 0
    for B, n_aug in ((50, 50), (17, 0), (61, 13)):
        u, p, q, nv, nxt = R.sample_batch(BIG_SEED, BIG_STEP, exist, I, rowptr, colidx, 128, begin, B, n_aug, ap, an)
        assert nxt == BIG_STEP + 1 and u.size == B + n_aug
        for got, ref in zip((u, p, q), whole):
            assert np.array_equal(got[:B], ref[begin:begin + B])
        kept = nv - B
        au = u[B:nv]
        assert len(set(au.tolist())) == kept and set(au.tolist()) <= set(u[:B].tolist())
        assert np.array_equal(p[B:nv], ap[au]) and np.array_equal(q[B:nv], an[au])
        assert ((p[B:nv] >= 0) & (p[B:nv] < I) & (q[B:nv] >= 0) & (q[B:nv] < I)).all()
        assert not u[nv:].any() and not p[nv:].any() and not q[nv:].any()
        if n_aug == B:                                          # every user of the slice was drawn: the dropped ones are exactly the invalid pairs
            ok = (ap[u[:B]] >= 0) & (ap[u[:B]] < I) & (an[u[:B]] >= 0) & (an[u[:B]] < I)
            assert kept == int(ok.sum()) and 0 < kept < B
        begin += B
    assert R.sample_batch(1, 2 ** 64 - 1, exist, I, rowptr, colidx, 8, 0, 8, 0)[4] == 0          # the counter is a 64-bit word


def test_sampler_entry_points_check_their_arguments_without_a_gpu():
    """llmrec_sample_bpr / llmrec_sample_batch validate before they touch the device: a non-zero status and the entry point's name in
    llmrec_last_error(); B = 0 is a valid empty batch for llmrec_sample_bpr (nothing launched)."""
    from llmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libllmrec_hip.so is not built (python -m llmrec_amd.build)")
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                               # a non-null pointer for the checks behind the null test (never dereferenced:
    P = ctypes.cast(buf, ctypes.c_void_p)                       # every case below is refused before a launch)
    bpr = [
        (1, 0, 10, P, 5, P, P, -1, P, P, P, None),               # B < 0
        (1, 0, 0, P, 5, P, P, 4, P, P, P, None),                 # no users
        (1, 0, 10, P, 0, P, P, 4, P, P, P, None),                # no items
        (1, 0, 10, None, 5, P, P, 4, P, P, P, None),             # null pointers with B > 0
        (1, 0, 10, P, 5, P, None, 4, P, P, P, None),
        (1, 0, 10, P, 5, P, P, 4, P, P, None, None),
    ]
    for args in bpr:
        assert lib.llmrec_sample_bpr(*args) != 0, args
        assert b"sample_bpr" in lib.llmrec_last_error(), (args, lib.llmrec_last_error())
    assert lib.llmrec_sample_bpr(1, 0, 10, None, 5, None, None, 0, None, None, None, None) == 0
    batch = [
        ((1, P, 10, P, 5, P, P, 16, 0, 8, 9, P, P, P, P, P, P, None), b"sample_batch: bad sizes"),          # n_aug > B
        ((1, P, 10, P, 5, P, P, 16, 9, 8, 0, P, P, P, P, P, P, None), b"sample_batch: bad sizes"),          # slice_begin + B > B_global
        ((1, P, 10, P, 5, P, P, 16, 0, 0, 0, P, P, P, P, P, P, None), b"sample_batch: bad sizes"),          # B = 0
        ((1, P, 10, P, 5, P, P, 16, -1, 8, 0, P, P, P, P, P, P, None), b"sample_batch: bad sizes"),
        ((1, None, 10, P, 5, P, P, 16, 0, 8, 0, P, P, P, P, P, P, None), b"sample_batch: null pointer"),    # no step counter
        ((1, P, 10, P, 5, P, P, 16, 0, 8, 4, None, P, P, P, P, P, None), b"sample_batch: augmented pairs missing"),
        ((1, P, 10, P, 5, P, P, 16, 0, 8, 4, P, None, P, P, P, P, None), b"sample_batch: augmented pairs missing"),
    ]
    for args, needle in batch:
        assert lib.llmrec_sample_batch(*args) != 0, args
        assert needle in lib.llmrec_last_error(), (args, lib.llmrec_last_error())


def test_users_without_train_items_never_reach_the_device_sampler(monkeypatch):
    """llmrec_sample_bpr draws the positive from the user's train row, so the list it samples from must hold users WITH train items only
    (include/llmrec_hip.h R11). Data builds the list that way; Data.checked_exist_users, which device_state goes through, refuses a list
    that does not."""
    import sys
    monkeypatch.setattr(sys, "argv", ["main.py", "--dataset", "netflix_valid_item"])
    sys.modules.pop("utility.load_data", None)
    import utility.load_data as LD
    D = LD.Data.__new__(LD.Data)
    D.train_items = {0: [3], 2: [1, 4]}
    D.exist_users = [0, 2]
    assert D.checked_exist_users() == [0, 2]
    for bad in ([0, 1, 2], [0, 2, 5]):
        D.exist_users = bad
        with pytest.raises(ValueError, match="no train items"):
            D.checked_exist_users()
    D.train_items[1] = []
    D.exist_users = [0, 1, 2]
    with pytest.raises(ValueError, match="no train items"):
        D.checked_exist_users()
