"""The reference the evaluation kernels are held to (tests/_eval_ref.py), checked on the host: the chain's zero padding, its distance from
the fp64 product, the ranking rule against the oracle's heapq form, and the NaN-surrounded table layouts."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests._eval_ref import GUARD, chain_scores, layouts, rank

RAGGED = [1, 3, 4, 15, 17, 20, 31, 33, 50, 65, 100, 127]


@pytest.mark.parametrize("d", RAGGED)
def test_chain_at_a_ragged_width_is_the_chain_of_the_zero_padded_rows_and_close_to_fp64(d):
    """The kernels pad d to whole 16-column chunks with zeros (fragments, LDS copies, packed tables): fma(0, 0, acc) = acc, so the padded chain
    is the ragged one bit for bit. And the chain is an fp32 summation of d exact products: |chain - exact| <= d 2^-24 (|eu| . |ei|)."""
    rng = np.random.default_rng(d)
    eu = (rng.standard_normal((48, d)) * 0.4).astype(np.float32)
    ei = (rng.standard_normal((700, d)) * 0.4).astype(np.float32)
    S = chain_scores(eu, ei)
    assert S.dtype == np.float32 and S.shape == (48, 700)
    dp = 16 * ((d + 15) // 16)
    eu_p, ei_p = np.zeros((48, dp), np.float32), np.zeros((700, dp), np.float32)
    eu_p[:, :d], ei_p[:, :d] = eu, ei
    assert np.array_equal(S.view(np.int32), chain_scores(eu_p, ei_p).view(np.int32))
    exact = eu.astype(np.float64) @ ei.astype(np.float64).T
    bound = d * 2.0 ** -24 * (np.abs(eu).astype(np.float64) @ np.abs(ei).astype(np.float64).T)
    assert (np.abs(S.astype(np.float64) - exact) <= bound).all()


def test_chain_visits_k_in_the_order_of_the_mfma():
    """One user, one item, values that make the order visible: 2^24 + 1 - 2^24 is 0 or 1 in fp32 depending on which product comes first."""
    eu = np.zeros((1, 32), np.float32)
    ei = np.ones((1, 32), np.float32)
    eu[0, 0], eu[0, 1], eu[0, 4] = 2.0 ** 24, 1.0, -2.0 ** 24          # chain order: k = 0, 4, 8, 12, 1, ...: the large terms cancel first
    assert chain_scores(eu, ei)[0, 0] == 1.0
    assert O.scores_fma_chain(eu, ei, order="natural")[0, 0] == 0.0


def test_rank_restates_the_oracles_heapq_rule_on_tie_heavy_tables():
    rng = np.random.default_rng(7)
    I, K = 300, 20
    eu = rng.integers(-2, 3, (12, 8)).astype(np.float32)
    ei = rng.integers(-1, 2, (I, 8)).astype(np.float32)
    S = chain_scores(eu, ei)
    assert len(np.unique(S[0])) < 40                                       # ties everywhere
    trains = [[], list(range(0, I, 2)), sorted(rng.choice(I, I - 13, replace=False).tolist()), list(range(I))] + \
             [sorted(rng.choice(I, int(rng.integers(0, 40)), replace=False).tolist()) for _ in range(8)]
    for u, tr in enumerate(trains):
        want = O.rank_topk(S[u], tr, K)
        ids, sc = rank(S[u], tr, K)
        n = len(want)
        assert n == min(K, I - len(tr))
        assert ids.dtype == np.int32 and sc.dtype == np.float32 and ids.shape == sc.shape == (K,)
        assert ids[:n].tolist() == want
        assert np.array_equal(sc[:n], S[u][want])
        assert (ids[n:] == -1).all() and np.isneginf(sc[n:]).all()
        assert not set(ids[:n].tolist()) & set(tr)
        pairs = [(-float(s), int(i)) for s, i in zip(sc[:n], ids[:n])]
        assert pairs == sorted(pairs)
    assert (rank(S[3], trains[3], K)[0] == -1).all()                       # every item in train
    assert rank(S[0], [], 1)[0][0] == int(np.flatnonzero(S[0] == S[0].max())[0])


@pytest.mark.parametrize("d", [1, 3, 4, 15, 16, 17, 50, 64, 127, 128])
def test_layouts_hold_the_values_inside_a_nan_surround(d):
    rng = np.random.default_rng(d)
    src = rng.standard_normal((9, d)).astype(np.float32)
    built = {name: make(src, device="cpu") for name, make in layouts(d).items()}
    assert sorted(built) == ["contig", "odd_ld", "padded", "shifted"]
    for name, tb in built.items():
        assert tb.t.shape == (9, d) and tb.t.stride() == (tb.ld, 1) and tb.ld >= d
        assert torch.equal(tb.t, torch.from_numpy(src))
        flat = tb.buf.numpy()
        assert np.isnan(flat[:GUARD + tb.col0]).all() and np.isnan(flat[-GUARD:]).all()
        assert int(np.isfinite(flat).sum()) == 9 * d
        if tb.ld > d:                                                      # the gap between two rows
            row1 = GUARD + tb.col0 + tb.ld
            assert np.isnan(flat[row1 - (tb.ld - d):row1]).all()
        tb.check()
    assert built["contig"].ld == d and built["contig"].col0 == 0
    assert built["padded"].ld % 4 == 0 and built["padded"].ld >= d + 4 and built["padded"].col0 == 0
    assert built["odd_ld"].ld % 4 != 0 and built["odd_ld"].ld in (d + 1, d + 2) and (built["odd_ld"].ld == d + 1 or (d + 1) % 4 == 0)
    assert built["shifted"].ld % 4 == 0 and built["shifted"].col0 == 1 and built["shifted"].base_mod16 == 4


def test_table_check_notices_a_write_outside_the_view_and_a_changed_value():
    src = np.arange(12, dtype=np.float32).reshape(3, 4)
    tb = layouts(4)["padded"](src, device="cpu")
    tb.buf[GUARD + 5] = 0.0                                                # the gap behind row 0
    with pytest.raises(AssertionError):
        tb.check()
    tb = layouts(4)["shifted"](src, device="cpu")
    tb.t[2, 3] += 1.0
    with pytest.raises(AssertionError):
        tb.check()
