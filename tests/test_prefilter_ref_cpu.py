"""The numpy restatement of the bf16 pre-filter (tests/_prefilter_ref.py) and its adversarial tables, checked on the host:
the split, the tables' claim that s' is exact in any order, the bound ub >= s pair by pair, how close the tables come to it (the reach),
which wrong slack constants the tables catch and which they cannot, the chain's invariance under the power-of-two factors the GPU tests
sweep, and the magnitude guard (what the arithmetic did without it at 2^-76, and that with it no scale returns a wrong list as proven)."""
import numpy as np
import pytest
import torch

from tests import _prefilter_ref as P
from tests._eval_ref import chain_scores

K = 50
VU = list(P.VICTIM_USERS)


def _exact(T, k=K):
    return P.exact_lists(T.chain[VU], k)


def test_split_is_round_to_nearest_even_twice_and_drops_at_most_2_to_the_minus_16():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(3.0),
                        np.ldexp(rng.standard_normal(2000), rng.integers(-100, 100, 2000)).astype(np.float32),
                        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 2.0 ** -8), 0.0, 1 + P.MID + P.RES], np.float32)])
    h, m = P.split(x)
    assert np.array_equal(h, torch.from_numpy(x).to(torch.bfloat16).float().numpy())            # ties to even included
    assert np.array_equal(m, torch.from_numpy(x - h).to(torch.bfloat16).float().numpy())
    assert not (h.view(np.uint32) & 0xFFFF).any() and not (m.view(np.uint32) & 0xFFFF).any()
    r = x.astype(np.float64) - h - m
    assert (np.abs(r) <= 2.0 ** -16 * np.abs(x)).all()
    assert h[-6] == 1.0 and h[-5] == np.float32(1 + 2.0 ** -6) and h[-4] == np.float32(1 + 2.0 ** -7)   # 1 + 2^-8 is a tie: to the even neighbour
    assert h[-1] == 1.0 and m[-1] == np.float32(P.MID) and r[-1] == P.RES


def _low_bit_exponent(t):
    """exponent of the lowest set bit of each non-zero float64"""
    m, e = np.frexp(t)
    mant = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = mant & -mant
    return e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)


@pytest.mark.parametrize("name", P.TABLES)
def test_every_partial_sum_of_s_prime_is_exact_in_fp32(name):
    """All 3 d products of a pair are multiples of q = 2^e and sum |product| <= 2^24 q: every sum of any subset, in any order and in any
    format at least as wide as fp32, is exact. So the MFMA's undocumented accumulation order cannot change s' - for the victim user against
    every strong, filler and victim row; a low row need not be exact, its |s'| in any order stays 8 below the fillers'."""
    T = P.victim_table(name)
    hu, mu = (a.astype(np.float64) for a in P.split(T.eu[VU]))                                  # (the victim user's rows: the benign users' lists
    hi, mi = (a.astype(np.float64) for a in P.split(T.ei))                                      #  are far from any boundary)
    terms = np.concatenate([hu[:, None, :] * hi[None, :, :], hu[:, None, :] * mi[None, :, :], mu[:, None, :] * hi[None, :, :]], axis=2)
    e = np.where(terms != 0, _low_bit_exponent(np.where(terms != 0, terms, 1.0)), 1000).min(axis=2)
    mass = np.abs(terms).sum(axis=2)
    with np.errstate(over="ignore"):
        exact = mass <= np.ldexp(1.0, 24 + e)
    sp = P.sprime(T.eu[VU], T.ei)
    top = T.kind != 3
    assert exact[:, top].all() and top.sum() == P.N_STRONG + P.N_FILLER + 1
    assert np.array_equal(sp[:, top].astype(np.float64), terms.sum(axis=2)[:, top])             # (and the fp32 rounding changed nothing)
    assert (exact | (mass * (1 + 2.0 ** -10) < sp[:, T.ids(1)].min() - 8))[:, ~top].all()


@pytest.mark.parametrize("name", P.TABLES)
def test_the_tables_are_built_as_described(name):
    T = P.victim_table(name)
    S = T.chain
    for u in VU:
        ev, es, ef = S[u, P.VICTIM_ITEM], S[u, T.ids(0)], S[u, T.ids(1)]
        assert len(es) == P.N_STRONG and len(ef) == P.N_FILLER and (es == es[0]).all() and (ef == ef[0]).all()
        assert ev > es[0] > ef[0] > S[u, T.ids(3)].max() + 8                                     # the true top 50: the victim and 49 strong rows
        sp = P.sprime(T.eu[u:u + 1], T.ei)[0]
        assert sp[P.VICTIM_ITEM] < sp[T.ids(1)].min() <= sp[T.ids(1)].max() < sp[T.ids(0)].min()   # ... and by s' the victim is 65th
    ids, _ = _exact(T)
    assert (ids[:, 0] == P.VICTIM_ITEM).all() and set(ids[0, 1:]) == set(T.ids(0)[:K - 1])
    assert T.eu.shape == (P.N_USERS, T.d) and T.ei.shape == (P.N_ITEMS, T.d) and P.N_ITEMS % 32 != 0
    assert P.Q_FULL.index(5) < 16 and len(P.Q_FULL) == 32 and len(P.Q_TAIL) == 33 and P.Q_TAIL[-1] == 33 and 5 not in P.Q_TAIL


@pytest.mark.parametrize("name", P.TABLES)
def test_the_bound_holds_for_every_pair_at_scale_one(name):
    """(a): ub >= the chain score, with the fp32 ub of the kernels and with s' + slack ||u|| ||i|| in float64 (true norms, no up-rounding)."""
    T = P.victim_table(name)
    ub, sp, ok = P.bounds(T.eu, T.ei)
    assert ok.all() and np.isfinite(ub).all()
    assert (ub >= T.chain).all()
    nu = np.sqrt((T.eu.astype(np.float64) ** 2).sum(1))
    ni = np.sqrt((T.ei.astype(np.float64) ** 2).sum(1))
    ub64 = sp.astype(np.float64) + float(P.pre_slack(T.d)) * nu[:, None] * ni[None, :]
    assert (ub64 >= T.chain.astype(np.float64)).all()


# (b) the reach (s - s') / (||u|| ||i||) in units of 2^-16, against the 3.02 the slack provides for (plus the accumulation term).
# One-sided tables miss <u_h, i_r> only: 0.9 x 2^-17 per element of about 1.002 -> 0.45. Two-sided tables miss <u_m, i_m> (0.98),
# <u_r, i> and <u_h, i_r> (0.45 each) per element of 1.016 -> about 1.9. (3.02 needs |r| = 2^-16 |x| and |m| = 2^-8 |x| at once in both
# operands; with round-to-nearest splits |r| <= 2^-17 |x| wherever |m| is near 2^-8 |x|.)
REACH_MIN = {"one64": 0.45, "neg64": 0.45, "one128": 0.45, "one20": 0.45, "two64": 1.5, "two128": 1.5, "two20": 1.5}


@pytest.mark.parametrize("name", P.TABLES)
def test_reach_of_the_tables(name):
    T = P.victim_table(name)
    r = P.reach(T.eu, T.ei, T.chain)
    print("reach %s: %.3f x 2^-16" % (name, r))
    assert REACH_MIN[name] <= r < 3.02 + 3 * T.d * 2.0 ** -8


# (c) the largest slack 2^e that each table KILLS: the restatement returns a wrong list with the proof holding. Larger mutants SURVIVE on
# that table: the proof fails, the exact sweep runs, the list is right. One-sided tables (reach 0.45) need the mutant's slack on the
# fillers, about d x 2^e, to fit under the 9 / 64 d x 2^-16 between the fillers' and the strong rows' s'; two-sided tables kill everything
# up to 2^-16 (< 1.56 x 2^-16). No table can kill 2^-15 or, at d = 128, the historic 2^-14: the reach of any input is below 2 x 2^-16
# unless the MFMA's accumulation error lines up, which no input can force.
KILLS = {"one64": -19, "neg64": -19, "one128": -19, "one20": -19, "two64": -16, "two128": -16, "two20": -16}
MUTANTS = list(range(-13, -21, -1))


@pytest.mark.parametrize("name", P.TABLES)
def test_slack_mutants_die_or_survive_as_recorded(name):
    T = P.victim_table(name)
    ex_i, ex_s = _exact(T)
    for e in MUTANTS:
        ids, sc, held = P.prefilter_lists(T.eu[VU], T.ei, K, slack=2.0 ** e, chain=T.chain[VU])
        wrong = (ids != ex_i).any(axis=1)
        if e <= KILLS[name]:
            assert (held & wrong).all(), (name, e, held, wrong)
        else:
            assert not held.any(), (name, e, held)                   # the proof fails: the exact sweep decides
    ids, sc, held = P.prefilter_lists(T.eu, T.ei, K, chain=T.chain)   # the real slack, every user: right or not proven
    all_i, all_s = P.exact_lists(T.chain, K)
    right = (ids == all_i).all(axis=1) & (sc.view(np.int32) == all_s.view(np.int32)).all(axis=1)
    assert (right | ~held).all() and not held[VU].any()
    # the benign users are proven, and still are with twice the slack: whatever the MFMA's accumulation adds to s' is inside the slack,
    # so on the GPU exactly the victim user's tile goes to the exact sweep (test_gpu_topk_bound.py counts the tiles)
    benign = np.setdiff1d(np.arange(P.N_USERS), VU)
    assert held[benign].all()
    assert P.prefilter_lists(T.eu[benign], T.ei, K, slack=2 * float(P.pre_slack(T.d)), chain=T.chain[benign])[2].all()


def test_every_width_has_a_table_that_kills_2_to_the_minus_16():
    for d in (64, 128, 20):
        assert any(P.victim_table(n).d == d and KILLS[n] >= -16 for n in P.TABLES)
    assert float(P.pre_slack(64)) == 2.0 ** -14 and float(P.pre_slack(65)) == 2.0 ** -13 and float(P.pre_slack(128)) == 2.0 ** -13


# (d) power-of-two factors change no rounding while nothing under- or overflows
def test_the_sweep_is_the_nine_pairs():
    assert sorted(P.SCALES) == sorted([(0, 0), (0, -40), (0, -70), (0, -76), (0, -100), (-76, 0), (-60, -60), (40, 0), (0, 62)])


@pytest.mark.parametrize("name", P.TABLES)
def test_the_chain_commutes_with_every_factor_of_the_sweep(name):
    T = P.victim_table(name)
    for a, b in P.SCALES:
        eu, ei, S = T.scaled(a, b)
        assert np.array_equal(np.ldexp(eu.astype(np.float64), -a), T.eu) and np.array_equal(np.ldexp(ei.astype(np.float64), -b), T.ei)
        got = chain_scores(eu, ei)
        assert np.array_equal(got.view(np.int32), S.view(np.int32)), (name, a, b)
        top = np.sort(S[VU], axis=1)[:, -120:]
        assert np.isfinite(S).all() and (np.abs(top) >= 2.0 ** -126).all(), (name, a, b)       # the victim user's lists: ordinary normal floats


# ---- the magnitude guard ----
@pytest.mark.parametrize("name", P.TABLES)
def test_without_the_guard_a_norm_that_underflows_proves_a_wrong_list(name):
    """What the arithmetic did before the guard: below 2^-75 every square is zero in fp32, the norm is 0, the slack term vanishes and the
    victim row's residual is no longer covered - while the scores themselves are ordinary normal floats."""
    T = P.victim_table(name)
    ex_i, _ = _exact(T)
    for a, b in [(0, -76), (0, -100), (-76, 0)]:
        eu, ei, S = T.scaled(a, b)
        ids, sc, held = P.prefilter_lists(eu[VU], ei, K, guard=False, chain=S[VU])
        assert held.all() and (ids != ex_i).any(axis=1).all(), (name, a, b)


@pytest.mark.parametrize("name", P.TABLES)
def test_with_the_guard_no_factor_of_the_sweep_proves_a_wrong_list(name):
    T = P.victim_table(name)
    ex_i, ex_s = P.exact_lists(T.chain, K)
    for a, b in P.SCALES:
        eu, ei, S = T.scaled(a, b)
        ids, sc, held = P.prefilter_lists(eu, ei, K, chain=S)
        right = (ids == ex_i).all(axis=1) & (sc.view(np.int32) == np.ldexp(ex_s, a + b).astype(np.float32).view(np.int32)).all(axis=1)
        assert (right | ~held).all(), (name, a, b)
        ss_u, ss_i = P.user_sumsq(eu), P.item_sumsq(ei)
        inside = (ss_u[0] >= P.SS_MIN) & (ss_u[0] <= P.SS_MAX) & (ss_i[P.VICTIM_ITEM] >= P.SS_MIN) & (ss_i[P.VICTIM_ITEM] <= P.SS_MAX)
        assert inside == ((a, b) in P.IN_WINDOW), (name, a, b)
        benign = np.setdiff1d(np.arange(P.N_USERS), VU)
        assert not held[VU].any() and held[benign].all() == inside and held[benign].any() == inside, (name, a, b)   # inside: the mode runs as itself


def test_sums_of_squares_follow_the_kernels_and_only_a_zero_row_sums_to_zero():
    rng = np.random.default_rng(5)
    for d in (20, 48, 64, 72, 96, 100, 128):
        x = (rng.standard_normal((40, d)) * 0.4).astype(np.float32)
        x[3] = 0.0
        x[4] = np.float32(2.0 ** -80)                   # every square underflows
        x[5, :] = 0.0; x[5, d - 1] = np.float32(2.0 ** -100)
        ref = (x.astype(np.float64) ** 2).sum(1)
        for got in (P.item_sumsq(x), P.item_sumsq(x, guard=False), P.user_sumsq(x)):
            assert np.allclose(got[6:], ref[6:], rtol=d * 2.0 ** -24, atol=0) and got[3] == 0
        g = P.item_sumsq(x)
        assert 0 < g[4] < P.SS_MIN and 0 < g[5] < P.SS_MIN
        assert P.item_sumsq(x, guard=False)[4] == 0 and P.user_sumsq(x)[4] == 0
        ub, _, ok = P.bounds(x, x)
        assert np.isinf(ub[6:, 4]).all() and np.isinf(ub[6:, 5]).all() and np.isfinite(ub[6:, 3]).all() and np.isfinite(ub[6:, 6:]).all()
        assert ok[6:].all() and not ok[3] and not ok[4] and not ok[5]


def test_the_restatement_agrees_with_the_exact_ranking_on_a_random_table_with_train_rows():
    rng = np.random.default_rng(9)
    eu = (rng.standard_normal((12, 48)) * 0.4).astype(np.float32)
    ei = (rng.standard_normal((400, 48)) * 0.4).astype(np.float32)
    train = [sorted(rng.choice(400, int(n), replace=False).tolist()) for n in rng.integers(0, 30, 12)]
    train[2] = sorted(rng.choice(400, 360, replace=False).tolist())                              # fewer than K candidates
    S = chain_scores(eu, ei)
    ids, sc, held = P.prefilter_lists(eu, ei, K, train=train, chain=S)
    ex_i, ex_s = P.exact_lists(S, K, train)
    assert held.all() and np.array_equal(ids, ex_i) and np.array_equal(sc.view(np.int32), ex_s.view(np.int32))
    assert (ids[2, 40:] == -1).all() and np.isneginf(sc[2, 40:]).all()
