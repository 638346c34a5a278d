"""The bf16 pre-filter's proof under attack (llmrec_score_topk_mode_f32, LLMREC_TOPK_MODE_PREFILTER and the calls built on it).

The mode promises the exact sweep's lists and score bits. The promise rests on  ub = s' + slack ||u|| ||i|| >= s  for every pair; the
tables of tests/_prefilter_ref.py put an item of the true top K exactly where only that statement protects it (the "victim" row: 65th by
s', first by exact score, one residual away from the strong rows), with one- and two-sided residuals, at d = 64, 128 and 20, with negative
scores - and then multiply the user and item tables by powers of two, which changes no rounding of the scores (test_prefilter_ref_cpu.py)
but drives the norms and the slack term through fp32's underflow and overflow.

Every case is three-way: the prefilter mode's ids and score bits == the exact mode's == the numpy fma chain's ranking; under a factor 2^a
on the users and 2^b on the items the ids are those of the unscaled table and the score bits are the unscaled scores times 2^(a + b).
The victim user sits once inside a full 16-user tile and once alone in a ragged last tile. 32 - 33 queries x 600 items per call."""
import numpy as np
import pytest
import torch

from tests import _prefilter_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 50
QUERIES = {"full": P.Q_FULL, "tail": P.Q_TAIL}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


_REF = {}


def _ref(name, k, place):
    """(ids, scores) [n_query, k] of the unscaled table by the numpy chain and the rank rule: computed once, read-only."""
    key = (name, k, place)
    if key not in _REF:
        T = P.victim_table(name)
        ids, sc = P.exact_lists(T.chain[QUERIES[place]], k)
        ids.setflags(write=False); sc.setflags(write=False)
        _REF[key] = (ids, sc)
    return _REF[key]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _assert_lists(got, ref_i, ref_s, what):
    i, s = got
    i = i.cpu().numpy()
    if not (np.array_equal(i, ref_i) and np.array_equal(_bits(s), ref_s.view(np.int32))):
        rows = np.flatnonzero((i != ref_i).any(axis=1) | (_bits(s) != ref_s.view(np.int32)).any(axis=1))
        r = int(rows[0])
        miss = sorted(set(ref_i[r].tolist()) - set(i[r].tolist()))
        raise AssertionError("%s: %d query rows differ from the chain's ranking (first: row %d, reference items missing from it: %s)"
                             % (what, len(rows), r, miss[:5]))


def _three_way(ops, eu, ei, q, k, ref_i, ref_s, what):
    """both modes against the reference; returns the prefilter call's statistics"""
    Eu, Ei = torch.from_numpy(eu).to(DEV), torch.from_numpy(ei).to(DEV)
    qd = torch.tensor(q, device=DEV)
    stats = {}
    exact = ops.score_topk(Eu, Ei, qd, None, k, mode="exact")
    pre = ops.score_topk(Eu, Ei, qd, None, k, mode="prefilter", stats=stats)
    torch.cuda.synchronize()
    print(what, stats)
    _assert_lists(exact, ref_i, ref_s, what + ", exact mode")
    _assert_lists(pre, ref_i, ref_s, what + ", prefilter mode")
    return stats


@pytest.mark.parametrize("place", ["full", "tail"])
@pytest.mark.parametrize("scale", P.SCALES, ids=lambda s: "u%+d_i%+d" % s)
@pytest.mark.parametrize("name", P.TABLES)
def test_lists_and_score_bits_are_the_chains_at_every_scale(ops, name, scale, place):
    a, b = scale
    T = P.victim_table(name)
    eu, ei, _ = T.scaled(a, b)
    ref_i, ref_s = _ref(name, K, place)
    assert ref_i[QUERIES[place].index(5 if place == "full" else 33), 0] == P.VICTIM_ITEM
    stats = _three_way(ops, eu, ei, QUERIES[place], K, ref_i, np.ldexp(ref_s, a + b).astype(np.float32), "%s %s %s" % (name, scale, place))
    # Inside the magnitude window the victim user's proof must FAIL (65 rows within the slack of the boundary) and every benign user's
    # holds, with a margin of the whole slack (test_prefilter_ref_cpu.py): one tile goes to the exact sweep. Outside it no proof is trusted.
    assert stats["fallback_tiles"] == (1 if scale in P.IN_WINDOW else stats["tiles"]), stats


@pytest.mark.parametrize("place", ["full", "tail"])
@pytest.mark.parametrize("scale", [(0, 0), (0, -76), (-76, 0)], ids=lambda s: "u%+d_i%+d" % s)
@pytest.mark.parametrize("k", [1, 56])
def test_the_smallest_and_the_largest_verified_cut_off(ops, k, scale, place):
    """K = 1: 63 spare slots; K = 56 (LLMREC_TOPK_PREFILTER_MAX_K): 8."""
    a, b = scale
    T = P.victim_table("two64")
    eu, ei, _ = T.scaled(a, b)
    ref_i, ref_s = _ref("two64", k, place)
    _three_way(ops, eu, ei, QUERIES[place], k, ref_i, np.ldexp(ref_s, a + b).astype(np.float32), "two64 K=%d %s %s" % (k, scale, place))


@pytest.mark.parametrize("place", ["full", "tail"])
@pytest.mark.parametrize("name", ["one64", "two128", "two20"])
def test_norms_that_overflow_beside_an_all_zero_user(ops, name, place):
    """Item table x 2^62: every squared item norm is +inf in fp32. One all-zero user row: 0 x inf, a NaN bound for every item - once inside a
    full tile, once as the only row of the last tile, where no neighbour's failed proof sends its tile to the exact sweep. Its scores are
    all +0.0: the list is items 0 .. K - 1."""
    T = P.victim_table(name)
    eu, ei, S = T.scaled(0, 62)
    eu = np.concatenate([eu, np.zeros((1, T.d), np.float32)])
    zero = eu.shape[0] - 1
    q = list(QUERIES[place])
    q[7 if place == "full" else len(q) - 1] = zero
    Sq = np.concatenate([S, np.zeros((1, P.N_ITEMS), np.float32)])[q]
    ref_i, ref_s = P.exact_lists(Sq, K)
    assert ref_i[q.index(zero)].tolist() == list(range(K)) and not ref_s[q.index(zero)].view(np.int32).any()
    _three_way(ops, eu, ei, q, K, ref_i, ref_s, "%s x 2^62 with a zero user, %s" % (name, place))


@pytest.mark.parametrize("place", ["full", "tail"])
@pytest.mark.parametrize("scale", [(0, 0), (0, -76)], ids=lambda s: "u%+d_i%+d" % s)
@pytest.mark.parametrize("name", ["one64", "two64"])
def test_the_serving_calls_run_the_same_sweeps(ops, name, scale, place):
    """K = 100: two passes of the single-sweep call (56 + 44 ranks in the prefilter mode), the victim row in the first. An allow-list that
    keeps the strong, filler and victim rows and every third low row: the compact table's sweep, ids mapped back."""
    a, b = scale
    T = P.victim_table(name)
    eu, ei, _ = T.scaled(a, b)
    q = QUERIES[place]
    Eu, Ei, qd = torch.from_numpy(eu).to(DEV), torch.from_numpy(ei).to(DEV), torch.tensor(q, device=DEV)
    ref_i, ref_s = _ref(name, 100, place)
    ref_s = np.ldexp(ref_s, a + b).astype(np.float32)
    for mode in ("exact", "prefilter"):
        _assert_lists(ops.score_topk(Eu, Ei, qd, None, 100, mode=mode), ref_i, ref_s, "%s %s %s K=100 %s" % (name, scale, place, mode))
    allow = T.kind != 3
    allow[T.ids(3)[::3]] = True
    dropped = np.flatnonzero(~allow)
    key = (name, "filtered", place)
    if key not in _REF:
        _REF[key] = P.exact_lists(T.chain[q], K, [dropped] * len(q))
    f_i, f_s = _REF[key]
    assert (f_i[q.index(5 if place == "full" else 33), 0] == P.VICTIM_ITEM) and not np.isin(f_i, dropped).any()
    filt = ops.ItemFilter(torch.from_numpy(allow).to(DEV))
    for mode in ("exact", "prefilter"):
        _assert_lists(ops.score_topk_filtered(Eu, Ei, qd, None, K, filt, mode=mode), f_i, np.ldexp(f_s, a + b).astype(np.float32),
                      "%s %s %s filtered %s" % (name, scale, place, mode))
