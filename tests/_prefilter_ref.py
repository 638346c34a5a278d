"""The bf16 pre-filter of llmrec_score_topk_mode_f32 (csrc/topk.hip, LLMREC_TOPK_MODE_PREFILTER) restated in numpy, and tables that attack
the one analytic statement its proof rests on:  ub = s' + slack ||u|| ||i||  is an upper bound of the exact score, item by item.
Nothing here imports llmrec_amd.

split            x -> (h, m): the round-to-nearest bf16 parts, by the bit formula of rn_bf16_bits_finite (r = x - h - m is what the sweep drops)
sprime           s' = <u_h, i_h> + <u_h, i_m> + <u_m, i_h>, summed in float64 and rounded once to fp32. The MFMA's own accumulation order is
                 not documented: the adversarial tables below keep every partial sum of s' exactly representable, so any order gives this value
item_sumsq / user_sumsq   the squared norms as the kernels form them: fp32 fma chains per thread, then a fixed butterfly of fp32 additions
bounds           ub [n_users, n_items] fp32 = fma(||u|| up, slack ||i|| up, s'), with the magnitude guard of the finished code (or without it)
prefilter_lists  the 64 largest ub (ties by item id), the exact re-rank of those 64 by the fma chain and the rank rule of tests/_eval_ref.py,
                 the proof ub_64 < e_K, and a flag per user saying whether the proof held (a user whose flag is False goes to the exact sweep)
victim_table     the adversarial tables; TABLES names the seven the suite uses
reach            max over pairs of (s - s') / (||u|| ||i||) in units of 2^-16

fp32 fma(a, b, c) is computed as float32(float64(a) * float64(b) + float64(c)), the form oracle.scores_fma_chain uses: the product is exact in
float64, the sum is rounded twice (a double rounding can differ from the fused result in the last bit about once in 2^29 sums; the norms and
bounds carry 2^-10 of head room, and the tables' chain scores are checked against exact rational values where a test depends on them)."""
import numpy as np

from tests._eval_ref import chain_scores, rank

F32 = np.float32
KEEP = 64                                   # slots of a user's list
NORM_UP = F32(1.0) + F32(2.0 ** -10)        # TK_NORM_UP
SS_MIN, SS_MAX = F32(2.0 ** -88), F32(2.0 ** 88)     # TK_SS_MIN / TK_SS_MAX: squared norms the bound's arithmetic is trusted for
ELEM_MAX = F32(2.0 ** 44)                   # TK_ELEM_MAX: an item element beyond it is packed as zero (its row is outside the window anyway)
FLT_MIN = F32(2.0 ** -126)

# the power-of-two factors (a on the user table, b on the item table) the GPU tests sweep; the chain commutes with every one of them
SCALES = [(0, 0), (0, -40), (0, -70), (0, -76), (0, -100), (-76, 0), (-60, -60), (40, 0), (0, 62)]


def pre_slack(d):
    """tk_pre_slack"""
    return F32(2.0 ** -14) if d <= 64 else F32(2.0 ** -13)


def _rn_bf16(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    hb = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return hb.view(F32)


def split(x):
    """(h, m) float32: h = RN_bf16(x), m = RN_bf16(x - h); x - h is exact in fp32."""
    x = np.ascontiguousarray(x, dtype=F32)
    h = _rn_bf16(x)
    m = _rn_bf16(x - h)
    return h, m


def _fma(a, b, c):
    with np.errstate(all="ignore"):         # (overflow to inf and underflow to zero are part of what is restated)
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _pad(x, cols):
    out = np.zeros((x.shape[0], cols), dtype=F32)
    out[:, :x.shape[1]] = x
    return out


def _butterfly(p):
    """p [n, W] fp32, W a power of two: v += shfl_xor(v, off) for off = W / 2 .. 1; every lane ends with the same sum."""
    W = p.shape[1]
    lane = np.arange(W)
    off = W // 2
    while off > 0:
        with np.errstate(all="ignore"):
            p = (p + p[:, lane ^ off]).astype(F32)
        off //= 2
    return p[:, 0]


def _sq_step(x, ss, guard):
    ss = _fma(x, x, ss)
    if guard:                               # a square that underflows still counts: only an all-zero row has a zero sum
        ss = np.maximum(ss, np.where(x != 0, FLT_MIN, F32(0)))
    return ss


def item_sumsq(ei, guard=True):
    """topk_pack_items_bf16_kernel (thread g of an item: k = 8 g .. 8 g + 7 in order, then a butterfly over the item's G threads) and, for
    d in (64, 96] (G = 12), topk_item_norm_kernel (lane gl: k = gl, gl + 16, ..., then a butterfly over 16 lanes)."""
    ei = np.ascontiguousarray(ei, dtype=F32)
    n, d = ei.shape
    G = (d + 31) // 32 * 4
    if G & (G - 1):
        x = _pad(ei, (d + 15) // 16 * 16).reshape(n, -1, 16)            # [n, step, lane]
        p = np.zeros((n, 16), dtype=F32)
        for t in range(x.shape[1]):
            p = _sq_step(x[:, t, :], p, guard)
        return _butterfly(p)
    x = _pad(ei, 8 * G).reshape(n, G, 8)
    p = np.zeros((n, G), dtype=F32)
    for j in range(8):
        p = _sq_step(x[:, :, j], p, guard)
    return _butterfly(p)


def user_sumsq(eu):
    """score_topk_pre_kernel: lane group lq of a row takes k = 32 c + 8 lq + j (for c, for j), then + xor 16, + xor 32."""
    eu = np.ascontiguousarray(eu, dtype=F32)
    n, d = eu.shape
    x = _pad(eu, (d + 31) // 32 * 32).reshape(n, -1, 4, 8)              # [n, c, lq, j]
    p = np.zeros((n, 4), dtype=F32)
    for c in range(x.shape[1]):
        for j in range(8):
            p = _fma(x[:, c, :, j], x[:, c, :, j], p)
    lane = np.arange(4)
    p = (p + p[:, lane ^ 1]).astype(F32)
    p = (p + p[:, lane ^ 2]).astype(F32)
    return p[:, 0]


def sprime(eu, ei, guard=True):
    hu, mu = split(eu)
    x = np.ascontiguousarray(ei, dtype=F32)
    if guard:
        x = np.where(np.abs(x) <= ELEM_MAX, x, F32(0))
    hi, mi = split(x)
    hu, mu, hi, mi = (a.astype(np.float64) for a in (hu, mu, hi, mi))
    with np.errstate(all="ignore"):
        return (hu @ hi.T + hu @ mi.T + mu @ hi.T).astype(F32)


def bounds(eu, ei, slack=None, guard=True):
    """(ub fp32 [n_users, n_items], s' fp32, user_ok bool [n_users]). guard: the finished code - an item whose squared norm is neither zero
    nor inside [SS_MIN, SS_MAX] has an infinite bound, a user whose squared norm is outside it is not trusted (its tile goes to the exact
    sweep). guard=False: the arithmetic before that, where a norm that underflows is a zero slack."""
    d = eu.shape[1]
    slack = pre_slack(d) if slack is None else F32(slack)
    with np.errstate(all="ignore"):
        ss_i, ss_u = item_sumsq(ei, guard), user_sumsq(eu)
        cn = (slack * (np.sqrt(ss_i) * NORM_UP).astype(F32)).astype(F32)
        un = (np.sqrt(ss_u) * NORM_UP).astype(F32)
        user_ok = np.ones(eu.shape[0], dtype=bool)
        if guard:
            cn = np.where((ss_i == 0) | ((ss_i >= SS_MIN) & (ss_i <= SS_MAX)), cn, F32(np.inf))
            user_ok = (ss_u >= SS_MIN) & (ss_u <= SS_MAX)
        sp = sprime(eu, ei, guard)
        ub = _fma(un[:, None], cn[None, :], sp)
    return ub, sp, user_ok


def prefilter_lists(eu, ei, K, train=None, slack=None, guard=True, chain=None):
    """The mode before its fallback: (ids int32 [n, K], scores fp32 [n, K], held bool [n]). eu: the QUERIED user rows. train: per-user id lists
    or None. chain: chain_scores(eu, ei) when the caller has it already."""
    eu, ei = np.ascontiguousarray(eu, dtype=F32), np.ascontiguousarray(ei, dtype=F32)
    n, n_items = eu.shape[0], ei.shape[0]
    ub, _, user_ok = bounds(eu, ei, slack, guard)
    S = chain_scores(eu, ei) if chain is None else chain
    ids = np.full((n, K), -1, dtype=np.int32)
    sc = np.full((n, K), -np.inf, dtype=F32)
    held = np.zeros(n, dtype=bool)
    for u in range(n):
        free = np.ones(n_items, dtype=bool)
        if train is not None:
            free[np.asarray(train[u], dtype=np.int64)] = False
        cand = [i for i in np.flatnonzero(free).tolist() if not np.isnan(ub[u, i])]           # (a NaN bound passes no filter)
        kept = sorted(cand, key=lambda i: (-float(ub[u, i]), i))[:KEEP]
        ub64 = float(ub[u, kept[-1]]) if len(kept) == KEEP else -np.inf
        outside = np.ones(n_items, dtype=bool)
        outside[kept] = False
        ids[u], sc[u] = rank(S[u], np.flatnonzero(outside), K)
        eK = float(sc[u, K - 1])
        held[u] = bool(user_ok[u]) and (ub64 == -np.inf or ub64 < eK)
    return ids, sc, held


def exact_lists(S, K, train=None):
    n = S.shape[0]
    out = [rank(S[u], [] if train is None else train[u], K) for u in range(n)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def reach(eu, ei, chain=None):
    """max over pairs of (s - s') / (||u|| ||i||) in units of 2^-16: s the chain score, s' in float64 (unrounded), norms in float64."""
    hu, mu = split(eu)
    hi, mi = split(ei)
    hu, mu, hi, mi = (a.astype(np.float64) for a in (hu, mu, hi, mi))
    sp = hu @ hi.T + hu @ mi.T + mu @ hi.T
    S = (chain_scores(eu, ei) if chain is None else chain).astype(np.float64)
    nu = np.sqrt((eu.astype(np.float64) ** 2).sum(1))
    ni = np.sqrt((ei.astype(np.float64) ** 2).sum(1))
    with np.errstate(all="ignore"):
        g = (S - sp) / (nu[:, None] * ni[None, :])
    return float(np.nanmax(g)) * 2.0 ** 16


# ---------------------------------------------------------------------------------------------------------------------------------------
# The adversarial tables. One "victim" user and, among ~600 items, K = 50 "strong" rows, 14 "fillers", one "victim" row and low-score rows:
#   one-sided  user element 1 (bf16-exact); item base b = 1 + 2^-9 (= h + m exactly). strong = b with d / 4 elements raised by g = 2^-16,
#              filler = b with d / 9 elements raised, victim = b + 0.9 x 2^-17 everywhere: its residual r > 0 is invisible to s', so
#              s'(victim) = d b < s'(filler) < s'(strong) = e(strong) < e(victim) = d b + 0.45 d g.
#   two-sided  user element 1 + (2^-8 - 2^-15) + 0.9 x 2^-17 (h = 1, the largest mid part that keeps h, a positive residual); item base
#              b2 = 1 + (2^-8 - 2^-15): now <u_m, i_m> (0.98 g per element) and <u_r, i> (0.45 g) are missing from EVERY row's s', and the
#              victim row misses <u_h, i_r> (0.45 g) on top: 1.9 g per element against ||u|| ||i|| of 1.016 per element.
#   negative   one-sided with the item rows' signs flipped (base -(1 + 1.5 x 2^-9), strong and filler raised by +g, victim base + 0.9 x 2^-17:
#              the residual still points towards the higher score; with -(1 + 2^-9) the mid part would sit at the top of its binade and the
#              finer grid below it would absorb the residual), and low rows of -1.25 .. -1.75 per element so that they stay below.
# For the victim user every product that enters s' of a strong, filler or victim row is a multiple of 2^-16 and the magnitudes sum to less
# than 2^8: s' is exact in fp32 in any order (test_prefilter_ref_cpu.py checks it from the values).
# All values are 0 or have 2^-4 <= |x| <= 2: the tables stay inside the chain's scale-invariant range for every pair of SCALES.
# ---------------------------------------------------------------------------------------------------------------------------------------
G16 = 2.0 ** -16
RES = 58 * 2.0 ** -23                       # 0.906 x 2^-17: the residual, on the fp32 grid of [1, 2)
MID = 2.0 ** -8 - 2.0 ** -15                # the mid part of the two-sided rows
N_STRONG, N_FILLER = 50, 14
N_ITEMS = 600
VICTIM_ITEM = 300
N_USERS = 34                                # rows 5 and 33 are the victim user; the others are benign
IN_WINDOW = [(0, 0), (0, -40), (40, 0)]     # the pairs of SCALES that leave every norm inside the magnitude window: the mode runs as itself
VICTIM_USERS = (5, 33)
Q_FULL = list(range(32))                                         # the victim user inside a full tile
Q_TAIL = [u for u in range(33) if u != 5] + [33]                 # ... and as the only row of a ragged third tile


class VictimTable:
    def __init__(self, name, d, two_sided, negative, seed):
        assert not (two_sided and negative)
        rng = np.random.default_rng(seed)
        self.name, self.d = name, d
        sign = -1.0 if negative else 1.0
        base = sign * (1.0 + (MID if two_sided else 1.5 * 2.0 ** -9 if negative else 2.0 ** -9))
        n_s, n_f = d // 4, d // 9
        cols = rng.permutation(d)
        strong = np.full(d, base); strong[cols[:n_s]] += G16
        filler = np.full(d, base); filler[cols[:n_f]] += G16
        victim = np.full(d, base + RES)
        n_low = N_ITEMS - N_STRONG - N_FILLER - 1
        if negative:
            low = -rng.choice([1.25, 1.5, 1.75], size=(n_low, d))
        else:
            low = rng.choice([0.0625, 0.125, 0.25, 0.5], size=(n_low, d)) * rng.choice([-1.0, 1.0], size=(n_low, d))
        if not negative:
            low[::37] = 0.0                                      # a few all-zero rows: a zero norm that is a true zero (score 0: below the strong rows)
        rows = np.concatenate([np.tile(strong, (N_STRONG, 1)), np.tile(filler, (N_FILLER, 1)), low])
        kind = np.array([0] * N_STRONG + [1] * N_FILLER + [3] * n_low)
        perm = rng.permutation(len(rows))
        rows, kind = rows[perm], kind[perm]
        self.ei = np.insert(rows, VICTIM_ITEM, victim, axis=0).astype(F32)
        self.kind = np.insert(kind, VICTIM_ITEM, 2)              # 0 strong, 1 filler, 2 victim, 3 low
        assert self.ei.shape == (N_ITEMS, d) and (self.ei.astype(np.float64)[VICTIM_ITEM] == victim).all()
        # benign users: every row sums to zero exactly, so the near-constant strong, filler and victim rows score ~0 for them and their
        # top K comes from the low rows, far apart: their proofs hold, and only the victim user's tile goes to the exact sweep
        half = rng.choice([0.25, 0.5, 1.0], size=(N_USERS, d // 2))
        eu = rng.permuted(np.concatenate([half, -half], axis=1), axis=1)
        eu[list(VICTIM_USERS)] = 1.0 + MID + RES if two_sided else 1.0
        self.eu = eu.astype(F32)
        assert (self.eu.astype(np.float64) == eu).all()
        for t in (self.eu, self.ei):
            a = np.abs(t[t != 0])
            assert a.min() >= 2.0 ** -4 and a.max() <= 2.0
        self._chain = None

    @property
    def chain(self):
        """chain_scores(eu, ei) [N_USERS, N_ITEMS], computed once (read-only)."""
        if self._chain is None:
            self._chain = chain_scores(self.eu, self.ei)
            self._chain.setflags(write=False)
        return self._chain

    def ids(self, kind):
        return np.flatnonzero(self.kind == kind)

    def scaled(self, a, b):
        """(eu 2^a, ei 2^b) float32 and the chain scores times 2^(a + b): exact while nothing under- or overflows (test_prefilter_ref_cpu)."""
        with np.errstate(over="raise", under="raise"):
            return np.ldexp(self.eu, a).astype(F32), np.ldexp(self.ei, b).astype(F32), np.ldexp(self.chain, a + b).astype(F32)


_SPECS = {
    "one64": (64, False, False), "two64": (64, True, False), "neg64": (64, False, True),
    "one128": (128, False, False), "two128": (128, True, False),
    "one20": (20, False, False), "two20": (20, True, False),
}
TABLES = list(_SPECS)
_CACHE = {}


def victim_table(name):
    if name not in _CACHE:
        d, two, neg = _SPECS[name]
        _CACHE[name] = VictimTable(name, d, two, neg, seed=[d, int(two), int(neg)])
    return _CACHE[name]
