"""The yardstick of tests/test_gpu_foldin.py for llmrec_fold_in_users_f32 (llmrec_amd/csrc/foldin.hip): the definition restated in
float64, a bound PER OUTPUT ELEMENT derived from the kernel's own order of operations, an fp32 emulation of that order (to check the bound
without a device) and the case table. numpy only; nothing here imports llmrec_amd or torch, and nothing calls the kernel.

DEFINITION (include/llmrec_hip.h; T [n_items, C d], C = L + 3 + n_attr slices: chain 0 .. L - 1 | image | text | attributes | profile)
  S = sum over the row's entries i, 0 <= i < n_items, of T[i] (repeats count, other entries add nothing);  g(c) = w S[slice c];
  out = (id_row + g(0) + ... + g(L - 2) + softmax(g(L - 1))) / (L + 1) + c_m n(g(L)) + c_m n(g(L + 1)) + c_u n(g(C - 1))
        + sum_k c_a n(g(L + 2 + k)),   n(x) = x / max(||x||, 1e-12); w is the caller's fp32 row_scale, taken as it is.

ORDER OF THE KERNEL (what emulate() restates)
  segments of SEG = 256 entries; inside a segment of len entries four runs of q = ceil(len / 4) consecutive entries, each a serial
  fp32 chain from 0 in the order given (an entry that adds nothing adds an exact 0), met as (r0 + r1) + (r2 + r3); the segment sums
  added in order. Then, per row: x = fl(w S); the softmax with one lane per column pair (c, c + 64): max, e = exp(fl(x - max)),
  fl(e_c + e_{c + 64}), a 64-lane butterfly (xor 32 .. 1), inv = fl(1 / s), fl(e inv); the mean: id_row, + every layer in order, times
  fl(1 / (L + 1)); a normalised term: fma(x_{c + 64}, x_{c + 64}, fl(x_c x_c)), the butterfly, sqrt, max with 1e-12f, fl(rate / nrm),
  fma into the accumulator.

BOUNDS (u = 2^-24; every constant was fixed before the first device run)
  gather     a term of the sum passes at most q0 + 2 + (nseg - 1) additions, q0 = ceil(min(len, 256) / 4), then the product with w:
             |err g_c| <= (q0 + nseg + 1 + 1 + 1) u w sum_i |T[i]_c| =: eg_c (the last 1 for the second-order terms; len counts
             every entry of the row, also those that add nothing).
  softmax    the kernel's own roundings as tests/_rowops_ref.py derives them for softmax_fwd_kernel, with a lane chain of 1 addition and
             a butterfly of 6 in place of L + 4 (taken as 8): rel <= u (|t_c| + max |t| + 2 E_EXP + 8 + C_SM_FWD), t = x - max; the inputs'
             error eg moves y_c by at most the factor exp(+-(eg_c + max eg)): y_c expm1(eg_c + max_j eg_j), rigorous, and the own term
             is taken on the larger value. An exponent below fp32's range flushes: + 2 TINY.
  mean       L additions, the product, the rounding of 1 / (L + 1), + 1: (L + 3) u ms sum_l |term_l| + ms sum_l err(term_l).
  normalise  the input error through n(x), first order: (eg_c + |n_c| sum_j |n_j| eg_j) rate / ||x||, times 1.05 for the second order
             (asserted: ||eg|| <= 1e-2 ||x||, so the neglected terms are below 3 % of the first-order ones); under the clamp
             rate eg_c / 1e-12. Own roundings as _rowops_ref's fusion forward with the chain 2 + 6 = 8 in place of L + 4:
             (8 / 2 + C_FF) u |contribution|, and 2 u |partial sum| for each fma into the accumulator.
             Every row's norm is either <= 1e-13 (or 0) or >= 1e-9 (asserted): no row sits where fp32 and fp64 could clamp differently.
  + 4 TINY on every element (results below fp32's normal range).
"""
from __future__ import annotations

import zlib
from typing import List, NamedTuple, Optional

import numpy as np

from tests._rowops_ref import C_FF, C_SM_FWD, E_EXP, EPS32, TINY, U

f32, f64 = np.float32, np.float64
SEG = 256
LANES = 64
N_ITEMS = 3000
N_ROWS = 203
LENGTHS = (0, 1, 2, 63, 64, 65, 257, 3000, 5000)
# which path of the kernel a length takes: "one" = one segment, finished by the block that summed it (fi_gather_kernel alone); "long" =
# several segments, each summed by a block of its own, added and finished by fi_finish_long_kernel. Within "one": 0 = no entry at all,
# 1 / 2 = fewer entries than waves (empty runs), 63 / 64 / 65 = runs of 16, 16 and 17 (a ragged last run), around one wave's worth;
# within "long": 257 = a second segment of ONE entry, 3000 = 12 segments, the last ragged (184), 5000 = 20 segments with repeats.
PATH = {0: "one", 1: "one", 2: "one", 63: "one", 64: "one", 65: "one", 257: "long", 3000: "long", 5000: "long"}
D_ALL, L_ALL, N_ATTR_ALL = (64, 128, 20, 7), (1, 2, 3), (0, 5)
RATES = (float(f32(0.55)), float(f32(0.038)), float(f32(0.005)))  # c_m, c_u, c_a: the magnitudes the drop-in's defaults have
SPRINKLED_ROW = 5 * len(LENGTHS) + 5                              # a row of 65 entries, sprinkled with -1, n_items and n_items + 5
HOT_ROW = 7 * len(LENGTHS) + 6                                    # a row of 257 entries whose scale makes the softmax see large logits
HOT_SCALE = 40.0


def ceil_div(a, b):
    return -(-a // b)


def n_slices(L, n_attr):
    return L + 3 + n_attr


def norm_slices(L, n_attr):
    """[(slice, rate index)] in the order the terms are added: image, text, profile, attributes"""
    return [(L, 0), (L + 1, 0), (L + 2 + n_attr, 1)] + [(L + 2 + k, 2) for k in range(n_attr)]


def nseg(length):
    return max(1, ceil_div(length, SEG))


def depth(length):
    """the additions a term of the row's sum passes at most"""
    return ceil_div(min(length, SEG), 4) + 2 + nseg(length) - 1


# ------------------------------------------------------------------------------------------------------------------------------------
# the definition in float64, with the bound
# ------------------------------------------------------------------------------------------------------------------------------------
def count_matrix(rows: List[np.ndarray], n_items: int) -> np.ndarray:
    """[n, n_items] float64: how often row r names item i (entries outside [0, n_items) are not counted)"""
    cnt = np.zeros((len(rows), n_items), dtype=f64)
    for r, h in enumerate(rows):
        h = np.asarray(h, dtype=np.int64)
        cnt[r] = np.bincount(h[(h >= 0) & (h < n_items)], minlength=n_items)
    return cnt


def gathered(T, rows):
    """(sum of T's rows, sum of |T|'s rows) at each row's entries, float64 [n, C d] each: the part of reference() that does not depend
    on the scale, the id rows or the rates"""
    T64 = np.asarray(T, dtype=f32).astype(f64)
    cnt = count_matrix(rows, T64.shape[0])
    return cnt @ T64, cnt @ np.abs(T64)


def reference(T, rows, w, id_rows, L, n_attr, d, rates, sums=None):
    """(out float64 [n, d], bound float64 [n, d]) from the fp32 table's values; rows: the entries of each new user AS GIVEN;
    sums: gathered(T, rows), where the caller has them"""
    n, C = len(rows), n_slices(L, n_attr)
    assert np.asarray(T).shape[1] == C * d
    plain, absolute = gathered(T, rows) if sums is None else sums
    w64 = np.asarray(w, dtype=f32).astype(f64)[:, None]
    lens = np.array([len(h) for h in rows])
    dep = np.array([depth(int(x)) for x in lens], dtype=f64)[:, None]
    G = w64 * plain                                                # g of every slice, [n, C d]
    EG = (dep + 3) * U * np.abs(w64) * absolute
    sl = lambda A, c: A[:, c * d:(c + 1) * d]
    ms = 1.0 / (L + 1)
    acc = np.zeros((n, d)) if id_rows is None else np.asarray(id_rows, dtype=f32).astype(f64)
    absum, err = np.abs(acc), np.zeros((n, d))
    for l in range(L):
        x, eg = sl(G, l), sl(EG, l)
        if l == L - 1:
            t = x - x.max(axis=1, keepdims=True)
            e = np.exp(t)
            y = e / e.sum(axis=1, keepdims=True)
            grow = eg + eg.max(axis=1, keepdims=True)
            own = U * (np.abs(t) + np.abs(t).max(axis=1, keepdims=True) + 2 * E_EXP + 8 + C_SM_FWD)
            x, eg = y, y * np.expm1(grow) + y * np.exp(grow) * own + 2 * TINY
        acc, absum, err = acc + x, absum + np.abs(x), err + eg
    out = ms * acc
    bound = ms * err + (L + 3) * U * ms * absum
    for c, ri in norm_slices(L, n_attr):
        x, eg, rate = sl(G, c), sl(EG, c), float(f32(rates[ri]))
        nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        live = nrm >= EPS32
        assert ((nrm <= 1e-13) | (nrm >= 1e-9)).all(), "a row between the clamp and 1e-9"
        safe = np.where(live, nrm, 1.0)
        assert (np.sqrt((eg * eg).sum(axis=1, keepdims=True)) <= 1e-2 * safe)[live].all()
        unit = x / safe
        moved = np.where(live, 1.05 * (eg + np.abs(unit) * (np.abs(unit) * eg).sum(axis=1, keepdims=True)) / safe, eg / EPS32)
        contrib = rate * x / np.maximum(nrm, EPS32)
        out = out + contrib
        bound = bound + abs(rate) * moved + U * ((8 / 2 + C_FF) * np.abs(contrib) + 2 * np.abs(out))
    return out, bound + 4 * TINY


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel's order in float32
# ------------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a b + c) through float64 (an emulation to check a bound; the product of two floats is exact in a double)"""
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def emu_sums(T, rows):
    """float32 [n, C d]: the sums of every row in the kernel's order (rows of one length walk their chains together)"""
    T = np.asarray(T, dtype=f32)
    out = np.zeros((len(rows), T.shape[1]), dtype=f32)
    lens = np.array([len(h) for h in rows], dtype=np.int64)
    for n in np.unique(lens):
        which = np.flatnonzero(lens == n)
        H = np.stack([np.asarray(rows[r], dtype=np.int64) for r in which]).reshape(len(which), n)
        ok = (H >= 0) & (H < T.shape[0])
        total = None
        for k in range(nseg(int(n))):
            seg, live = H[:, k * SEG:(k + 1) * SEG], ok[:, k * SEG:(k + 1) * SEG]
            q = ceil_div(seg.shape[1], 4)
            runs = np.zeros((len(which), 4, T.shape[1]), dtype=f32)
            first = np.arange(4) * q
            for j in range(q):                                     # step j of the four chains (an exact 0 where a chain adds nothing)
                e = first + j
                on = e < np.minimum(first + q, seg.shape[1])
                e = np.where(on, e, 0)
                add = on[None, :] & live[:, e]
                runs = (runs + np.where(add[:, :, None], T[np.where(add, seg[:, e], 0)], f32(0))).astype(f32)
            s = ((runs[:, 0] + runs[:, 1]).astype(f32) + (runs[:, 2] + runs[:, 3]).astype(f32)).astype(f32)
            total = s if total is None else (total + s).astype(f32)
        out[which] = total
    return out


def emu_row_sum(T, h):
    """the [C d] fp32 sums of one row in the kernel's order"""
    return emu_sums(T, [h])[0]


def _butterfly(v):
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ off]).astype(f32)
    return v


def _lanes(x):
    """[n, d] -> the two registers [n, 64] of a lane (columns c and c + 64; 0 beyond d)"""
    p = np.zeros((x.shape[0], 2 * LANES), dtype=f32)
    p[:, :x.shape[1]] = x
    return p[:, :LANES], p[:, LANES:]


def _unlanes(a0, a1, d):
    return np.concatenate([a0, a1], axis=1)[:, :d]


def emulate(T, rows, w, id_rows, L, n_attr, d, rates, mutant=None, S=None):
    """float32 [n, d] in the kernel's order (S: emu_sums(T, rows), where the caller has them). mutants (each wrong on purpose):
    no_softmax, deg_plus_1 (w from len + 1), swap_profile_image, mean_without_layer0 (divisor L instead of L + 1)"""
    n = len(rows)
    S = emu_sums(T, rows) if S is None else S
    w = np.asarray(w, dtype=f32)
    if mutant == "deg_plus_1":
        w = ((np.array([len(h) for h in rows], dtype=f64) + 1.0 + 1e-8) ** -0.5).astype(f32)
    col = np.arange(2 * LANES).reshape(2, LANES)
    in0, in1 = (col[0] < d)[None], (col[1] < d)[None]
    g = lambda c: _lanes((w[:, None] * S[:, c * d:(c + 1) * d]).astype(f32))
    acc0, acc1 = _lanes(np.zeros((n, d), dtype=f32) if id_rows is None else np.asarray(id_rows, dtype=f32))
    for l in range(L):
        x0, x1 = g(l)
        if l == L - 1 and mutant != "no_softmax":
            mx = np.maximum(np.where(in0, x0, -np.inf), np.where(in1, x1, -np.inf)).max(axis=1, keepdims=True).astype(f32)
            with np.errstate(under="ignore"):
                e0 = np.where(in0, np.exp((x0 - mx).astype(f32)), f32(0)).astype(f32)
                e1 = np.where(in1, np.exp((x1 - mx).astype(f32)), f32(0)).astype(f32)
            inv = (f32(1) / _butterfly((e0 + e1).astype(f32))).astype(f32)
            with np.errstate(under="ignore"):
                x0, x1 = (e0 * inv).astype(f32), (e1 * inv).astype(f32)
        acc0, acc1 = (acc0 + x0).astype(f32), (acc1 + x1).astype(f32)
    ms = f32(1.0) / f32(L if mutant == "mean_without_layer0" else L + 1)
    acc0, acc1 = (acc0 * ms).astype(f32), (acc1 * ms).astype(f32)
    order = norm_slices(L, n_attr)
    if mutant == "swap_profile_image":
        order = [(order[2][0], 0), order[1], (order[0][0], 1)] + order[3:]
    for c, ri in order:
        x0, x1 = g(c)
        ss = _butterfly(_fma(x1, x1, _fma(x0, x0, f32(0))))
        nrm = np.maximum(np.sqrt(ss).astype(f32), f32(1e-12))
        wt = (f32(rates[ri]) / nrm).astype(f32)
        acc0, acc1 = _fma(wt, x0, acc0), _fma(wt, x1, acc1)
    return _unlanes(acc0, acc1, d)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class Case(NamedTuple):
    d: int
    L: int
    n_attr: int
    T: np.ndarray                   # float32 [N_ITEMS, C d]
    rows: List[np.ndarray]          # int32 entries of each of the N_ROWS new users, as given to the kernel
    w: np.ndarray                   # float32 [N_ROWS]
    id_rows: np.ndarray             # float32 [N_ROWS, d]
    tiny_slice: int                 # the slice scaled so that its normalise takes the clamp

    @property
    def name(self):
        return "d%d-L%d-a%d" % (self.d, self.L, self.n_attr)

    @property
    def rowptr(self):
        return np.concatenate([[0], np.cumsum([len(h) for h in self.rows])]).astype(np.int32)

    @property
    def colidx(self):
        return np.concatenate(self.rows).astype(np.int32)


def row_scale(lengths):
    """float32((float64(deg) + 1e-8) ** -0.5)"""
    return ((np.asarray(lengths, dtype=f64) + 1e-8) ** -0.5).astype(f32)


def case(d, L, n_attr) -> Case:
    """N_ROWS rows whose lengths cycle through LENGTHS: 3000 = every item once (shuffled), 5000 = with repeats. Slice c of T is scaled by
    2^(c mod 5 - 3); the text slice by 1e-16: every row's text term takes the 1e-12 clamp. Row SPRINKLED_ROW carries entries that add
    nothing; row HOT_ROW's scale is HOT_SCALE times its D^-1/2 (the caller's to choose): its last layer's logits span tens of units."""
    rng = _rng("foldin", d, L, n_attr)
    C = n_slices(L, n_attr)
    T = rng.standard_normal((N_ITEMS, C * d))
    T = T + 0.05 * np.sign(T)
    for c in range(C):
        T[:, c * d:(c + 1) * d] *= 2.0 ** (c % 5 - 3)
    tiny = L + 1
    T[:, tiny * d:(tiny + 1) * d] *= 1e-16 / 2.0 ** (tiny % 5 - 3)
    rows = []
    for r in range(N_ROWS):
        n = LENGTHS[r % len(LENGTHS)]
        if n == N_ITEMS:
            h = rng.permutation(N_ITEMS)
        else:
            h = rng.integers(0, N_ITEMS, n)
        rows.append(h.astype(np.int32))
    assert len(rows[SPRINKLED_ROW]) == 65 and len(rows[HOT_ROW]) == 257
    rows[SPRINKLED_ROW][[0, 7, 16, 33, 64]] = (-1, N_ITEMS, -1, N_ITEMS + 5, -1)
    w = row_scale([len(h) for h in rows])
    w[HOT_ROW] = f32(w[HOT_ROW] * HOT_SCALE)
    id_rows = (rng.standard_normal((N_ROWS, d)) * 0.1).astype(f32)
    return Case(d, L, n_attr, T.astype(f32), rows, w, id_rows, tiny)


def cases():
    return [(d, L, a) for d in D_ALL for L in L_ALL for a in N_ATTR_ALL]
