"""The yardstick of tests/test_gpu_rowops_families.py for the row kernels of llmrec_amd/csrc/rowops.hip: the dispatch restated, fp64
references with a bound PER ELEMENT, fp32 emulations of the kernels' own order (to check the bounds without a device) and the case table.
numpy only; nothing here imports llmrec_amd or torch (fma32 is tests/_dense_ref.py's closed-rounding step).

DISPATCH (include/llmrec_hip.h "Only the float4 row family (d % 4 == 0, 16-byte aligned rows, d <= 512) ..." and the entry points)
  A row is swept by 16 lanes; lane gl owns the elements (k 16 + gl) VEC + q, k < NCHUNK, q < VEC. Every entry takes the float4 family
  (VEC 4; NCHUNK 1, 2, 4, 8 for d <= 64, 128, 256, 512) when d % 4 == 0, every participating ld % 4 == 0 and every participating base is
  16-byte aligned (a NULL source does not take part), else the scalar family (VEC 1; NCHUNK 1, 4, 8, 16 for d <= 16, 64, 128, 256). A d
  beyond the family's last member is refused with LLMREC_EUNSUPPORTED before anything is launched; llmrec_fuse_fwd_multi_sumsq_compact_f32
  has the float4 family only and llmrec_step_rows_group_f32 only <4, 1>. A launch has min(ceil(rows / 16), 2048) blocks of 16 rows; block b
  takes the rows b 16 + i + j nblk 16. The paired launches give each problem its own block range and nblk.

BOUNDS (u = 2^-24, L = NCHUNK VEC = the length of a lane's chain; every constant was fixed before the first device run)
  Every fp32 operation rounds once: relative error <= u. "c" collects the roundings that are not part of a chain plus one u for the
  second-order terms (the largest first-order factor below is ~150 u = 1e-5, its square is far below u).
  dot / sum of a row     RowReg::dot is L fmaf steps (the padding slots add an exact 0) and four butterfly additions: every term passes
                         at most L + 4 roundings, |err| <= (L + 4 + 1) u sum|terms|.
  softmax forward        t = fl(z - max) carries u |t|, which exp() turns into the relative error |t| u of e_c; expf adds E_EXP ulp =
                         2 E_EXP u (an ulp is at most 2 u of the value). E_EXP = 3 is OpenCL's full-profile limit for exp, which the ROCm
                         device library is written to meet: a published limit, not a property of this code. The sum takes L additions per
                         lane and four in the butterfly; its terms carry at most max_j |t_j| u (a weighted mean of the e_j's errors); then
                         inv = fl(1 / s) and fl(e inv): 2, + 1 second order -> c = 3.
                         rel err(y_c) <= u (|t_c| + max_j |t_j| + 2 E_EXP + L + 4 + 3).
                         (The allowance 2 E_EXP u is taken ONCE for numerator and denominator together, as the issue sets it: expf errors
                         of full size and opposite sign in both would need 4 E_EXP u. np.exp in float32 and the device are both measured
                         against it - see profiles/experiments/rowops_families.md for the worst observed value.)
  softmax backward       g' = fl(alpha g_j): u. dot: (L + 4 + 1) u S on the rounded g', + u S for g' itself, S = sum_j |y_j alpha g_j|.
                         fl(g' - dot): the error of g' (u |alpha g_c|), of dot, and u |g' - dot|; fl(y (.)): u more. With
                         |g' - dot| <= |alpha g_c| + S that is 3 roundings on |alpha g_c| and 4 on S outside the chain, each counted as one
                         ulp = 2 u (a single rounding reaches u |value| just above a power of two, and the CPU soundness test demands
                         that the kernel's own order stays below HALF of the bound):
                         |err| <= u |y_c| (C1 |alpha g_c| + (L + 4 + C2) S), C1 = 6, C2 = 8.
                         Listed kernel: its chain is c += 16 (L = ceil(d / 16)); fl(post_scale (.)) adds u |dz|. (The compiler may contract
                         alpha g - dot into one fma there: fewer roundings, the same bound.)
  fusion forward         mean part: n_mean - 1 additions, one product: <= (n_mean + 2) u |mean_scale| sum_t |m_t,c|. A normalised term:
                         ||x||^2 has relative error (L + 4 + 1) u, sqrt halves it and rounds (+ 1), rate / nrm rounds (+ 1), + 1 second order:
                         ((L + 4) / 2 + C_FF) u |rate x_c| / max(||x||, eps), C_FF = 3.5; the fmaf into the accumulator rounds the PARTIAL
                         sum after term i: 2 u |acc_i| each (the issue's n_norm u |out_c| with the partial sums in place of the final value,
                         which a cancellation between terms can make smaller than what was rounded; counted twice - see the backward).
  fusion backward        h = (L + 5) / 2 + 2 bounds inv = 1 / fl(sqrt(fl(<x, x>))) (in u). proj = fl(fl(dot inv) inv): (L + 5) S' + (2 + 2 h) P
                         with S' = sum_j |x_j g_j| / ||x||^2, P = |<x, g>| / ||x||^2; w = fl(rate inv): h + 1; fl(g - fl(x proj)): u |x_c| P and
                         u |tmp|; fl(o + fl(w tmp)): 2 u |w tmp| and the rounding of the result. With |tmp| <= |g_c| + |x_c| P:
                         |err| <= |w| u [C1 |g_c| + |x_c| (L + 4 + C2) S' + C3 |x_c| P],  C1 = h + 3 + 1, C2 = 1 + 1, C3 = 3 h + 6 + 1
                         (the cancellation in g - x proj is why S' and not P carries the chain length). Clamp branch (||x|| < 1e-12):
                         rate 1e12 g, 3 u. Adding the old value / source and the regulariser: c = 2 each - the addition rounds
                         |base + grad| once, the fmaf |base + grad + reg2 x_c| once, and each is counted twice, because one rounding alone
                         reaches u |value| just above a power of two while the CPU soundness test demands that the kernel's own order
                         stays below HALF of the bound: 4 u (|base| + |grad|) + 2 u |reg2 x_c|.
                         (Contraction of w (g - x proj) + o into fmas removes roundings: the same bound.)
  sumsq                  (ceil(n / (blocks 256)) + 8 + 4 + 8 + 2) u |coef| sum x^2 + u |old|: a thread's fma chain, the block tree, the
                         final kernel's four partials per thread (1024 / 256), its tree, coef and the addition.
  fuse_fwd_multi_sumsq   a partial sums (L + 5) u-accurate squared norms: passes n_sumsq additions in a thread, a tree of 8.
  axpy                   fl(alpha alpha_dev), fl(a x), fl(y + .): 3 u (|a x| + |y_old|).   scale_rows: u |s x|.
  gather_mean            n_terms - 1 additions and the scale: (n_terms + 1) u |scale| sum_t |x_t|.
  weighted_colsum        a block's fma chain over ceil(rows / blocks) rows, four interleaved sums of ceil(blocks / 4) partials + 2, then one
                         addition per group that shares the destination and one for accumulate.
  AdamW                  one ulp = 2 u per operation of adamw_element, propagated through m, v, denom and p in fp64 magnitudes (adamw()); the
                         sqrt's error is taken from sqrt(v -+ (e_v + 2^-126)) so a v that underflows (|g| = 1e-30) is covered. The same
                         bound serves adamw_kernel, whose products may be contracted: that only removes roundings.

EMULATIONS (float32 numpy, the kernels' order): emu_softmax_fwd / _bwd, emu_fuse_fwd / _bwd, emu_sumsq, with the mutants
tests/test_rowops_ref_cpu.py uses to show that the bounds are not vacuous. They exist to check the bounds, not to be compared with the
device bit for bit (expf is not reproducible off the device).
"""
from __future__ import annotations

import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

from tests._dense_ref import fma32

U = 2.0 ** -24
E_EXP = 3                                             # ulp allowed to expf
TINY = 2.0 ** -126
SENTINEL = 12345.0                                    # what an output and its surroundings hold before a call
GUARD = 64                                            # tests/_eval_ref.GUARD (restated: this module imports no torch)
EPS32 = float(np.float32(1e-12))                      # "1e-12f": F.normalize's eps as the kernels hold it
BIG32 = float(np.float32(1e12))                       # "1e12f": the clamp branch of the backward
F32_MAX = float(np.finfo(np.float32).max)
RL = 16
ROWS_PER_BLOCK = 16
MAX_BLOCKS = 2048
SUMSQ_BLOCKS = 1024
COLSUM_BLOCKS = 128
BIG_ROWS = MAX_BLOCKS * ROWS_PER_BLOCK + 19           # the smallest interesting row count with a second pass of the sweep
SMALL_ROWS = (1, 15, 16, 17, 67)
FLAT_BIG = 2 ** 21 + 777
C_SM_FWD, C_SM_B1, C_SM_B2, C_FF = 3, 6, 8, 3.5
EUNSUPPORTED, EINVAL = -4, -1

f32, f64 = np.float32, np.float64


def ceil_div(a, b):
    return -(-a // b)


def _ceil4(x):
    return (x + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------------
FAMILY = {True: ((64, 1), (128, 2), (256, 4), (512, 8)), False: ((16, 1), (64, 4), (128, 8), (256, 16))}
ALL_INSTANCES = {(4, 1), (4, 2), (4, 4), (4, 8), (1, 1), (1, 4), (1, 8), (1, 16)}
TEMPLATED = ("softmax_fwd", "softmax_bwd", "fuse_fwd", "fuse_bwd", "fuse_fwd_multi", "fuse_bwd_src_multi")


def instance(d, vec4):
    """(VEC, NCHUNK) of the kernel an entry launches, None where it refuses"""
    for limit, nchunk in FAMILY[bool(vec4)]:
        if d <= limit:
            return (4 if vec4 else 1, nchunk)
    return None


def vec4_of(d, lds, base_mod16s):
    """the rule every entry applies; None entries (a NULL source) do not take part"""
    return d % 4 == 0 and all(ld % 4 == 0 for ld in lds if ld is not None) and all(b % 16 == 0 for b in base_mod16s if b is not None)


def grid_for(work, per_block, max_blocks=MAX_BLOCKS):
    return int(min(max(ceil_div(work, per_block), 1), max_blocks))


def row_blocks(rows):
    return grid_for(rows, ROWS_PER_BLOCK)


def row_passes(rows):
    """passes of ROW_LOOP_HEADER / ROW_LOOP_MULTI over a problem of `rows` rows"""
    return ceil_div(rows, row_blocks(rows) * ROWS_PER_BLOCK)


def flat_passes(n, per_block, max_blocks=MAX_BLOCKS):
    """passes of a flat grid-stride kernel: sumsq (256 * 8, SUMSQ_BLOCKS), axpy / adamw_f32 / scale_rows (256 * 4)"""
    return ceil_div(n, grid_for(n, per_block, max_blocks) * 256)


def sumsq_blocks(n):
    return 1 if n == 0 else grid_for(n, 256 * 8, SUMSQ_BLOCKS)


def visits(rows, nblk, stride_blocks=None):
    """how often the sweep of nblk blocks visits each row; stride_blocks: a mutant's row stride in blocks (the kernel's: nblk)"""
    stride = (nblk if stride_blocks is None else stride_blocks) * ROWS_PER_BLOCK
    count = np.zeros(rows, dtype=np.int64)
    for b in range(nblk):
        start = b * ROWS_PER_BLOCK
        while start < rows:
            count[start:start + ROWS_PER_BLOCK] += 1
            start += stride
    return count


# ------------------------------------------------------------------------------------------------------------------------------------
# (b), (c) fp64 references with their per-element bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _64(x):
    return np.asarray(x, dtype=f32).astype(f64)


def softmax_fwd(Z, L):
    z = _64(Z)
    t = z - z.max(axis=1, keepdims=True)
    e = np.exp(t)
    y = e / e.sum(axis=1, keepdims=True)
    return y, U * y * (np.abs(t) + np.abs(t).max(axis=1, keepdims=True) + 2 * E_EXP + L + 4 + C_SM_FWD)


def softmax_expf_ulp(dev, Z, L):
    """(worst relative error of dev in u; the worst of that error less |t_c| + max |t| - what the rounded exponent argument explains - in
    u, to be held against 2 E_EXP + L + 4 + c; the worst share left to expf in ulp once the arithmetic's L + 4 + c is taken off as well,
    halved because an ulp is 2 u, to be held against E_EXP; negative: the allowance for expf was not touched)"""
    z = _64(Z)
    t = np.abs(z - z.max(axis=1, keepdims=True))
    y = softmax_fwd(Z, 0)[0]
    rel = np.abs(np.asarray(dev, dtype=f64) - y) / (U * y)
    rest = rel - (t + t.max(axis=1, keepdims=True))
    return float(rel.max()), float(rest.max()), float(((rest - (L + 4 + C_SM_FWD)) / 2).max())


def softmax_bwd(Y, G, alpha, L, post_scale=None):
    """dz = y (alpha g - <y, alpha g>) [* post_scale[r]]; L = the chain length of the kernel that runs (listed: ceil(d / 16))"""
    y, ag = _64(Y), float(f32(alpha)) * _64(G)
    S = np.abs(y * ag).sum(axis=1, keepdims=True)
    dz = y * (ag - (y * ag).sum(axis=1, keepdims=True))
    bound = U * np.abs(y) * (C_SM_B1 * np.abs(ag) + (L + 4 + C_SM_B2) * S)
    if post_scale is not None:
        ps = _64(post_scale)[:, None]
        dz, bound = ps * dz, np.abs(ps) * (bound + U * np.abs(dz))
    return dz, bound


def fuse_fwd(means, mean_scale, norms, rates, L):
    ms = float(f32(mean_scale))
    shape = (means[0] if means else norms[0]).shape
    out, absum = np.zeros(shape), np.zeros(shape)
    for m in means:
        out, absum = out + _64(m), absum + np.abs(_64(m))
    out = ms * out
    bound = U * (len(means) + 2) * abs(ms) * absum
    for x, rate in zip(norms, rates):
        x = _64(x)
        nrm = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), EPS32)
        contrib = float(f32(rate)) * x / nrm
        out = out + contrib
        bound = bound + U * (((L + 4) / 2 + C_FF) * np.abs(contrib) + 2 * np.abs(out))
    return out, bound


def fuse_bwd(G, norms, rates, L, bases, n_reg, reg2):
    """[(value, bound)] per term. bases[i]: the old value (accumulate), the source (source mode) or None (overwrite / NULL source)."""
    g = _64(G)
    h = (L + 5) / 2 + 2
    c1, c2, c3 = h + 4, 2, 3 * h + 7
    res = []
    for i, (x, rate) in enumerate(zip(norms, rates)):
        x, rate = _64(x), float(f32(rate))
        n2 = (x * x).sum(axis=1, keepdims=True)
        nrm = np.sqrt(n2)
        live = nrm >= EPS32
        n2s, nrms = np.where(live, n2, 1.0), np.where(live, nrm, 1.0)
        P = (x * g).sum(axis=1, keepdims=True) / n2s
        S = np.abs(x * g).sum(axis=1, keepdims=True) / n2s
        w = rate / nrms
        grad = np.where(live, w * (g - x * P), rate * BIG32 * g)
        b = np.where(live, np.abs(w) * U * (c1 * np.abs(g) + np.abs(x) * ((L + 4 + c2) * S + c3 * np.abs(P))), 3 * U * np.abs(grad))
        base = np.zeros_like(g) if bases[i] is None else _64(bases[i])
        reg = float(f32(reg2)) * x if i < n_reg else np.zeros_like(g)
        res.append((base + grad + reg, b + 4 * U * (np.abs(base) + np.abs(grad)) + 2 * U * np.abs(reg)))
    return res


def sumsq(X, coef, old, blocks):
    """(value, bound) of out[0] = (old or 0) + coef * sum x^2; old None: overwrite"""
    x = _64(X)
    ssq = float((x * x).sum())
    c, o = float(f32(coef)), 0.0 if old is None else float(f32(old))
    return o + c * ssq, (ceil_div(max(x.size, 1), blocks * 256) + 8 + 4 + 8 + 2) * U * abs(c) * ssq + U * abs(o)


def multi_sumsq(norm_sets, L, adds):
    """the fp64 sum of the first n_sumsq norm terms of every problem (norm_sets: the arrays) and the bound on the fp64 sum of the
    partials; adds = passes * n_sumsq: the additions of a thread"""
    ssq = float(sum((_64(x) ** 2).sum() for x in norm_sets))
    return ssq, (L + 5 + adds + 8) * U * ssq


def axpy(X, Y_old, alpha, alpha_dev, accumulate):
    a = float(f32(alpha)) * (1.0 if alpha_dev is None else float(f32(alpha_dev)))
    ax, y0 = a * _64(X), (_64(Y_old) if accumulate else 0.0)
    return ax + y0, 3 * U * (np.abs(ax) + np.abs(y0))


def scale_rows(s, X):
    v = _64(s)[:, None] * _64(X)
    return v, U * np.abs(v)


def gather_mean(terms, idx, scale):
    sc = float(f32(scale))
    rows = [_64(t)[idx] for t in terms]
    return sc * sum(rows), (len(terms) + 1) * U * abs(sc) * sum(np.abs(r) for r in rows)


def weighted_colsum(X, w, n_groups, gw, dest, olds):
    """dest[q]: the destination of group q; olds[k]: its old value [gw] or None (overwrite). -> {k: (value, bound)}"""
    x = _64(X) * (1.0 if w is None else _64(w)[:, None])
    rows = x.shape[0]
    blocks = min(max(rows, 1), COLSUM_BLOCKS)
    depth = ceil_div(max(rows, 1), blocks) + ceil_div(blocks, 4) + 2 + n_groups + 1
    col, acol = x.sum(axis=0), np.abs(x).sum(axis=0)
    res = {}
    for k in sorted(set(dest)):
        v = np.zeros(gw) if olds[k] is None else _64(olds[k]).copy()
        a = np.abs(v)
        for q in range(n_groups):
            if dest[q] == k:
                v, a = v + col[gw * q:gw * q + gw], a + acol[gw * q:gw * q + gw]
        res[k] = (v, depth * U * a)
    return res


def adamw_state(t, lr, b1, b2):
    """state3 after t calls of llmrec_adamw_advance (adamw_advance_kernel: doubles of the float arguments, results rounded to float)"""
    lr, b1, b2 = float(f32(lr)), float(f32(b1)), float(f32(b2))
    return np.array([np.array(t, dtype=np.int32).view(f32), f32(lr / (1.0 - b1 ** t)), f32(np.sqrt(1.0 - b2 ** t))], dtype=f32)


def adamw(p, g, m, v, state, lr, b1, b2, eps, wd, g_scale=1.0):
    """one step in fp64 from the fp32 inputs: dict of (value, bound) for p, m, v and the gradient used (g_out). A v beyond the fp32 range
    is inf, and the update of that element 0, as in the kernel."""
    p, g, m, v = _64(p), _64(g), _64(m), _64(v)
    gs = float(f32(g_scale))
    decay = float(f32(1.0 - float(f32(lr)) * float(f32(wd))))
    step, bc2s, eps = float(state[1]), float(state[2]), float(f32(eps))
    w1, w2, b2 = float(f32(1.0) - f32(b1)), float(f32(1.0) - f32(b2)), float(f32(b2))
    u = 2 * U                                                     # one ulp per operation
    gi = gs * g
    eg = (0.0 if gs == 1.0 else u) * np.abs(gi)
    m1 = m + w1 * (gi - m)
    em = w1 * eg + u * (2 * w1 * np.abs(gi - m) + np.abs(m1)) + TINY
    v1 = w2 * gi * gi + b2 * v
    ev = u * (3 * w2 * gi * gi + b2 * v + v1) + TINY
    over = v1 > F32_MAX
    v1s, evs = np.where(over, 1.0, v1), np.where(over, 0.0, ev)
    sq = np.sqrt(v1s)
    e_sq = np.maximum(sq - np.sqrt(np.maximum(v1s - evs, 0.0)), np.sqrt(v1s + evs) - sq) + u * sq
    q = sq / bc2s
    denom = q + eps
    e_den = e_sq / bc2s + u * q + u * denom
    den_lo = denom - e_den
    assert (den_lo > 0).all()
    r = m1 / denom
    e_r = em / den_lo + np.abs(m1) * e_den / (den_lo * den_lo) + u * np.abs(r)
    pd = p * decay
    p1 = np.where(over, pd, pd - step * r)
    ep = u * np.abs(pd) + np.where(over, 0.0, step * (e_r + u * np.abs(r))) + u * np.abs(p1)
    return {"p": (p1, ep), "m": (m1, em), "v": (np.where(over, np.inf, v1), np.where(over, 0.0, ev)), "g_out": (gi, eg)}


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) fp32 emulations of the kernels' own order
# ------------------------------------------------------------------------------------------------------------------------------------
def lane_index(VEC, NCHUNK):
    """[16, L] element index of lane gl's j-th slot (k-major, q-minor: the order of the kernels' loops)"""
    k, gl, q = np.arange(NCHUNK)[None, :, None], np.arange(RL)[:, None, None], np.arange(VEC)[None, None, :]
    return ((k * RL + gl) * VEC + q).reshape(RL, NCHUNK * VEC)


def to_lanes(X, idx):
    """[rows, 16, L] float32: RowReg::load (slots at or beyond d hold 0)"""
    X = np.asarray(X, dtype=f32)
    pad = np.zeros((X.shape[0], int(idx.max()) + 1), dtype=f32)
    pad[:, :X.shape[1]] = X
    return pad[:, idx]


def from_lanes(V, idx, d):
    out = np.zeros((V.shape[0], d), dtype=f32)
    live = idx < d
    out[:, idx[live]] = V[:, live]
    return out


def butterfly(s, mutant=None):
    """group_sum<16>: xor 8, 4, 2, 1 over the lane axis ([rows, 16])"""
    lane = np.arange(RL)
    for off in (8, 4, 2) if mutant == "no_last_step" else (8, 4, 2, 1):
        s = (s + s[:, lane ^ off]).astype(f32)
    return s


def emu_dot(A, B, VEC, mutant=None):
    """RowReg::dot of two [rows, 16, L] registers -> [rows, 16, 1] (every lane's copy of the sum)"""
    L = A.shape[2]
    s = np.zeros(A.shape[:2], dtype=f32)
    for j in range(L - VEC if mutant == "no_last_chunk" else L):
        s = fma32(A[:, :, j], B[:, :, j], s)
    return butterfly(s, mutant)[:, :, None]


def emu_softmax_fwd(Z, VEC, NCHUNK, mutant=None):
    d = Z.shape[1]
    idx = lane_index(VEC, NCHUNK)
    z, live = to_lanes(Z, idx), (idx < d)[None]
    mx = np.asarray(Z, dtype=f32).max(axis=1)[:, None, None]
    with np.errstate(under="ignore"):
        e = np.where(live, np.exp((z - mx).astype(f32)), f32(0)).astype(f32)
    s = np.zeros(e.shape[:2], dtype=f32)
    for j in range(e.shape[2] - VEC if mutant == "no_last_chunk" else e.shape[2]):
        s = (s + e[:, :, j]).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):          # (a mutant's sum may be 0)
        inv = (f32(1) / butterfly(s, mutant)).astype(f32)[:, :, None]
        return from_lanes((e * inv).astype(f32), idx, d)


def emu_softmax_bwd(Y, G, alpha, VEC, NCHUNK, mutant=None):
    d = Y.shape[1]
    idx = lane_index(VEC, NCHUNK)
    y, g = to_lanes(Y, idx), to_lanes(G, idx)
    if mutant != "no_alpha":
        g = (g * f32(alpha)).astype(f32)
    dot = emu_dot(y, g, VEC, mutant)
    return from_lanes((y * (g - dot).astype(f32)).astype(f32), idx, d)


def emu_fuse_fwd(means, mean_scale, norms, rates, VEC, NCHUNK, mutant=None):
    d = (means[0] if means else norms[0]).shape[1]
    idx = lane_index(VEC, NCHUNK)
    acc = np.zeros((len((means[0] if means else norms[0])), RL, idx.shape[1]), dtype=f32)
    for m in means:
        acc = (acc + to_lanes(m, idx)).astype(f32)
    if mutant != "mean_scale_late":
        acc = (acc * f32(mean_scale)).astype(f32)
    for x, rate in zip(norms, rates):
        t = to_lanes(x, idx)
        root = np.sqrt(emu_dot(t, t, VEC, mutant)).astype(f32)
        nrm = np.minimum(root, f32(1e-12)) if mutant == "clamp_wrong" else np.maximum(root, f32(1e-12))
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            w = (f32(rate) / nrm).astype(f32)
            acc = fma32_any(w, t, acc)
    if mutant == "mean_scale_late":
        acc = (acc * f32(mean_scale)).astype(f32)
    return from_lanes(acc, idx, d)


def fma32_any(a, b, c):
    """fma32 where a mutant may have produced inf / nan (the closed-rounding step insists on finite, normal values)"""
    a, b, c = np.broadcast_arrays(a, b, c)
    ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    with np.errstate(invalid="ignore", over="ignore"):
        plain = (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    if ok.all():
        return fma32(a, b, c)
    return plain


def emu_fuse_bwd(G, norms, rates, bases, n_reg, reg2, VEC, NCHUNK, mutant=None, count=None):
    """[dterm float32] per term, one fuse_bwd_kernel / fuse_bwd_src_multi_rows pass; count[r] > 1 (a mutant sweep that visits a row
    again, accumulate mode): the pass is repeated on those rows with its own result as the old value"""
    d = G.shape[1]
    idx = lane_index(VEC, NCHUNK)
    g = to_lanes(G, idx)
    res = []
    for i, (x, rate) in enumerate(zip(norms, rates)):
        t = to_lanes(x, idx)
        nn = np.sqrt(emu_dot(t, t, VEC, mutant)).astype(f32)
        live = (nn < f32(1e-12)) if mutant == "clamp_wrong" else (nn >= f32(1e-12))
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            inv = (f32(1) / nn).astype(f32)
            proj = ((emu_dot(t, g, VEC, mutant) * inv).astype(f32) * inv).astype(f32)
            w = (f32(rate) * inv).astype(f32)
            a = (w * (g - (t * proj).astype(f32)).astype(f32)).astype(f32)
        b = ((f32(rate) * f32(1e12)).astype(f32) * g).astype(f32)
        o = np.zeros_like(g) if bases[i] is None else to_lanes(bases[i], idx)
        times = 1 if count is None else int(count.max())
        for rep in range(times):
            with np.errstate(over="ignore", invalid="ignore"):
                new = (o + np.where(live, a, b)).astype(f32)
                if i < n_reg + (1 if mutant == "reg_one_more" else 0):
                    new = fma32_any(f32(reg2), t, new)
            o = new if count is None else np.where((count > rep)[:, None, None], new, o)
        res.append(from_lanes(o, idx, d))
    return res


def emu_sumsq(X, coef, old, blocks, mutant=None):
    """sumsq_partial_kernel + sumsq_final_kernel on the dense [rows, d] values (the kernel walks e = r d + c in this order)"""
    x = np.asarray(X, dtype=f32).reshape(-1)
    per = blocks * 256
    passes = ceil_div(max(x.size, 1), per)
    pad = np.zeros(passes * per, dtype=f32)
    pad[:x.size] = x
    pad = pad.reshape(passes, blocks, 256)
    s = np.zeros((blocks, 256), dtype=f32)
    for j in range(passes):
        s = fma32(pad[j], pad[j], s)

    def tree(red):
        for off in (128, 64, 32, 16, 8, 4, 2) if mutant == "no_last_step" else (128, 64, 32, 16, 8, 4, 2, 1):
            red = red.copy()
            red[..., :off] = (red[..., :off] + red[..., off:2 * off]).astype(f32)
        return red[..., 0]

    partial = tree(s)
    fin = np.zeros(256, dtype=f32)
    for i0 in range(0, blocks, 256):
        chunk = partial[i0:i0 + 256]
        fin[:chunk.size] = (fin[:chunk.size] + chunk).astype(f32)
    total = tree(fin)
    return f32((f32(0) if old is None else f32(old)) + f32(f32(coef) * total))


# ------------------------------------------------------------------------------------------------------------------------------------
# (f) inputs: seeded; rows of mixed scale, so that no per-tensor maximum can hide a row
# ------------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def row_scale(rows):
    return 2.0 ** ((np.arange(rows) % 9) - 4)


def mixed(rows, d, *key):
    """gaussians pushed away from 0 by 0.05, row r scaled by 2^(r mod 9 - 4)"""
    n = _rng(*key).standard_normal((rows, d))
    return ((n + 0.05 * np.sign(n)) * row_scale(rows)[:, None]).astype(f32)


ZERO_ROW, TINY_ROW, EQUAL_ROW, DOMINANT_ROW = 1, 3, 2, 4          # r % 16 == ...: the special rows of a table


def logits(rows, d, *key):
    """uniform in +-30 2^(r mod 9 - 8) (the widest rows span +-30), rows r % 16 == 2 of equal values, r % 16 == 4 with one dominant entry"""
    rng = _rng(*key)
    z = rng.uniform(-1.0, 1.0, (rows, d)) * (30.0 * 2.0 ** ((np.arange(rows) % 9) - 8.0))[:, None]
    r = np.arange(rows)
    z[r % 16 == EQUAL_ROW] = 7.25
    dom = np.flatnonzero(r % 16 == DOMINANT_ROW)
    z[dom] = -30.0 + 0.01 * rng.standard_normal((dom.size, d))
    z[dom, dom % d] = 30.0
    return z.astype(f32)


class Fuse(NamedTuple):
    """the operands of one fusion problem (float32 arrays [rows, d]; srcs[1] is None: a NULL source)"""
    means: tuple
    norms: tuple
    G: np.ndarray
    olds: tuple
    srcs: tuple


N_MEAN, N_NORM, N_REG = 2, 3, 2
MEAN_SCALE = float(f32(1.0 / 3.0))
RATES = tuple(float(f32(r)) for r in (0.02, 2.8, -0.005))
REG2 = float(f32(0.25))
ALPHA = float(f32(0.2))                                           # (1 / (L + 1) of the ID chain: not a power of two)


def fuse_inputs(rows, d, *key):
    """norm term 0 has exactly-zero rows (r % 16 == 1), term 1 rows of norm <= 1e-13 (r % 16 == 3); every other row's fp64 norm is >= 1e-6
    (check_fuse_split asserts it): no row sits where the fp32 norm could fall on the other side of the clamp"""
    means = tuple(mixed(rows, d, key, "mean", i) for i in range(N_MEAN))
    norms = [mixed(rows, d, key, "norm", i) for i in range(N_NORM)]
    r = np.arange(rows)
    norms[0][r % 16 == ZERO_ROW] = 0.0
    tiny = r % 16 == TINY_ROW
    n = _rng(key, "tiny").standard_normal((int(tiny.sum()), d))                    # (|n| + 0.5: the squares stay normal fp32 numbers)
    norms[1][tiny] = (np.sign(n) * (np.abs(n) + 0.5) * (1e-14 / np.sqrt(d))).astype(f32)
    G = mixed(rows, d, key, "G")
    olds = tuple(mixed(rows, d, key, "old", i) for i in range(N_NORM))
    srcs = (mixed(rows, d, key, "src", 0), None, mixed(rows, d, key, "src", 2))
    p = Fuse(means, tuple(norms), G, olds, srcs)
    check_fuse_split(p)
    return p


def check_fuse_split(p: Fuse):
    """every row of a normalised term is exactly zero, of norm <= 1e-13, or of norm >= 1e-6: nothing needs excluding from a comparison"""
    for i, x in enumerate(p.norms):
        nrm = np.sqrt((_64(x) ** 2).sum(axis=1))
        zero, tiny, live = nrm == 0.0, (nrm > 0.0) & (nrm <= 1e-13), nrm >= 1e-6
        assert (zero | tiny | live).all(), "term %d has a row between the clamp and 1e-6" % i
        r = np.arange(len(nrm))
        if i == 0:
            assert (zero == (r % 16 == ZERO_ROW)).all()
        elif i == 1:
            assert (tiny == (r % 16 == TINY_ROW)).all() and not zero.any()
        else:
            assert live.all()


def fuse_cut(p: Fuse, n):
    cut = lambda a: None if a is None else a[:n]
    return Fuse(tuple(cut(a) for a in p.means), tuple(cut(a) for a in p.norms), p.G[:n], tuple(cut(a) for a in p.olds), tuple(cut(a) for a in p.srcs))


def softmax_inputs(rows, d, *key):
    """(Z, Y, dY): Y is the float32-rounded fp64 softmax of Z - a legitimate input of the backward whatever the forward kernel does"""
    Z = logits(rows, d, key, "Z")
    Y = softmax_fwd(Z, 0)[0].astype(f32)
    return Z, Y, mixed(rows, d, key, "dY")


ADAMW = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


def adamw_inputs(n, *key):
    """(p, g, m, v) with the edge elements at the front: g = 0 with v = 0, |g| = 1e-30, |g| = 1e19 (v = 1e35, still finite in fp32 at
    beta2 = 0.999), |g| = 1e21 (v overflows: inf, update 0), a negative p"""
    rng = _rng(key, "adamw")
    p = (rng.standard_normal(n) * 0.1).astype(f32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)).astype(f32)
    m = (rng.standard_normal(n) * 0.01).astype(f32)
    v = (rng.standard_normal(n) ** 2 * 1e-4).astype(f32)
    edge = min(n, 16)
    g[:edge] = np.array([0, 0, 1e-30, -1e-30, 1e19, -1e19, 1e21, -1e21, 1, -1, 0.5, 3, 1e-3, -7, 2, 0], dtype=f32)[:edge]
    v[:4] = 0.0
    m[:2] = 0.0
    p[8:12] = -np.abs(p[8:12]) - 0.5
    return p, g, m, v


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) the case table
# ------------------------------------------------------------------------------------------------------------------------------------
D_FLOAT4 = (4, 64, 68, 128, 132, 256, 260, 512)
D_SCALAR = (1, 16, 17, 63, 65, 127, 129, 255)
# one d per NCHUNK, for the bit-exact relations. 20, 100 and 200 are multiples of 4: contiguous they are float4 shapes too (<4, 1>, <4, 2>,
# <4, 4>), so each is run a second time with ld = d + 1 on one operand, which makes it the scalar <1, 4>, <1, 8>, <1, 16>
D_RELATIONS = tuple((d, "contig") for d in (64, 128, 256, 512, 20, 100, 200)) + tuple((d, "ld1") for d in (20, 100, 200))
FORCED = ("mis_base", "ld1", "ld3")


def layout_spec(layout, d):
    """(ld, col0, base_mod16) of an operand of d columns"""
    return {"contig": (d, 0, 0), "slice": (3 * d, d, (4 * (GUARD + d)) % 16), "mis_base": (_ceil4(d + 1), 1, 4), "ld1": (d + 1, 0, 0),
            "ld3": (d + 3, 0, 0)}[layout]


_FWD = ("out",) + tuple("m%d" % i for i in range(N_MEAN)) + tuple("n%d" % i for i in range(N_NORM))
_BWD = ("dOut",) + tuple("n%d" % i for i in range(N_NORM)) + tuple("d%d" % i for i in range(N_NORM)) + ("s0", "s2")
OPERANDS = {"softmax_fwd": ("Z", "Y"), "softmax_bwd": ("Y", "dY", "dZ"), "fuse_fwd": _FWD, "fuse_bwd": _BWD,
            "fuse_fwd_multi": tuple("p%d.%s" % (k, o) for k in (0, 1) for o in _FWD),
            "fuse_bwd_src_multi": tuple("p%d.%s" % (k, o) for k in (0, 1) for o in _BWD),
            "fuse_fwd_multi_sumsq_compact": tuple("p%d.%s" % (k, o) for k in (0, 1) for o in _FWD)}
MODES = {"fuse_bwd": ("overwrite", "accumulate", "source")}


class Case(NamedTuple):
    entry: str
    d: int
    layout: str                      # contig | slice (every operand) | mis_base | ld1 | ld3 (ONE operand: `operand`)
    operand: Optional[str]
    rows: Tuple[int, ...]            # the row counts run on the same operands (problem 0 of a paired launch)
    rows1: Tuple[int, ...] = ()      # paired launches: problem 1's row count beside each of `rows`

    @property
    def name(self):
        return "%s-d%d-%s%s-r%d" % (self.entry, self.d, self.layout, "-" + self.operand if self.operand else "", max(self.rows + self.rows1))

    def spec(self, operand):
        if self.layout in ("contig", "slice"):
            return layout_spec(self.layout, self.d)
        return layout_spec(self.layout if operand == self.operand else "contig", self.d)

    def vec4(self, mode=None):
        ops = [o for o in OPERANDS[self.entry] if not (o.split(".")[-1] in ("s0", "s2") and mode in ("overwrite", "accumulate"))]
        specs = [self.spec(o) for o in ops]
        return vec4_of(self.d, [s[0] for s in specs], [s[2] for s in specs])

    def expect(self, mode=None):
        """(VEC, NCHUNK) or None (LLMREC_EUNSUPPORTED)"""
        v = self.vec4(mode)
        if self.entry == "fuse_fwd_multi_sumsq_compact" and not v:
            return None
        return instance(self.d, v)


def _paired(entry):
    return entry in ("fuse_fwd_multi", "fuse_bwd_src_multi", "fuse_fwd_multi_sumsq_compact")


def _rows(entry, rows):
    return dict(rows=rows, rows1=tuple(37 for _ in rows) if _paired(entry) else ())


def cases():
    out = []
    for entry in TEMPLATED:
        ops = OPERANDS[entry]
        for d in D_FLOAT4 + D_SCALAR:                                              # every instance, contiguous
            out.append(Case(entry, d, "contig", None, **_rows(entry, SMALL_ROWS)))
        out.append(Case(entry, 16, "ld1", ops[0], **_rows(entry, SMALL_ROWS)))     # d = 16 in the scalar family: <1, 1> with every lane live
        k = 0
        for d in (64, 128):                                                        # the scalar path forced, one operand and one clause at a time
            for way in FORCED:
                out.append(Case(entry, d, way, ops[(k * 5 + len(entry)) % len(ops)], **_rows(entry, SMALL_ROWS)))
                k += 1
        for d in (64, 128, 256, 512):                                              # strided float4: the middle third of [rows, 3 d]
            out.append(Case(entry, d, "slice", None, **_rows(entry, SMALL_ROWS)))
        # a second pass of the sweep, float4 and scalar. (An aligned, contiguous d = 20 is a float4 shape - <4, 1> - so the scalar sweep
        # <1, 4> is d = 20 with ld = 21 on one operand.)
        for d, layout, operand in ((64, "contig", None), (20, "ld1", ops[0])):
            if _paired(entry):
                out.append(Case(entry, d, layout, operand, rows=(BIG_ROWS,), rows1=(37,)))
                out.append(Case(entry, d, layout, operand, rows=(37,), rows1=(BIG_ROWS,)))
            else:
                out.append(Case(entry, d, layout, operand, rows=(BIG_ROWS,)))
    return out


def refusals():
    out = []
    for entry in TEMPLATED:
        out.append(Case(entry, 516, "contig", None, **_rows(entry, (17,))))
        out.append(Case(entry, 257, "contig", None, **_rows(entry, (17,))))
        out.append(Case(entry, 260, "mis_base", OPERANDS[entry][1], **_rows(entry, (17,))))
    out.append(Case("fuse_fwd_multi_sumsq_compact", 64, "mis_base", "p1.n1", **_rows("fuse_fwd_multi_sumsq_compact", (17,))))
    return out


class GroupCase(NamedTuple):
    """llmrec_step_rows_group_f32: the fusion member (two problems), an AdamW member, the softmax member; d = 64 (<4, 1> only)"""
    name: str
    fuse_rows: Tuple[int, int]
    sm_rows: int
    adamw_n: Tuple[int, ...]


def group_cases():
    return [GroupCase("small", (67, 37), 17, (1000, 2048 + 5)),
            GroupCase("big-fusion", (BIG_ROWS, 37), 67, (1000,)),
            GroupCase("big-softmax", (67, 37), BIG_ROWS, (1000,))]


class FlatCase(NamedTuple):
    entry: str                       # sumsq | axpy | adamw | scale_rows | gather_mean | weighted_colsum
    rows: int
    d: int
    ld: int


def _factor(n, lo):
    d = lo
    while n % d:
        d += 1
    return d


def flat_cases():
    d_big = _factor(FLAT_BIG, 3)                                                   # rows d = 2^21 + 777 exactly
    return [FlatCase("sumsq", 50, 20, 23), FlatCase("sumsq", FLAT_BIG // d_big, d_big, d_big + 5),
            FlatCase("axpy", 50, 20, 20), FlatCase("axpy", 1, FLAT_BIG, FLAT_BIG),
            FlatCase("adamw", 1, 1000, 1000), FlatCase("adamw", 1, FLAT_BIG, FLAT_BIG),
            FlatCase("scale_rows", 50, 20, 23), FlatCase("scale_rows", BIG_ROWS, 64, 64),
            FlatCase("gather_mean", 67, 20, 23), FlatCase("gather_mean", 67, 64, 64),
            FlatCase("weighted_colsum", 300, 3 * 64, 3 * 64 + 4), FlatCase("weighted_colsum", 7, 2 * 20, 41)]
