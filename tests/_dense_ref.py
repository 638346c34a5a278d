"""float64 reference, the dispatch rules restated, per-element thresholds and the case table of the projection and weight-gradient
kernels (llmrec_amd/csrc/dense.hip). NumPy only: no device, no torch, nothing from llmrec_amd. Used by tests/test_dense_ref_cpu.py (the
yardstick is sound, not vacuous, sees a defect, and the table reaches every instantiation) and tests/test_gpu_dense_families.py.

The operations:  Y = X W^T + bias_scale . b     dW (+)= sum_p dY_p^T X_p     db (+)= sum_p sum_r w_p[r] dY_p[r]

DISPATCH, restated from the host code of dense.hip (the quoted fragments locate each rule should the lines drift):
  llmrec_linear_fwd_f32          "const int NT = (N + 15) / 16;"  "const bool rows_mode = M >= 32 * 2048;"  and the switch
                                 "case 4: if (rows_mode) LAUNCH_ROWS(4, 2)" / "case 5: if (rows_mode) LAUNCH_ROWS(5, 1)": RT = 2 up to NT = 4
                                 in row mode, else 1; split-K is always <NT, 1, true>.                                   -> fwd_plain()
  linear_fwd_grouped_impl        "const int rows_per_unit = units128 >= 256 ? 128 : 64;"
                                 "fast = fast && g.vec_ok[i] && (g.K[i] % 4 == 0) && g.K[i] >= 4;"
                                 "k32 = k32 && (g.K[i] % 32 == 0) && (p[i].M * p[i].ldx + g.K[i]) < (1ll << 30) && ((int64_t)N * p[i].ldw + ..."
                                 "#define K32MODE 3" (bf16x3) / "#define K32MODE 2" (fp32); vec_ok = ldx % 4 == 0, ldw % 4 == 0, X | W
                                 16-byte aligned. One problem outside a rule turns the whole launch.                     -> fwd_grouped()
  linear_wgrad_grouped_impl      "bool fast_shape = (N % 64 == 0) && (K % 64 == 0);"  (+ lddy % 4, ldx % 4, dY | X aligned, every problem)
                                 "small_offsets && (p[i].M + 256) * std::max(p[i].lddy, p[i].ldx) < (1ll << 30)"
                                 "if (use_bf16 && N == 64 && K % W2_KW == 0)" + every M > 0: handed to the multi launch as one target
                                 "MC = use_bf16 ? wgrad_slab_rows_bf16(...) : wgrad_slab_rows(M_total, K, false)"         -> wgrad_grouped()
  wgrad_slab_rows                "align_up(ceil_div(M_total > 0 ? M_total : 1, want_slabs), bf16x3 ? 64 : 48)", "(!bf16x3 && mc < 144) ? 144"
  wgrad_slab_rows_bf16           "lo = std::max<int64_t>(64, align_up(wgrad_slab_rows(M_total, K, true) / 2, 32))", "cost <= best_cost"
  llmrec_linear_wgrad_workspace_bytes   "std::min(wgrad_slab_rows(M, K, false), wgrad_slab_rows(M, K, true))", "+ LLMREC_LINEAR_MAX_PROBLEMS"
  wgrad_rows_eff / wgrad_multi_version / wgrad_multi_slab_rows / wgrad_multi_ok / llmrec_linear_wgrad_multi_workspace_bytes
                                 "if (!q.row_list || q.rows_expected <= 0) return q.M;"  "if (t[i].K % W2_KW) return 1;"
                                 "lo = std::max<int64_t>(64, align_up(ceil_div(work, 4 * 2 * budget), 32))"
                                 "if (q.row_list && (!q.n_rows || t[i].K % W2_KW || ..."                                 -> the same names here

REFERENCES
  y64 / dw64 / db64   the fp64 values; s_fwd / s_dw / s_db the same expressions over absolute values (the magnitude sums S).
  chain()             the fp32 forward kernels' contract: acc = fmaf(x[k], w[k], acc) over k in the order
                      for c, for s in 0..3, for q in 0..3: k = 16 c + 4 q + s  (oracle.scores_fma_chain(order="mfma16x16x4")). fma32()
                      closes that function's double rounding: the product of two fp32 numbers is exact in fp64, s = fl64(p + c) is rounded
                      to fp32, and where s sits exactly half-way between two fp32 numbers (the 29 dropped bits are 1000...0) the TwoSum
                      residual of p + c decides the direction. (Only there can rounding twice differ from rounding once.)
  chain_splitk()      linear_fwd_kernel<NT, 1, true>: four chains over [w kq, min(K, (w + 1) kq)), kq = ceil(ceil(K / 4) / 16) * 16 (a
                      multiple of 16, so every wave visits its k's in the same order), then ((p0 + p1) + p2) + p3, then + b.
                      Row mode and the grouped kernel: fl(chain + b) (fmaf(1, b, chain) is the same number), or fmaf(bias_scale[r], b, chain).
  split3()            dense.hip "r.h = __float_as_uint(x) & 0xffff0000u;" : mask, exact subtract, mask, exact subtract.
  y6 / dw6            the ideal value of the six kept products hh, hm, mh, mm, hl, lh (first letter: the X / dY term), summed in fp64.

THRESHOLDS (u = 2^-24)
  fp32 forward        bit for bit the chain.
  fp32 gradient       |err| <= (n + 6) u S, n = the rows summed. Every term x y passes one rounding when its fma adds it and one per later
                      addition it takes part in: at most m (the rows of its slab) in the slab's chain, then ceil(c / 4) + 2 in the
                      reduction over the c partial slabs (four interleaved sums, "(s0 + s1) + (s2 + s3)"), then one for accumulate. Every
                      slab but the term's own holds at least one row, so m <= n - (c - 1), and the depth is at most
                      n - (c - 1) + ceil(c / 4) + 3 <= n + 4. To first order the error is depth u S; the second-order terms
                      ((n + 4)^2 u^2 / 2 S) stay below 2 u S up to n = 8000. db is the same sum with n + 2 shuffle additions less chain:
                      the same bound holds (bf16x3 kernels sum db in plain fp32 too). S includes |old| when accumulating.
  bf16x3              |dev - Y6| <= T_ACC S  and  |dev - Y64| <= (2^-20 (1 + 2^-6) + T_ACC) S.
                      The split truncates: h = x cut to 8 significant bits, so r1 = x - h has |r1| < 2^-7 |x|; m = r1 cut to 8 bits, so
                      |m| <= |r1| < 2^-7 |x| and l = r1 - m has |l| < 2^-7 |r1| < 2^-14 |x|; |h| <= |x|. The dropped products are m l, l m
                      and l l: |x w - six terms| < (2^-21 + 2^-21 + 2^-28) |x w| = 2^-20 (1 + 2^-8) |x w|; summed over k that is
                      2^-20 (1 + 2^-8) S <= 2^-20 (1 + 2^-6) S (the bias term is not split). For the gradient the operands are dY and X.
                      T_ACC covers the fp32 accumulation inside and between the bf16 MFMAs, whose number of roundings no document states.
                      It is NOT fitted to the device: emulate() adds the six terms' products one by one, rounding to fp32 after every
                      single product (the hardware cannot round more often), in four summation orders; T_ACC[class] = 4 x the worst
                      |emulation - Y6| / S over the class's precision cases (tests/test_dense_ref_cpu.py re-measures and asserts
                      emulation <= T_ACC / 4). The 4 stands for the orders not tried. profiles/experiments/r13_dense_families.md has the
                      measurement.
  Operands stay within 2^-30 .. 2^30 in magnitude (or are exactly +-0): no split term or product leaves the normal range. Subnormal and
  non-finite operands are out of scope (dense.hip: "past K the staged W tile is zero and X is finite" is a precondition).
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

U = 2.0 ** -24
DROPPED = 2.0 ** -20 * (1 + 2.0 ** -6)
MAX_PROBLEMS, MAX_TARGETS, W2_KW = 8, 4, 128          # LLMREC_LINEAR_MAX_PROBLEMS, LLMREC_WGRAD_MAX_TARGETS, W2_KW
SENTINEL = 12345.0                                    # what an output and its surroundings hold before a call
PRECISION_DEPTH = 8
PERIOD = 257                                          # the rows of a long operand repeat with this period (prime: no tile length divides it)
# 4 x the worst |emulation - Y6| / S over the class's precision cases (measured on the CPU, see the header)
T_ACC = {"fwd": 4 * 4.30e-7, "wgrad": 4 * 4.78e-7}
TERMS = ("lh", "hl", "mm", "mh", "hm", "hh")          # the kernels' order, smallest first; first letter = X (forward) / dY (gradient)


def ceil_div(a, b):
    return -(-a // b)


def align_up(a, b):
    return ceil_div(a, b) * b


# ------------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------------------
class FwdP(NamedTuple):          # one problem of a forward launch
    M: int
    K: int
    ldx: int
    ldw: int
    xmod: int = 0                # X's base address % 16
    wmod: int = 0


class WgP(NamedTuple):           # one problem of a weight-gradient launch
    M: int
    lddy: int
    ldx: int
    ymod: int = 0
    xmod: int = 0
    listed: bool = False
    rows_expected: int = 0
    has_n_rows: bool = True
    list_mod64: int = 0
    weighted: bool = False       # db_row_weight


class WgT(NamedTuple):           # one target of a multi-target launch
    K: int
    lddw: int
    problems: Tuple[WgP, ...]
    db: bool = True
    accumulate: bool = False


def fwd_plain(M, N, K):
    """llmrec_linear_fwd_f32 -> ("linear_fwd_kernel", NT, RT, SPLITK) or None (refused: N > 128)"""
    if N > 128:
        return None
    NT = ceil_div(N, 16)
    rows_mode = M >= 32 * 2048
    return ("linear_fwd_kernel", NT, (2 if NT <= 4 else 1) if rows_mode else 1, not rows_mode)


def fwd_grouped(problems, N, precision):
    """linear_fwd_grouped_impl -> (kernel, NT, RT, MODE); None: refused (N > 64) or nothing to launch"""
    if N > 64:
        return None
    units128 = sum(ceil_div(p.M, 128) for p in problems)
    rows_per_unit = 128 if units128 >= 256 else 64
    if sum(ceil_div(p.M, rows_per_unit) for p in problems) == 0:
        return None
    vec_ok = [p.ldx % 4 == 0 and p.ldw % 4 == 0 and p.xmod == 0 and p.wmod == 0 for p in problems]
    fast = all(v and p.K % 4 == 0 and p.K >= 4 for v, p in zip(vec_ok, problems))
    k32 = fast and all(p.K % 32 == 0 and p.M * p.ldx + p.K < (1 << 30) and N * p.ldw + p.K < (1 << 30) for p in problems)
    bf = precision == "bf16x3"
    mode = (3 if bf else 2) if k32 else (1 if fast else 0)
    return ("linear_fwd_grouped_bf16x3_kernel" if bf else "linear_fwd_grouped_kernel", ceil_div(N, 16), rows_per_unit // 64, mode)


def wgrad_slab_rows(M_total, K, bf16x3):
    want_slabs = ceil_div(2048, ceil_div(K, 64))
    mc = align_up(ceil_div(M_total if M_total > 0 else 1, want_slabs), 64 if bf16x3 else 48)
    return 144 if (not bf16x3 and mc < 144) else mc


def wgrad_slab_rows_bf16(Ms, M_total, K):
    n_kslab = ceil_div(K, 64)
    lo = max(64, align_up(wgrad_slab_rows(M_total, K, True) // 2, 32))
    best, best_cost = lo, -1
    for mc in range(lo, align_up(max(Ms), 32) + 32 + 1, 32):
        blocks = ceil_div(sum(ceil_div(m, mc) for m in Ms), 4) * n_kslab
        cost = ceil_div(blocks, 256) * (mc + 96)
        if best_cost < 0 or cost <= best_cost:
            best, best_cost = mc, cost
    return best


def wgrad_ws_bytes(n_slabs, N, K):
    return align_up(4 * n_slabs * N * K, 256) + align_up(4 * n_slabs * N, 256)


def wgrad_workspace_bytes(M, N, K):
    """llmrec_linear_wgrad_workspace_bytes"""
    if M < 0 or N <= 0 or K <= 0:
        return -1
    mc = min(wgrad_slab_rows(M, K, False), wgrad_slab_rows(M, K, True))
    return wgrad_ws_bytes(ceil_div(M if M > 0 else 1, mc) + MAX_PROBLEMS, N, K)


def wgrad_rows_eff(q: WgP):
    if not q.listed or q.rows_expected <= 0:
        return q.M
    return min(q.M, max(q.rows_expected, 16))


def wgrad_multi_version(targets):
    return 1 if any(t.K % W2_KW for t in targets) else 2


def wgrad_multi_slab_rows(targets, block_budget=0):
    kw = 64 if wgrad_multi_version(targets) == 1 else W2_KW
    budget = block_budget if 0 < block_budget <= 256 else 256
    eff = [[wgrad_rows_eff(q) for q in t.problems] for t in targets]
    m_max = max(max(e) for e in eff)
    work = sum(sum(e) * ceil_div(t.K, kw) for e, t in zip(eff, targets))
    lo = max(64, align_up(ceil_div(work, 4 * 2 * budget), 32))
    best, best_cost = lo, -1
    for mc in range(lo, align_up(m_max, 32) + 32 + 1, 32):
        blocks = sum(ceil_div(sum(ceil_div(m, mc) for m in e), 4) * ceil_div(t.K, kw) for e, t in zip(eff, targets))
        cost = ceil_div(blocks, budget) * (mc + 96)
        if best_cost < 0 or cost <= best_cost:
            best, best_cost = mc, cost
    return best


def wgrad_multi_ok(targets, N):
    """the clause that refuses (a short name), or None when the launch is inside the fast path"""
    if not 1 <= len(targets) <= MAX_TARGETS:
        return "n_targets"
    if N <= 0 or N % 64:
        return "N % 64"
    for t in targets:
        if not 1 <= len(t.problems) <= MAX_PROBLEMS:
            return "n_problems"
        if t.K <= 0 or t.K % 64:
            return "K % 64"
        if t.lddw < t.K:
            return "lddw < K"
        for q in t.problems:
            if q.M <= 0:
                return "M <= 0"
            if q.lddy < N or q.ldx < t.K:
                return "ld too small"
            if q.lddy % 4 or q.ldx % 4 or q.ymod or q.xmod:
                return "alignment"
            if (q.M + 256) * max(q.lddy, q.ldx) >= (1 << 30):
                return "offsets"
            if q.listed and not q.has_n_rows:
                return "list without n_rows"
            if q.listed and t.K % W2_KW:
                return "list with K % 128"
            if q.listed and q.M * max(q.lddy, q.ldx) * 4 >= (1 << 31):
                return "list offsets"
            if q.listed and q.list_mod64:
                return "list alignment"
    return None


def wgrad_multi(targets, N, block_budget=0):
    """linear_wgrad_multi_impl -> dict(kernel, reduce, MC, n_chunks per target, bytes) or None (refused; the row-list / row-weight refusals of
    organisation 1 included)"""
    if wgrad_multi_ok(targets, N) is not None:
        return None
    version = wgrad_multi_version(targets)
    if version == 1 and any(q.listed or q.weighted for t in targets for q in t.problems):
        return None
    mc = wgrad_multi_slab_rows(targets, block_budget)
    chunks = [ceil_div(sum(ceil_div(wgrad_rows_eff(q), mc) for q in t.problems), 4) for t in targets]
    kernels = set()
    if version == 1:
        kernels.add("linear_wgrad_bf16x3_multi_kernel")
    else:
        for t in targets:
            for q in t.problems:
                kernels.add("linear_wgrad_bf16x3_v2_multi_kernel/" + ("listed" if q.listed else "dense"))
    red = {"reduce_chunks_multi_kernel<false>/acc%d/%s" % (t.accumulate, "db" if t.db else "nodb") for t in targets}
    return dict(kernels=kernels, reduce=red, MC=mc, n_chunks=chunks, grid_y=N // 64,
                bytes=sum(wgrad_ws_bytes(c, N, t.K) for c, t in zip(chunks, targets)))


def wgrad_multi_workspace_bytes(targets, N, block_budget=0):
    """llmrec_linear_wgrad_multi_workspace_bytes (the organisation-1 refusals come from the launch, not from this query)"""
    if wgrad_multi_ok(targets, N) is not None:
        return -1
    mc = wgrad_multi_slab_rows(targets, block_budget)
    return sum(wgrad_ws_bytes(ceil_div(sum(ceil_div(wgrad_rows_eff(q), mc) for q in t.problems), 4), N, t.K) for t in targets)


def wgrad_grouped(problems, N, K, precision, db=True, accumulate=False, lddw=None):
    """linear_wgrad_grouped_impl -> dict(kernels, reduce, MC, n_slabs, n_chunks, bytes, bound)"""
    M_total = sum(p.M for p in problems)
    bound = wgrad_workspace_bytes(M_total, N, K)
    if M_total == 0:
        return dict(kernels={"memset"}, reduce=set(), MC=0, n_slabs=0, n_chunks=0, bytes=0, bound=bound)
    aligned = all(p.lddy % 4 == 0 and p.ldx % 4 == 0 and p.ymod == 0 and p.xmod == 0 for p in problems)
    fast_shape = N % 64 == 0 and K % 64 == 0 and aligned
    small = all((p.M + 256) * max(p.lddy, p.ldx) < (1 << 30) for p in problems)
    use_bf16 = precision == "bf16x3" and fast_shape and small
    if use_bf16 and N == 64 and K % W2_KW == 0 and all(p.M > 0 for p in problems):
        out = wgrad_multi((WgT(K, lddw or K, tuple(problems), db, accumulate),), N)
        if out is not None:
            out["bound"] = bound
        return out
    if any(p.weighted or p.listed for p in problems):
        return None
    MC = wgrad_slab_rows_bf16([p.M for p in problems], M_total, K) if use_bf16 else wgrad_slab_rows(M_total, K, False)
    n_slabs = sum(ceil_div(p.M, MC) for p in problems)
    if use_bf16:
        kernel, n_chunks = "linear_wgrad_bf16x3_kernel", ceil_div(n_slabs, 4)
    else:
        kernel, n_chunks = "linear_wgrad_kernel<%s>" % ("true" if fast_shape else "false"), n_slabs
    return dict(kernels={kernel}, reduce={"reduce_chunks_kernel/acc%d/%s" % (accumulate, "db" if db else "nodb")}, MC=MC, n_slabs=n_slabs,
                n_chunks=n_chunks, grid_y=ceil_div(N, 64), bytes=wgrad_ws_bytes(n_slabs, N, K), bound=bound)


# every instantiation the host can launch
ALL_FWD_PLAIN = {("linear_fwd_kernel", nt, (2 if nt <= 4 else 1) if rows else 1, not rows) for nt in range(1, 9) for rows in (False, True)}
ALL_FWD_GROUPED = {(k, nt, rt, m) for k, modes in (("linear_fwd_grouped_kernel", (0, 1, 2)), ("linear_fwd_grouped_bf16x3_kernel", (0, 1, 3)))
                   for nt in range(1, 5) for rt in (1, 2) for m in modes}
ALL_WGRAD = {"linear_wgrad_kernel<true>", "linear_wgrad_kernel<false>", "linear_wgrad_bf16x3_kernel", "linear_wgrad_bf16x3_multi_kernel",
             "linear_wgrad_bf16x3_v2_multi_kernel/dense", "linear_wgrad_bf16x3_v2_multi_kernel/listed"}
ALL_REDUCE = ({"reduce_chunks_kernel/acc%d/%s" % (a, d) for a in (0, 1) for d in ("db", "nodb")}
              | {"reduce_chunks_multi_kernel<false>/acc%d/%s" % (a, d) for a in (0, 1) for d in ("db", "nodb")}
              | {"reduce_chunks_multi_kernel<true>/acc0/db", "reduce_chunks_multi_kernel<true>/acc0/nodb"})


# ------------------------------------------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c), one rounding (a, b, c float32 arrays that broadcast)"""
    p = a.astype(np.float64) * b.astype(np.float64)              # exact: 24 x 24 bits
    c64 = c.astype(np.float64)
    s = p + c64
    r = s.astype(np.float32)
    tie = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    if tie.any():
        p, c64 = np.broadcast_to(p, s.shape)[tie], np.broadcast_to(c64, s.shape)[tie]
        st = s[tie]
        bb = st - p
        err = (p - (st - bb)) + (c64 - bb)                       # TwoSum: p + c == s + err exactly
        rt = r[tie]
        up = np.where(rt.astype(np.float64) > st, rt, np.nextafter(rt, np.float32(np.inf)))
        dn = np.where(rt.astype(np.float64) > st, np.nextafter(rt, np.float32(-np.inf)), rt)
        r[tie] = np.where(err > 0, up, np.where(err < 0, dn, rt))
    a_s = np.abs(s)
    assert not ((a_s > 0) & (a_s < 2.0 ** -126)).any() and np.isfinite(s).all(), "outside the normal fp32 range"
    return r


def chain_order(k_begin, k_end):
    return [k for c in range(k_begin // 16, ceil_div(max(k_end, k_begin), 16)) for s in range(4) for q in range(4)
            for k in (16 * c + 4 * q + s,) if k_begin <= k < k_end]


def chain(X, W, k_begin=0, k_end=None, block=2048):
    """float32 [M, N]: the fma chain over k in [k_begin, k_end) in the order of v_mfma_f32_16x16x4_f32's users in dense.hip"""
    X, W = np.asarray(X, dtype=np.float32), np.asarray(W, dtype=np.float32)
    k_end = X.shape[1] if k_end is None else k_end
    out = np.zeros((X.shape[0], W.shape[0]), dtype=np.float32)
    ks = chain_order(k_begin, k_end)
    for r0 in range(0, X.shape[0], block):                       # row blocks: the working set stays in the cache
        acc = out[r0:r0 + block]
        for k in ks:
            acc = fma32(X[r0:r0 + block, k:k + 1], W[None, :, k], acc)
        out[r0:r0 + block] = acc
    return out


def chain_fwd(X, W, b=None, bias_scale=None, splitk=False):
    """what the fp32 forward kernels return, bit for bit"""
    X, W = np.asarray(X, dtype=np.float32), np.asarray(W, dtype=np.float32)
    M, K = X.shape
    bv = np.zeros(W.shape[0], dtype=np.float32) if b is None else np.asarray(b, dtype=np.float32)
    if splitk:
        assert bias_scale is None
        kq = ceil_div(ceil_div(K, 4), 16) * 16
        p = [chain(X, W, w * kq, min(K, (w + 1) * kq)) for w in range(4)]
        return (((p[0] + p[1]) + p[2]) + p[3]) + bv[None, :]
    acc = chain(X, W)
    if bias_scale is None or b is None:
        return acc + bv[None, :]
    return fma32(np.asarray(bias_scale, dtype=np.float32)[:, None], bv[None, :], acc)


def split3(x):
    """(h, m, l) float32: dense.hip's split3 - mask, exact subtract, mask, exact subtract; h + m + l == x"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    mask = np.uint32(0xffff0000)
    h = (x.view(np.uint32) & mask).view(np.float32)
    r1 = x - h
    m = (r1.view(np.uint32) & mask).view(np.float32)
    r2 = r1 - m
    l = (r2.view(np.uint32) & mask).view(np.float32)             # the pack keeps the high half; r2 has <= 8 significant bits
    return h, m, l


def _terms(a, b):
    sa, sb = dict(zip("hml", split3(a))), dict(zip("hml", split3(b)))
    return [(sa[t[0]], sb[t[1]]) for t in TERMS]


def _bias64(M, N, b, bias_scale):
    if b is None:
        return np.zeros((M, N))
    bs = np.ones(M) if bias_scale is None else np.asarray(bias_scale, dtype=np.float64)
    return bs[:, None] * np.asarray(b, dtype=np.float64)[None, :]


def y64(X, W, b=None, bias_scale=None):
    return np.asarray(X, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + _bias64(X.shape[0], W.shape[0], b, bias_scale)


def s_fwd(X, W, b=None, bias_scale=None):
    return np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(np.asarray(W, dtype=np.float64)).T + np.abs(_bias64(X.shape[0], W.shape[0], b, bias_scale))


def y6(X, W, b=None, bias_scale=None):
    return sum(a.astype(np.float64) @ w.astype(np.float64).T for a, w in _terms(X, W)) + _bias64(X.shape[0], W.shape[0], b, bias_scale)


def dw64(pairs, old=None):
    """pairs: [(dY [M, N], X [M, K])] float32 (the LISTED rows only for a listed problem)"""
    out = sum(np.asarray(dy, dtype=np.float64).T @ np.asarray(x, dtype=np.float64) for dy, x in pairs)
    return out if old is None else out + np.asarray(old, dtype=np.float64)


def s_dw(pairs, old=None):
    out = sum(np.abs(np.asarray(dy, dtype=np.float64)).T @ np.abs(np.asarray(x, dtype=np.float64)) for dy, x in pairs)
    return out if old is None else out + np.abs(np.asarray(old, dtype=np.float64))


def dw6(pairs, old=None):
    out = sum(a.astype(np.float64).T @ x.astype(np.float64) for dy, xx in pairs for a, x in _terms(dy, xx))
    return out if old is None else out + np.asarray(old, dtype=np.float64)


def db64(dys, weights=None, old=None, absolute=False):
    """dys: [dY [M, N]]; weights: [w [M] or None]"""
    f = np.abs if absolute else (lambda v: v)
    out = 0.0
    for i, dy in enumerate(dys):
        w = None if weights is None else weights[i]
        d = f(np.asarray(dy, dtype=np.float64))
        out = out + (d if w is None else d * f(np.asarray(w, dtype=np.float64))[:, None]).sum(0)
    return out if old is None else out + f(np.asarray(old, dtype=np.float64))


def bound_f32(n_rows):
    return (n_rows + 6) * U


# ------------------------------------------------------------------------------------------------------------------------------------
# the per-product emulation of the bf16x3 kernels and its mutants (CPU only: the yardstick's yardstick)
# ------------------------------------------------------------------------------------------------------------------------------------
def _positions(n, order, step):
    """the contraction positions of one `step`-long MFMA step after the other, inside a step in the given order"""
    out = []
    for p0 in range(0, n, step):
        ks = list(range(p0, min(n, p0 + step)))
        if order == 1:
            ks = ks[::-1]
        elif order >= 2:
            ks = [ks[i] for i in np.random.default_rng(order).permutation(len(ks))]
        out.append(ks)
    return out


def emulate(A, B, order=0, step=32, add=None, mutant=None):
    """float32 [A.shape[1], B.shape[1]] = sum over the contraction index (axis 0 of both) of the six kept products of A[r, :] (x) B[r, :],
    every product added to the fp32 accumulator with its own rounding (the products themselves are exact: 8 x 8 bits). Orders: 0 = the
    kernels' (per step: term by term, positions ascending), 1 = positions descending, 2 / 3 = two random orders of positions AND terms.
    add = (float32 [n_a] scale, float32 [n_b] vector): the forward's closing fmaf(scale, vector, acc) / the plain bias addition.
    mutant: ("lost", term, j) the term's products at positions p % 8 == j are dropped;  ("swap", "A" | "B") m and l of one operand change
    places;  ("dup", i) row i of every 16-row output tile repeats row i - 1;  ("bias2",) the closing addition happens twice."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    sa, sb = dict(zip("hml", split3(A))), dict(zip("hml", split3(B)))
    if mutant and mutant[0] == "swap":
        s_ = sa if mutant[1] == "A" else sb
        s_["m"], s_["l"] = s_["l"], s_["m"]
    acc = np.zeros((A.shape[1], B.shape[1]), dtype=np.float32)
    for ks in _positions(A.shape[0], order, step):
        todo = [(t, k) for t in TERMS for k in ks]
        if order >= 2:
            todo = [todo[i] for i in np.random.default_rng(order + 7).permutation(len(todo))]
        for t, k in todo:
            if mutant and mutant[0] == "lost" and t == mutant[1] and k % 8 == mutant[2]:
                continue
            acc = acc + sa[t[0]][k][:, None] * sb[t[1]][k][None, :]          # float32: the product is exact, the sum rounds once
    if mutant and mutant[0] == "dup":
        rows = np.arange(mutant[1], acc.shape[0], 16)
        acc[rows] = acc[rows - 1]
    if add is not None:
        for _ in range(2 if (mutant and mutant[0] == "bias2") else 1):
            acc = fma32(add[0][:, None], add[1][None, :], acc)
    return acc


# ------------------------------------------------------------------------------------------------------------------------------------
# values and layouts
# ------------------------------------------------------------------------------------------------------------------------------------
VALUE_CLASSES = ("gauss", "positive", "scaled", "low16clear", "full24", "zeros", "negzero")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def values(cls, shape, *key, scale=1.0):
    """float32 values of one class; magnitudes within 2^-30 .. 2^30 or exactly zero"""
    rng = _rng(cls, shape, key)
    g = rng.standard_normal(shape)
    g = np.sign(g) * np.clip(np.abs(g), 2.0 ** -8, 8.0) * scale
    if cls == "gauss":
        v = g
    elif cls == "positive":
        v = np.abs(g)
    elif cls == "scaled":
        v = g * 2.0 ** rng.integers(-20, 21, size=shape)
        v = np.sign(v) * np.clip(np.abs(v), 2.0 ** -30, 2.0 ** 30)
    elif cls == "low16clear":                                     # m = l = 0
        v = (g.astype(np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    elif cls == "full24":                                         # all 24 significand bits set
        v = np.sign(g) * (2.0 - 2.0 ** -23) * 2.0 ** rng.integers(-3, 3, size=shape) * scale
    elif cls == "zeros":                                          # exact zeros as whole rows and columns
        v = g.copy()
        v[::3] = 0.0
        if len(shape) == 2:
            v[:, 1::4] = 0.0
    elif cls == "negzero":
        v = g.copy()
        v[rng.random(shape) < 0.3] = -0.0
        v[1::5] = -0.0
    else:
        raise ValueError(cls)
    v = np.ascontiguousarray(v, dtype=np.float32)
    a = np.abs(v[v != 0])
    assert a.size == 0 or (a.min() >= 2.0 ** -30 and a.max() <= 2.0 ** 30)
    return v


def long_rows(cls, M, d, *key, scale=1.0):
    """[M, d] whose rows repeat with period PERIOD: a reference over PERIOD rows states all of them"""
    base = values(cls, (min(M, PERIOD), d), *key, scale=scale)
    return base[np.arange(M) % PERIOD] if M > PERIOD else base


def layout_spec(name, d):
    """(ld, col0, base % 16) of tests._eval_ref.layouts(d)[name]"""
    c4 = lambda x: (x + 3) // 4 * 4
    return {"contig": (d, 0, 0), "padded": (c4(d) + 4, 0, 0), "odd_ld": (d + 1 if (d + 1) % 4 else d + 2, 0, 0),
            "shifted": (c4(d + 1), 1, 4)}[name]


LAYOUTS = ("contig", "padded", "odd_ld", "shifted")


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
class PlainCase(NamedTuple):
    name: str
    M: int
    N: int
    K: int
    xl: str
    wl: str
    bias: bool
    cls: str
    expect: tuple


def plain_cases():
    out = []
    Ns = (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)
    Ks, Ms = (1, 16, 17, 64, 65, 100), (1, 15, 16, 17, 33)
    for i, N in enumerate(Ns):                                    # split-K: every NT with both of its N, every K and M at least twice
        M, K = Ms[i % 5], Ks[(i + i // 6) % 6]
        out.append(PlainCase("splitk%d" % i, M, N, K, LAYOUTS[i % 4], LAYOUTS[(i // 4) % 4], i % 3 != 0, VALUE_CLASSES[i % 7],
                             ("linear_fwd_kernel", ceil_div(N, 16), 1, True)))
    for nt in range(1, 9):                                        # row mode: each NT at an N that is no multiple of 16
        N = 16 * (nt - 1) + 5
        out.append(PlainCase("rows%d" % nt, 65573, N, 20 + nt % 2, LAYOUTS[nt % 4], LAYOUTS[(nt + 1) % 4], nt % 2 == 0, VALUE_CLASSES[nt % 7],
                             ("linear_fwd_kernel", nt, 2 if nt <= 4 else 1, False)))
    out.append(PlainCase("rows_exact", 65536, 64, 4, "contig", "contig", True, "gauss", ("linear_fwd_kernel", 4, 2, False)))
    for c in out:
        assert fwd_plain(c.M, c.N, c.K) == c.expect, c
    return out


def plain_inputs(c: PlainCase):
    X = long_rows(c.cls, c.M, c.K, c.name, "X")
    W = values(c.cls, (c.N, c.K), c.name, "W", scale=0.25)
    b = values("gauss", (c.N,), c.name, "b") if c.bias else None
    return X, W, b


class GJob(NamedTuple):          # one problem of a grouped forward launch
    M: int
    K: int
    xl: str
    wl: str
    bias: str                    # "none" | "bias" | "scale"
    y_slice: bool                # Y is a column slice of a wider buffer
    cls: str


class GroupedCase(NamedTuple):
    name: str
    N: int
    rt: int
    mode: int                    # 0, 1, or 2 (= the k32 mode: 2 in fp32, 3 in bf16x3)
    jobs: Tuple[GJob, ...]


GROUPED_N = (5, 16, 17, 32, 40, 48, 49, 64)
FILLER_M = 255 * 128 + 1


def grouped_cases():
    """one launch per (N, 64 / 128-row units, mode); the seven small problems of a (N, mode) are the same in both unit sizes, so their
    results can be compared bit for bit"""
    out = []
    Ms = (0, 1, 63, 64, 65, 129, 300)
    for ni, N in enumerate(GROUPED_N):
        for mode in (0, 1, 2):
            Ks = {0: (5, 36, 100, 33, 4, 36, 100), 1: (4, 36, 100, 36, 100, 4, 36), 2: (32, 96, 128, 32, 96, 128, 32)}[mode]
            jobs = []
            for j, M in enumerate(Ms):
                xl, wl = ("contig", "padded")[(j + ni) % 2], ("contig", "padded")[(j // 2 + ni) % 2]     # padded W: ldw > K
                if mode == 0:                                     # K % 4 != 0 (j = 0, 3), a base 4 bytes off (j = 1), an odd ld (j = 2)
                    xl = {1: "shifted", 2: "odd_ld"}.get(j, xl)
                    wl = {5: "odd_ld"}.get(j, wl)
                jobs.append(GJob(M, Ks[j], xl, wl, ("none", "bias", "scale")[(j + ni) % 3], (j + ni) % 2 == 1, VALUE_CLASSES[(j + ni + mode) % 7]))
            for rt in (1, 2):
                js = tuple(jobs)
                if rt == 2:
                    js += (GJob(FILLER_M, 32 if mode == 2 else 36, "contig", "contig", "bias", False, "gauss"),)
                out.append(GroupedCase("g_N%d_rt%d_m%d" % (N, rt, mode), N, rt, mode, js))
    return out


def grouped_problems(c: GroupedCase):
    ps = []
    for j in c.jobs:
        (ldx, _, xm), (ldw, _, wm) = layout_spec(j.xl, j.K), layout_spec(j.wl, j.K)
        ps.append(FwdP(j.M, j.K, ldx, ldw, xm, wm))
    return ps


def grouped_expect(c: GroupedCase, precision):
    k, nt, rt, mode = fwd_grouped(grouped_problems(c), c.N, precision)
    assert (nt, rt, min(mode, 2)) == (ceil_div(c.N, 16), c.rt, c.mode), (c.name, precision, nt, rt, mode)
    return (k, nt, rt, mode)


def grouped_inputs(c: GroupedCase, j: int):
    """(X, W, b, bias_scale) of problem j - the same for both unit sizes and both precisions"""
    job = c.jobs[j]
    key = (c.N, c.mode, j)
    X = long_rows(job.cls, job.M, job.K, key, "X")
    W = values(job.cls, (c.N, job.K), key, "W", scale=0.25)
    b = None if job.bias == "none" else values("gauss", (c.N,), key, "b")
    bs = values("positive", (job.M,), key, "bs") if job.bias == "scale" and job.M <= PERIOD else None
    if job.bias == "scale" and bs is None:
        bs = values("positive", (PERIOD,), key, "bs")[np.arange(job.M) % PERIOD]
    return X, W, b, bs


class WgCase(NamedTuple):
    name: str
    kind: str                    # "f32" | "bf16x3" (the grouped entries)
    N: int
    K: int
    Ms: Tuple[int, ...]
    layout: str                  # of X and dY: contig | padded | shifted | odd_ld | slice (dY = the middle third of a [M, 3 N] buffer)
    db: bool
    accumulate: bool
    wide_dw: bool                # lddw > K
    cls: str
    expect: str


def wgrad_cases():
    out = []
    all_m = (433, 0, 1, 47, 48, 49, 143, 144)
    i = 0

    def add(kind, N, K, Ms, layout, db, acc, wide, expect):
        nonlocal i
        out.append(WgCase("w%02d_%s_%dx%d" % (i, kind, N, K), kind, N, K, tuple(Ms), layout, db, acc, wide, VALUE_CLASSES[i % 7], expect))
        i += 1

    for (N, K) in ((64, 64), (128, 192)):                         # fp32, fast
        add("f32", N, K, all_m, "contig", True, False, False, "linear_wgrad_kernel<true>")
        add("f32", N, K, (145,), "padded", False, True, True, "linear_wgrad_kernel<true>")
        add("f32", N, K, (144, 433, 49), "contig", True, True, False, "linear_wgrad_kernel<true>")
    for (N, K) in ((1, 1), (16, 40), (64, 36), (65, 65), (48, 100)):   # fp32, slow
        add("f32", N, K, all_m, "contig", True, False, False, "linear_wgrad_kernel<false>")
        add("f32", N, K, (145, 1), "odd_ld", False, True, True, "linear_wgrad_kernel<false>")
    add("f32", 64, 64, (433, 145, 48), "shifted", True, False, True, "linear_wgrad_kernel<false>")      # behind a misaligned view
    add("f32", 64, 64, (0, 0), "contig", True, False, False, "memset")
    for (N, K) in ((64, 64), (64, 192), (128, 64), (128, 128)):   # bf16x3, 64-wide k slabs through the grouped entry
        add("bf16x3", N, K, (1, 31, 32, 33, 63, 64, 65, 97), "contig", True, False, False, "linear_wgrad_bf16x3_kernel")
        add("bf16x3", N, K, (300, 97, 1), "slice", N == 64, True, True, "linear_wgrad_bf16x3_kernel")
        add("bf16x3", N, K, (300,), "padded", False, False, False, "linear_wgrad_bf16x3_kernel")
    add("bf16x3", 64, 128, (65, 0, 300), "contig", True, False, False, "linear_wgrad_bf16x3_kernel")   # an empty problem keeps the launch here
    add("bf16x3", 64, 128, (65, 300), "contig", True, False, False, "linear_wgrad_bf16x3_v2_multi_kernel/dense")   # the hand-over
    add("bf16x3", 64, 36, (65, 300), "contig", True, False, False, "linear_wgrad_kernel<false>")        # the fall-back: fast_shape fails
    add("bf16x3", 64, 64, (65, 300), "shifted", True, True, False, "linear_wgrad_kernel<false>")
    for c in out:
        plan = wgrad_grouped(wg_problems(c), c.N, c.K, c.kind, c.db, c.accumulate)
        assert plan["kernels"] == {c.expect}, (c, plan)
    return out


def wg_layout(layout, N, K):
    """((lddy, dY base % 16), (ldx, X base % 16))"""
    if layout == "slice":
        return (3 * N, (4 * N) % 16), (K, 0)
    (ly, _, my), (lx, _, mx) = layout_spec(layout, N), layout_spec(layout, K)
    return (ly, my), (lx, mx)


def wg_problems(c: WgCase):
    (ly, my), (lx, mx) = wg_layout(c.layout, c.N, c.K)
    return [WgP(M, ly, lx, my, mx) for M in c.Ms]


def wg_inputs(c, p: int, N=None, K=None, M=None, cls=None, name=None):
    """(dY [M, N], X [M, K]) of problem p of a gradient case"""
    N, K, M = N or c.N, K or c.K, c.Ms[p] if M is None else M
    cls, name = cls or c.cls, name or c.name
    if M > 100 and cls in ("positive", "scaled"):                 # (T_ACC is measured 8 deep: long all-positive or few-term sums keep to short problems)
        cls = "gauss"
    return values(cls, (M, N), name, p, "dY", scale=2.0 ** -6), values(cls, (M, K), name, p, "X")


class MProb(NamedTuple):
    M: int
    weight: bool = False         # db_row_weight
    n_list: Optional[int] = None  # a row list of this length
    hint: int = 0                # rows_expected
    slice_dy: bool = False       # dY = the middle third of a [M, 3 N] buffer


class MTarget(NamedTuple):
    K: int
    problems: Tuple[MProb, ...]
    db: bool
    accumulate: bool
    wide_dw: bool = False


class MultiCase(NamedTuple):
    name: str
    N: int
    budget: int
    targets: Tuple[MTarget, ...]
    cls: str
    version: int


def multi_cases():
    P = MProb
    big = 10 ** 6
    out = [
        MultiCase("o1_two", 64, 0, (MTarget(192, (P(517), P(16)), True, False), MTarget(64, (P(1), P(15), P(17), P(33)), False, True)), "gauss", 1),
        MultiCase("o1_four", 128, 7, (MTarget(192, (P(33), P(17, slice_dy=True)), True, True, True), MTarget(128, (P(517),), False, False),
                                     MTarget(64, (P(1),), True, False), MTarget(256, (P(15), P(16)), True, True, True)), "positive", 1),
        MultiCase("o1_budget1", 64, 1, (MTarget(192, (P(33), P(1)), True, False), MTarget(192, (P(517),), True, True)), "scaled", 1),
        MultiCase("o2_three", 64, 0, (MTarget(128, (P(517), P(1)), False, False), MTarget(256, (P(15), P(16, slice_dy=True), P(17)), True, True),
                                     MTarget(384, (P(33, True), P(517, True), P(16)), True, False)), "full24", 2),
        MultiCase("o2_budget1", 128, 1, (MTarget(128, (P(33), P(517, True)), True, True, True), MTarget(384, (P(1), P(17)), True, False, True)),
                  "low16clear", 2),
        MultiCase("o2_four", 64, 7, (MTarget(256, (P(517),), True, False), MTarget(128, (P(16),), False, True), MTarget(128, (P(15), P(1)), True, True),
                                    MTarget(384, (P(17), P(33)), False, False)), "zeros", 2),
        MultiCase("o2_n128", 128, 0, (MTarget(256, (P(517), P(33)), True, False), MTarget(128, (P(1, True),), True, True)), "negzero", 2),
        # row lists of every length beside a dense target; hints: none, too small, too large
        MultiCase("list64", 64, 0, (MTarget(128, (P(33, True, 0, 0), P(33, False, 1, 1), P(33, True, 15, big), P(33, False, 16, 0),
                                                  P(33, True, 17, 1), P(33, False, 33, big), P(517, True, 517, 20), P(517, False, 200, big)), True, False),
                                    MTarget(256, (P(33), P(517)), True, True)), "gauss", 2),
        MultiCase("list128", 128, 7, (MTarget(384, (P(517, False, 0, big), P(517, True, 1, 0), P(517, False, 15, 1), P(517, True, 16, big),
                                                    P(517, False, 17, 0), P(517, True, 517, 1)), True, True, True),
                                      MTarget(128, (P(17),), False, False)), "positive", 2),
        MultiCase("list_empty_only", 64, 0, (MTarget(128, (P(33, True, 0, 0),), True, False), MTarget(128, (P(16),), True, False)), "gauss", 2),
    ]
    for c in out:
        assert wgrad_multi_version(multi_targets(c)) == c.version and wgrad_multi(multi_targets(c), c.N, c.budget) is not None, c.name
    return out


def multi_targets(c: MultiCase):
    return tuple(WgT(t.K, t.K + 8 if t.wide_dw else t.K,
                     tuple(WgP(p.M, 3 * c.N if p.slice_dy else c.N, t.K, (4 * c.N) % 16 if p.slice_dy else 0, 0, p.n_list is not None, p.hint,
                               True, 0, p.weight) for p in t.problems), t.db, t.accumulate) for t in c.targets)


def multi_inputs(c: MultiCase, ti: int, pi: int):
    """(dY, X, w or None, ids or None): ids = the ascending row list (int32) of a listed problem"""
    t, p = c.targets[ti], c.targets[ti].problems[pi]
    dY, X = wg_inputs(None, (ti, pi), c.N, t.K, p.M, c.cls, c.name)
    w = values("positive", (p.M,), c.name, ti, pi, "w") if p.weight else None
    ids = None
    if p.n_list is not None:
        ids = np.sort(_rng(c.name, ti, pi, "ids").permutation(p.M)[:p.n_list]).astype(np.int32)
    return dY, X, w, ids


def adamw_cases():
    """multi-target launches run with the AdamW update inside the reduction (dW contiguous, nothing accumulated): N = 128 and organisation 1"""
    P = MProb
    return [MultiCase("adamw_n128", 128, 0, (MTarget(256, (P(517), P(33, True)), True, False), MTarget(128, (P(17),), False, False)), "gauss", 2),
            MultiCase("adamw_o1", 64, 0, (MTarget(192, (P(517), P(33)), True, False), MTarget(64, (P(17),), False, False)), "gauss", 1)]


# the cases the T_ACC measurement, the emulation checks and the mutants run on: (class, name, A [n, a], B [n, b], add) with
# out[a, b] = sum_r A[r, a] B[r, b]; forward: A = X^T's rows = k, i.e. A = X.T, B = W.T
@functools.lru_cache(maxsize=None)
def precision_cases():
    """8 deep: at this depth every mutant of tests/test_dense_ref_cpu.py exceeds 2 x T_ACC x S while T_ACC keeps its factor 4 over the
    per-product emulation (deeper cases do not: the emulation's error grows with the depth, a lost 2^-16 term does not)."""
    out = []
    for i, cls in enumerate(VALUE_CLASSES):
        X, W = values(cls, (48, PRECISION_DEPTH), "pf", i, "X"), values(cls, (40, PRECISION_DEPTH), "pf", i, "W", scale=0.25)
        b, bs = values("gauss", (40,), "pf", i, "b"), values("positive", (48,), "pf", i, "bs")
        out.append(("fwd", "fwd_%s" % cls, X.T.copy(), W.T.copy(), (bs, b)))
    for i, cls in enumerate(VALUE_CLASSES):
        dY, X = values(cls, (PRECISION_DEPTH, 32), "pw", i, "dY", scale=2.0 ** -6), values(cls, (PRECISION_DEPTH, 64), "pw", i, "X")
        out.append(("wgrad", "wgrad_%s" % cls, dY, X, None))
    return tuple(out)


def precision_reference(case):
    """(ideal six-term value, fp64 value, S) of a precision case"""
    _, _, A, B, add = case
    six = sum(a.astype(np.float64).T @ b.astype(np.float64) for a, b in _terms(A, B))
    full = A.astype(np.float64).T @ B.astype(np.float64)
    S = np.abs(A.astype(np.float64)).T @ np.abs(B.astype(np.float64))
    if add is not None:
        bias = add[0].astype(np.float64)[:, None] * add[1].astype(np.float64)[None, :]
        six, full, S = six + bias, full + bias, S + np.abs(bias)
    return six, full, S
