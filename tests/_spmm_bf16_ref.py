"""float64 reference and per-element bounds of the SpMM that gathers bf16 rows (llmrec_amd/csrc/spmm_bf16.hip: llmrec_spmm_xbf16_f32,
llmrec_rows_to_bf16). NumPy only. Used by tests/test_spmm_bf16_cpu.py (the yardstick is sound and tells the bf16 gather from an fp32
one) and tests/test_gpu_spmm_bf16.py.

The contract: Y = post_scale . op(alpha Z + diag(rs) (P . val) diag(cs) widen(Xb)), Xb = RNE_bf16(X) - exactly llmrec_spmm_f32 on the
fp32 tensor widen(Xb). So everything of tests/_spmm_ref.py is reused by import - its graph (100 x 2200, rows of 0 .. 2100 nnz), its
operands, the formulas of reference() and linear_bound - with ONE substitution: X is rounded to bf16 (round to nearest even) first.
The rounding is an input transformation, not an error of the kernel, so the bound keeps its (deg + 6) u: it does not widen by the
2^-9 of a bf16 rounding, and that is what lets it tell a kernel that gathered the fp32 rows from one that gathered the bf16 ones.

rn_bf16_bits restates the bit formula of the kernels (common.h: rn_bf16_bits, which spmm_body.h and topk.hip share):
    b = bits(x);  bf16 = (b + 0x7fff + ((b >> 16) & 1)) >> 16        (NaN -> 0x7fc0)
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

from tests import _spmm_ref as R

KINDS = ("pattern_rs", "val_cs")                 # the plain and the weighted kernel (the masked products stay fp32)
WIDTHS = (12, 16, 20, 32, 36, 64, 68, 128, 132, 256)          # every family at its representative and its full width
PLAN_WIDTHS = (36, 64, 128)
EPILOGUE_WIDTHS = (64, 128)


def rn_bf16_bits(x: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns of an fp32 array, round to nearest even"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7fffffff) > 0x7f800000
    return np.where(nan, np.uint16(0x7fc0), out)


def widen(bits: np.ndarray) -> np.ndarray:
    """the fp32 array with the values of uint16 bf16 bit patterns (exact)"""
    return (bits.astype(np.uint32) << 16).view(np.float32)


def round_bf16(x: np.ndarray) -> np.ndarray:
    return widen(rn_bf16_bits(x))


@functools.lru_cache(maxsize=16)
def rounded_x(d: int) -> np.ndarray:
    """widen(RNE_bf16(X)) of the width's X of tests/_spmm_ref.py"""
    Xr = round_bf16(R.width_inputs(d)[0])
    Xr.setflags(write=False)
    return Xr


@functools.lru_cache(maxsize=24)
def _linear_rounded(has_val: bool, has_cs: bool, mask_name, d: int):
    A = R._dense(has_val, has_cs, mask_name)
    X = rounded_x(d).astype(np.float64)
    return A @ X, np.abs(A) @ np.abs(X)


@contextlib.contextmanager
def _x_rounded():
    """inside: R.reference() sums the rounded X (its _linear is the only place X enters)"""
    keep = R._linear
    R._linear = _linear_rounded
    try:
        yield
    finally:
        R._linear = keep


def reference(case: R.Case, Y0=None):
    """(want, bound, relative) of R.reference for the case on widen(bf16(X))"""
    assert not case.masked and case.slice_width == 0 and not case.misaligned
    with _x_rounded():
        return R.reference(case, Y0)


def cases():
    """The kernel cases of the GPU test: (a) every width x both kinds, all buckets in one launch, the epilogues in rotation; (b) the three
    threshold triples, plain and (pattern-only) permuted plans; (c) every epilogue with and without post_scale at d = 64 and 128."""
    out = []
    for i, d in enumerate(WIDTHS):
        for k, kind in enumerate(KINDS):
            op, post = R.EPILOGUES[(i + 3 * k) % len(R.EPILOGUES)]
            out.append(R.Case(d, kind, op, post, "buckets"))
    for i, d in enumerate(PLAN_WIDTHS):
        for k, kind in enumerate(KINDS):
            for p, plan in enumerate(R.TRIPLES):
                op, post = R.EPILOGUES[(i + 2 * k + 3 * p) % len(R.EPILOGUES)]
                for permuted in ((False, True) if kind == "pattern_rs" else (False,)):
                    out.append(R.Case(d, kind, op, post, plan, permuted=permuted))
    for i, d in enumerate(EPILOGUE_WIDTHS):
        for k, kind in enumerate(KINDS):
            for e, (op, post) in enumerate(R.EPILOGUES):
                out.append(R.Case(d, kind, op, post, tuple(R.TRIPLES)[(i + k + e) % 3]))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return tuple(uniq)


def fp32_chain(case: R.Case, X: np.ndarray) -> np.ndarray:
    """The linear part of a case (op none / z, no post_scale) as ONE sequential fp32 chain per row over the rows of X, in column order:
    acc = fl(acc + fl(w_j x_j)), then the row scale and alpha z - a legitimate summation order of the kernel's terms in NumPy fp32."""
    assert case.op in ("none", "z") and not case.post
    rowptr, colidx, _ = R.graph()
    inp = R.inputs(case)
    out = np.zeros((R.N_ROWS, case.d), dtype=np.float32)
    for r in range(R.N_ROWS):
        acc = np.zeros(case.d, dtype=np.float32)
        for e in range(rowptr[r], rowptr[r + 1]):
            c = colidx[e]
            w = np.float32(1.0)
            if inp["val"] is not None:
                w = inp["val"][e]
            if inp["cs"] is not None:
                w = np.float32(w * inp["cs"][c])
            acc = acc + (X[c] if (inp["val"] is None and inp["cs"] is None) else w * X[c])
        if inp["rs"] is not None:
            acc = acc * inp["rs"][r]
        if case.has_z:
            acc = inp["alpha"] * inp["Z"][r] + acc
        out[r] = acc
    return out


def rows_out_of_bound(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """bool per row: some element errs by more than its bound"""
    return (np.abs(got.astype(np.float64) - want) > bound).any(1)


def worst_ratio(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    err = np.abs(got.astype(np.float64) - want)
    pos = bound > 0
    assert np.all(err[~pos] == 0.0)
    return float((err[pos] / bound[pos]).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# The row-sharded step in bf16 gather mode (llmrec_amd/dist_fused.py, gather_dtype = "bf16") against the single-process oracle.
# The 900 x 700 problem of tests/test_gpu_dist_fused.py, restated; the oracle's loop with every operand a bf16 product gathers rounded
# at the point the step rounds it:
#   forward   U^{l+1} = diag(s_u) R bf16(I^l),  I^{l+1} = diag(s_i) R^T bf16(U^{l+1})     (the row-restricted last layer stays fp32)
#   backward  dI^l = R^T bf16(s_u . dU^{l+1}),  dU^{l+1} += R bf16(s_i . dI^{l+1})        (the last layer's masked R g stays fp32)
# Its largest loss deviation from the fp32 oracle over the steps is what rounding the gathered rows costs on this problem, and four
# times that figure is the gate of the GPU test (the factor covers the different summation trees of torch's CPU sums and the kernels).
# The figures are recorded in STEP_DEVIATION (torch CPU, fp32, three steps); tests/test_spmm_bf16_cpu.py recomputes them and holds the
# record to within a factor of two (torch's CPU sums may be cut differently on another machine).
# ---------------------------------------------------------------------------------------------------------------------------------
STEP_U, STEP_I, STEP_L, STEP_B, STEP_STEPS = 900, 700, 2, 128, 3
STEP_DROP, STEP_DECAY, STEP_LR = 0.71, 1e-5, 1e-3
STEP_CASES = ((64, 0), (128, 6))                 # (d, augmented triples per rank)
# (d, n_aug, sparse_forward, world) -> the largest |loss(bf16 rounding) - loss(fp32)| of oracle_losses over the three steps (the losses
# are about 0.72: seven to eighteen units of the sixth significant digit)
STEP_DEVIATION = {(64, 0, True, 1): 5.48e-6, (64, 0, False, 1): 5.13e-6, (128, 6, True, 1): 1.264e-5, (128, 6, False, 1): 1.162e-5,
                  (64, 0, True, 2): 6.08e-6, (128, 6, True, 2): 8.46e-6,
                  (64, 0, False, 1, "dense backward"): 5.25e-6}            # sparse_backward=False


def step_problem(world: int, D: int, n_aug: int):
    """(rows, cols, user table, item table, batches[step][rank] = (users, pos, neg)): hubs on both sides, duplicate gradient rows"""
    U_, I_ = STEP_U, STEP_I
    rng = np.random.default_rng(4)
    deg = rng.integers(1, 30, size=U_); deg[7] = 600; deg[U_ - 3] = 200
    rows = np.repeat(np.arange(U_), deg)
    cols = np.concatenate([rng.choice(I_, size=c, replace=False) for c in deg])
    hot = rng.integers(0, U_, size=2500); rows = np.concatenate([rows, hot]); cols = np.concatenate([cols, np.full(hot.size, 5)])
    key = np.unique(rows * I_ + cols); rows, cols = key // I_, key % I_
    u_tab = (rng.standard_normal((U_, D)) * 0.1).astype(np.float32)
    i_tab = (rng.standard_normal((I_, D)) * 0.1).astype(np.float32)
    per = (U_ + world - 1) // world
    batches = []
    for s in range(STEP_STEPS):
        per_rank = []
        for r in range(world):
            u0, u1 = r * per, min((r + 1) * per, U_)
            pos = rng.integers(0, I_, size=STEP_B); pos[:40] = 5
            us, ns = rng.integers(u0, u1, size=STEP_B), rng.integers(0, I_, size=STEP_B)
            if n_aug:
                us, pos, ns = np.concatenate([us, us[:n_aug]]), np.concatenate([pos, rng.integers(0, I_, size=n_aug)]), \
                    np.concatenate([ns, rng.integers(0, I_, size=n_aug)])
            per_rank.append((us, pos, ns))
        batches.append(per_rank)
    return rows, cols, u_tab, i_tab, batches


@functools.lru_cache(maxsize=None)
def oracle_losses(world: int, D: int, n_aug: int, gather: str, sparse_forward: bool = True, sparse_backward: bool = True):
    """the losses of the oracle's training loop (torch CPU, fp32) on step_problem; gather = "bf16": the gathered operands rounded as the
    step rounds them (above; sparse_backward=False: the last layer's R g is a dense bf16 product too). A tuple of STEP_STEPS floats."""
    import scipy.sparse as sp
    import torch
    from oracle import oracle as O
    rows, cols, u_tab, i_tab, batches = step_problem(world, D, n_aug)
    Rm = sp.csr_matrix((np.ones(rows.size, dtype=np.float32), (rows, cols)), shape=(STEP_U, STEP_I))
    idx = torch.from_numpy(np.vstack((rows, cols)).astype(np.int64))
    R_ui = torch.sparse_coo_tensor(idx, torch.ones(rows.size), (STEP_U, STEP_I)).coalesce()
    R_iu = R_ui.t().coalesce()
    inv = lambda deg: torch.where(deg > 0, (1.0 / torch.sqrt(deg.double())).float(), torch.zeros_like(deg))
    s_u = inv(torch.tensor(np.asarray(Rm.sum(1)).ravel(), dtype=torch.float32))
    s_i = inv(torch.tensor(np.asarray(Rm.sum(0)).ravel(), dtype=torch.float32))
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)

    class Product(torch.autograd.Function):
        """Y = diag(s) P q(X);  dX = P^T q'(s . dY);  q, q' = the bf16 rounding where the step's product gathers bf16 rows"""
        @staticmethod
        def forward(ctx, P, Pt, s, X, round_fwd, round_bwd):
            ctx.Pt, ctx.s, ctx.round_bwd = Pt, s, round_bwd
            return s[:, None] * torch.sparse.mm(P, bf(X) if round_fwd else X)

        @staticmethod
        def backward(ctx, dY):
            h = ctx.s[:, None] * dY
            return None, None, None, torch.sparse.mm(ctx.Pt, bf(h) if ctx.round_bwd else h), None, None

    on = gather == "bf16"
    pu = torch.tensor(u_tab, requires_grad=True); pi = torch.tensor(i_tab, requires_grad=True)
    opt = torch.optim.AdamW([{"params": [pu, pi]}], lr=STEP_LR)
    cfg = O.Config(batch_size=world * STEP_B, decay=STEP_DECAY, prune_loss_drop_rate=STEP_DROP)
    losses = []
    for per_rank in batches:
        us = np.concatenate([b[0] for b in per_rank]); ps = np.concatenate([b[1] for b in per_rank]); ns = np.concatenate([b[2] for b in per_rank])
        u, i = pu, pi
        ul, il = [u], [i]
        for l in range(STEP_L):
            last = l == STEP_L - 1
            dense_fwd = on and not (last and sparse_forward)      # the row-restricted last layer: both products fp32
            # backward of the user product = the chunked R^T h (always dense); of the item product = R g (masked fp32 on the last layer)
            u = Product.apply(R_ui, R_iu, s_u, i, dense_fwd, on)
            if last: u = torch.softmax(u, -1)
            i = Product.apply(R_iu, R_ui, s_i, u, dense_fwd, on and not (last and sparse_backward))
            if last: i = torch.softmax(i, -1)
            ul.append(u); il.append(i)
        eu, ei = torch.mean(torch.stack(ul), 0), torch.mean(torch.stack(il), 0)
        mf, emb = O.bpr_loss(eu[torch.tensor(us)], ei[torch.tensor(ps)], ei[torch.tensor(ns)], cfg)
        opt.zero_grad(); (mf + emb).backward(); opt.step()
        losses.append(float((mf + emb).detach()))
    return tuple(losses)


def step_deviation(D: int, n_aug: int, sparse_forward: bool, world: int = 1, sparse_backward: bool = True) -> float:
    """max over the steps of |loss(bf16 rounding) - loss(fp32)| of the oracle's loop"""
    a, b = oracle_losses(world, D, n_aug, "bf16", sparse_forward, sparse_backward), oracle_losses(world, D, n_aug, "fp32", True)    # (fp32: one loop either way)
    return max(abs(x - y) for x, y in zip(a, b))
