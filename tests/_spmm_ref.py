"""float64 reference, derived per-element error bounds and the case table of the SpMM kernel families (llmrec_amd/csrc/spmm.hip).
NumPy only: no device, no torch.cuda. Used by tests/test_spmm_ref_cpu.py (the bounds are sound and not vacuous, the table reaches every
kernel) and tests/test_gpu_spmm_families.py (every kernel family against this reference).

The operation:  Y = post_scale . op(alpha Z + diag(rs) (P . val) diag(cs) X),  op in {none, row softmax, row softmax backward}.

family_and_variant() restates the dispatch rule of spmm_prepare (llmrec_amd/csrc/spmm.hip:816-831: the epi_aligned line, then
"const int dd = a.d;" to "out.variant = ..."; the quoted fragments locate the rule should the line numbers drift):
    dd    = slice_width > 0 ? slice_width : d
    vec4  = dd % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (Z, S absent or ld % 4 == 0 and 16-byte aligned) && X, Y, partials 16-byte aligned
    vec4:   family 0 (dd <= 16), 1 (<= 32), 2 (<= 64), 3 (<= 128), 4 (<= 256), 5 (<= 512), 6 (<= 1024), else unsupported
    scalar: family 7 (dd <= 16), 8 (<= 64), 9 (<= 256), else unsupported
    weighted = val || col_scale;  variant = x_row_mask ? (weighted ? MASKED_W : MASKED) : (weighted ? WEIGHTED : PLAIN)
and spmm_run's switch maps the families to (LPR, NCHUNK, VEC) = <4,1,4> <8,1,4> <16,1,4> <32,1,4> <64,1,4> <64,2,4> <64,4,4> <16,1,1>
<64,1,1> <64,4,1>. llmrec_spmm_rows_compact_f32 (spmm.hip:1056-1083) has the same rule without Z / S, up to 256 (vector) / 64 (scalar)
columns.

Error bounds (u = 2^-24, the unit round-off of fp32; deg = the row's nnz):
  linear part   t = alpha z + rs * sum_j w_j x_j,  w_j = val_j cs_j:
      B = (deg + 6) u (|rs| sum_j |val_j| |cs_j| |x_j| + |alpha z|)
    Any order of n fp32 additions errs by at most (n - 1) u (1 + O(nu)) times the sum of the magnitudes; the product val * cs, the fma
    that adds a term, the row scale and the alpha fma are four more roundings; the remaining two units cover the second-order terms
    ((deg + 4)^2 u^2 / 2 < 2 u up to deg = 2100). B == 0 (an empty row without Z, a row without an active neighbour) demands exactly 0.0.
    Masked products: the sum of magnitudes runs over the ACTIVE columns only, but deg stays the row's full nnz, as the formula is set:
    for a row with few active neighbours (the 2100-nnz row with about 210 of them) the bound is several times looser than the count
    of additions the kernel really makes would allow. It is still a per-element bound on that row's own magnitudes, and zero where
    nothing is active.
  post_scale multiplies every bound by |post_scale| (its own rounding is inside the slack of the bound it scales).
  softmax       y_k = exp(t_k - m) / sum_j exp(t_j - m), m = max t. A perturbation |dt| <= Bmax = max_k B_k of the row changes every y_k by
    at most the relative amount exp(2 Bmax) - 1 ~ 2 Bmax. In fp32: the subtraction t_k - m errs by u |t_k - m|, which expf turns into the
    same RELATIVE error; expf itself, the d - 1 additions of the denominator, the reciprocal and the final product are d + O(1) more
    relative roundings:   rel_k = 2 Bmax + (d + max_k |t_k - m| + 8) u.
    Nothing may underflow for this to hold: reference() asserts max_k |t_k - m| <= 30 (exp(-30) ~ 1e-13, far above the fp32 subnormals).
  softmax backward   out_k = S_k (t_k - c), c = sum_j t_j S_j, from the computed t' = t + dt, |dt_k| <= B_k:
      c' = fl(sum_j t'_j S_j): d products and d - 1 additions in any order: |c' - sum t'_j S_j| <= gamma_{d+1} sum |t'_j S_j| with
           gamma_n = n u / (1 - n u) <= (n + 1) u while n (n + 1) u <= 1 (n <= 4095), so
      Ec = |c' - c| <= sum_j B_j |S_j| + (d + 2) u sum_j (|t_j| + B_j) |S_j|;
      the subtraction, the product with S_k and post_scale are three roundings of (t'_k - c'): relative gamma_3 <= 4 u of
      |t'_k - c'| <= |t_k| + |c| + B_k + Ec:
      |out'_k - out_k| <= |S_k| (B_k + Ec + 4 u (|t_k| + |c| + B_k + Ec)).
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Tuple

import numpy as np

U = 2.0 ** -24
N_ROWS, N_COLS = 100, 2200
LONG_ROW = 32                        # LLMREC_SPMM_LONG_ROW
ROW_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 700, 1000, 2100)
STAMP = 77                           # x_mask_active
SENTINEL = 12345.0                   # what Y and its guards hold before a call

# (t_wave, t_block, segment)
TRIPLES = {
    "buckets": (64, 128, 128),       # every bucket populated; rows of 129 and 257 nnz end in a segment of 1 nnz
    "block8": (64, 1024, 1024),      # the 1000-nnz row runs all 8 waves of block_range
    "split": (32, 32, 32),           # everything past the lane-group bucket is split; 2100 nnz = 66 segments > 256 / 4
}
BUCKETS = ("lane_group", "wavefront", "block", "split")

FAMILY_SHAPE = ((4, 1, 4), (8, 1, 4), (16, 1, 4), (32, 1, 4), (64, 1, 4), (64, 2, 4), (64, 4, 4), (16, 1, 1), (64, 1, 1), (64, 4, 1))
VARIANTS = ("plain", "weighted", "masked", "masked_weighted")

# (width, behind a misaligned view) per family
FAMILY_WIDTHS = {
    0: ((4, False), (12, False), (16, False)),
    1: ((20, False), (32, False)),
    2: ((36, False), (64, False)),
    3: ((68, False), (128, False)),
    4: ((132, False), (256, False)),
    5: ((260, False), (448, False), (512, False)),
    6: ((516, False), (1024, False)),
    7: ((1, False), (3, False), (15, False), (16, True)),
    8: ((17, False), (50, False), (63, False), (64, True)),
    9: ((65, False), (130, False), (255, False), (256, True)),
}
# the width each family's plan and epilogue sweeps run at: one where the last lanes of a group hold no column
FAMILY_REP = {0: (12, False), 1: (20, False), 2: (36, False), 3: (68, False), 4: (132, False), 5: (260, False), 6: (516, False),
              7: (15, False), 8: (50, False), 9: (130, False)}

KINDS = ("pattern_rs", "val", "cs_rs", "val_cs", "mask_none", "mask_all", "mask_some", "mask_cs")
VARIANT_KINDS = ("pattern_rs", "val_cs", "mask_some", "mask_cs")           # one operand kind per kernel variant
OPS = ("none", "z", "acc", "softmax", "softmax_bwd")
EPILOGUES = tuple((op, post) for op in OPS for post in (False, True))
TRIGGERS = ("X", "ldx", "Y", "ldy", "Z", "S", "partials")


@dataclasses.dataclass(frozen=True)
class Case:
    d: int
    kind: str                        # KINDS
    op: str                          # OPS: none | z (alpha Z, alpha = 1/3) | acc (Z = Y, alpha = 1) | softmax | softmax_bwd (with alpha Z)
    post: bool                       # post_scale
    plan: str                        # TRIPLES
    permuted: bool = False           # the plan carries the permuted CSR (pattern-only operands)
    slice_width: int = 0
    misaligned: Tuple[str, ...] = () # TRIGGERS

    @property
    def width(self):
        return self.slice_width or self.d

    @property
    def masked(self):
        return self.kind.startswith("mask")

    @property
    def has_val(self):
        return self.kind in ("val", "val_cs")

    @property
    def has_cs(self):
        return self.kind in ("cs_rs", "val_cs", "mask_cs")

    @property
    def has_rs(self):
        # the softmax cases always scale by 1/sqrt(deg): the reference's no-underflow condition
        return self.kind not in ("val", "val_cs") or self.op in ("softmax", "softmax_bwd")

    @property
    def has_z(self):
        return self.op in ("z", "acc", "softmax_bwd")

    @property
    def alpha(self):
        return {"z": np.float32(1.0 / 3.0), "acc": np.float32(1.0), "softmax_bwd": np.float32(1.0 / 3.0)}.get(self.op, np.float32(0.0))

    def label(self):
        f, v = family_and_variant(self)
        return "family %d <%d,%d,%d> %s, d = %d%s, %s, plan %s %s%s, epilogue %s%s%s" % (
            (f,) + FAMILY_SHAPE[f] + (v, self.d, " sliced by %d" % self.slice_width if self.slice_width else "", self.kind, self.plan,
                                      TRIPLES[self.plan], " permuted" if self.permuted else "", self.op, " + post_scale" if self.post else "",
                                      " misaligned " + "+".join(self.misaligned) if self.misaligned else ""))


def family_of_width(w: int, vec4: bool) -> int:
    """the family of spmm_prepare for dd = w; -1: outside the compiled families (LLMREC_EUNSUPPORTED)"""
    if vec4:
        for f, top in enumerate((16, 32, 64, 128, 256, 512, 1024)):
            if w <= top:
                return f
        return -1
    for f, top in ((7, 16), (8, 64), (9, 256)):
        if w <= top:
            return f
    return -1


def family_and_variant(case: Case):
    vec4 = case.width % 4 == 0 and not case.misaligned
    weighted = case.has_val or case.has_cs
    variant = ("masked_weighted" if weighted else "masked") if case.masked else ("weighted" if weighted else "plain")
    return family_of_width(case.width, vec4), variant


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr int32 [N_ROWS + 1], colidx int32 [nnz], deg int64 [N_ROWS]): the listed row lengths at scattered rows, 0..12 elsewhere;
    distinct ascending columns per row."""
    rng = np.random.default_rng(2024)
    deg = rng.integers(0, 13, size=N_ROWS)
    for k, n in enumerate(ROW_LENGTHS):
        deg[(k * 5 + 2) % N_ROWS] = n
    rowptr = np.zeros(N_ROWS + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    colidx = np.concatenate([np.sort(rng.choice(N_COLS, size=int(n), replace=False)) for n in deg])
    for a in (rowptr, colidx, deg):
        a.setflags(write=False)
    return rowptr.astype(np.int32), colidx.astype(np.int32), deg.astype(np.int64)


def row_buckets(plan: str):
    """bucket name per row under the plan's thresholds (llmrec_spmm_plan_t)"""
    t_wave, t_block, _ = TRIPLES[plan]
    deg = graph()[2]
    return np.where(deg <= LONG_ROW, 0, np.where(deg <= t_wave, 1, np.where(deg <= t_block, 2, 3)))


def _signed(rng, n):
    return (rng.uniform(0.5, 1.5, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def graph_inputs():
    rowptr, colidx, deg = graph()
    rng = np.random.default_rng(7)
    out = dict(val=_signed(rng, colidx.size), cs=_signed(rng, N_COLS), ps=_signed(rng, N_ROWS),
               rs=(1.0 / np.sqrt(np.maximum(deg, 1))).astype(np.float32))
    act = rng.random(N_COLS) < 0.10
    stale = rng.integers(0, 60, size=N_COLS).astype(np.uint8)                   # stale byte values count as not active
    out["mask_some"] = np.where(act, np.uint8(STAMP), stale)
    out["mask_none"] = stale.copy()
    out["mask_all"] = np.full(N_COLS, STAMP, dtype=np.uint8)
    out["z_rows"] = rng.random(N_ROWS) < 0.5                                    # the non-zero rows of Z (z_row_flag)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def width_inputs(d: int):
    """X [N_COLS, d] unit normal, Z [N_ROWS, d] (zero outside z_rows), S [N_ROWS, d] softmax rows: fp32, one set per width"""
    rng = np.random.default_rng(1000 + d)
    X = rng.standard_normal((N_COLS, d)).astype(np.float32)
    Z = rng.standard_normal((N_ROWS, d)).astype(np.float32)
    Z[~graph_inputs()["z_rows"]] = 0.0
    e = np.exp(rng.standard_normal((N_ROWS, d)))
    S = (e / e.sum(1, keepdims=True)).astype(np.float32)
    for a in (X, Z, S):
        a.setflags(write=False)
    return X, Z, S


def inputs(case: Case):
    """the fp32 operands of a case (None = absent); mask: uint8 [N_COLS] or None; X as the kernel may see it (inactive rows NOT zeroed here:
    the device test poisons them, reference() zeroes them)"""
    gi = graph_inputs()
    X, Z, S = width_inputs(case.d)
    return dict(X=X, Z=Z if case.has_z else None, S=S if case.op == "softmax_bwd" else None, alpha=case.alpha,
                val=gi["val"] if case.has_val else None, cs=gi["cs"] if case.has_cs else None, rs=gi["rs"] if case.has_rs else None,
                ps=gi["ps"] if case.post else None,
                mask={"mask_none": gi["mask_none"], "mask_all": gi["mask_all"], "mask_some": gi["mask_some"],
                      "mask_cs": gi["mask_some"]}.get(case.kind))


@functools.lru_cache(maxsize=None)
def _dense(has_val: bool, has_cs: bool, mask_name):
    """float64 dense (P . val) diag(cs) with the inactive columns removed"""
    rowptr, colidx, deg = graph()
    gi = graph_inputs()
    A = np.zeros((N_ROWS, N_COLS))
    rows = np.repeat(np.arange(N_ROWS), deg)
    A[rows, colidx] = gi["val"].astype(np.float64) if has_val else 1.0
    if has_cs:
        A = A * gi["cs"].astype(np.float64)[None, :]
    if mask_name is not None:
        A = A * (gi[mask_name] == STAMP)[None, :]
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=24)
def _linear(has_val: bool, has_cs: bool, mask_name, d: int):
    """(sum_j w_j x_j, sum_j |w_j| |x_j|) in float64, before the row scale"""
    A = _dense(has_val, has_cs, mask_name)
    X = width_inputs(d)[0].astype(np.float64)
    return A @ X, np.abs(A) @ np.abs(X)


def linear_bound(deg, mag):
    """(deg + 6) u * (sum of the magnitudes that enter the row): the linear part's bound"""
    return (np.asarray(deg, dtype=np.float64)[:, None] + 6.0) * U * mag


def reference(case: Case, Y0=None):
    """(want, bound, relative): float64 result of the case and its per-element error bound; relative = True (softmax): the bound is a
    relative tolerance |got - want| <= bound * |want|. Y0: the contents of Y before an accumulating call (op acc; default: Z of the case)."""
    deg = graph()[2]
    inp = inputs(case)
    mask_name = {"mask_cs": "mask_some"}.get(case.kind, case.kind) if case.masked else None
    lin, mag = _linear(case.has_val, case.has_cs, mask_name, case.d)
    if inp["rs"] is not None:
        rs = inp["rs"].astype(np.float64)[:, None]
        lin, mag = rs * lin, np.abs(rs) * mag
    if case.has_z:
        z = (Y0 if (case.op == "acc" and Y0 is not None) else inp["Z"]).astype(np.float64) * np.float64(inp["alpha"])
        lin, mag = lin + z, mag + np.abs(z)
    t, B = lin, linear_bound(deg, mag)
    ps = inp["ps"].astype(np.float64)[:, None] if inp["ps"] is not None else 1.0
    if case.op == "softmax":
        m = t.max(1, keepdims=True)
        spread = (m - t).max(1, keepdims=True)
        assert float(spread.max()) <= 30.0, ("softmax case would underflow", case, float(spread.max()))
        e = np.exp(t - m)
        want = ps * e / e.sum(1, keepdims=True)
        rel = 2.0 * B.max(1, keepdims=True) + (case.d + spread + 8.0) * U
        return want, np.broadcast_to(rel, want.shape).copy(), True
    if case.op == "softmax_bwd":
        S = inp["S"].astype(np.float64)
        aS = np.abs(S)
        c = (t * S).sum(1, keepdims=True)
        Ec = (B * aS).sum(1, keepdims=True) + (case.d + 2.0) * U * ((np.abs(t) + B) * aS).sum(1, keepdims=True)
        bound = aS * (B + Ec + 4.0 * U * (np.abs(t) + np.abs(c) + B + Ec))
        return ps * S * (t - c), np.abs(ps) * bound, False
    return ps * t, np.abs(ps) * B, False


def row_hit(case: Case):
    """rows whose result can be non-zero as y_row_flag defines it: an active neighbour, or a flagged (non-zero) Z row"""
    assert case.masked
    mask_name = {"mask_cs": "mask_some"}.get(case.kind, case.kind)
    hit = np.abs(_dense(False, False, mask_name)).sum(1) > 0
    if case.has_z:
        hit = hit | graph_inputs()["z_rows"]
    return hit


def _cases():
    out = []
    # A: every width of every family x every operand kind, all buckets in one launch; the epilogues in rotation (mask_all takes
    #    pattern_rs's epilogue: the two must agree bit for bit)
    i = 0
    for f, widths in FAMILY_WIDTHS.items():
        for d, mis in widths:
            i += 1
            for k, kind in enumerate(KINDS):
                op, post = EPILOGUES[(i + (0 if kind == "mask_all" else 3 * k)) % len(EPILOGUES)]
                out.append(Case(d, kind, op, post, "buckets", misaligned=("X", "Y") if mis else ()))
    # B: every threshold triple, as the plain and (pattern-only operands) as the permuted plan, per family
    for f, (d, mis) in FAMILY_REP.items():
        for k, kind in enumerate(VARIANT_KINDS):
            for p, plan in enumerate(TRIPLES):
                op, post = EPILOGUES[(f + 2 * k + 3 * p) % len(EPILOGUES)]
                for permuted in ((False, True) if kind in ("pattern_rs", "mask_some") else (False,)):
                    out.append(Case(d, kind, op, post, plan, permuted=permuted))
    # C: every epilogue x every kernel variant per family, the plans in rotation
    for f, (d, mis) in FAMILY_REP.items():
        for k, kind in enumerate(VARIANT_KINDS):
            for e, (op, post) in enumerate(EPILOGUES):
                out.append(Case(d, kind, op, post, tuple(TRIPLES)[(f + k + e) % 3]))
    # D: column slices (the softmax epilogues need the whole row)
    sliceable = tuple(e for e in EPILOGUES if e[0] in ("none", "z", "acc"))
    for s, (d, mis) in enumerate(((128, False), (448, False), (128, True))):
        for k, kind in enumerate(KINDS):
            for p, plan in enumerate(("buckets", "split")):
                op, post = sliceable[(s + (0 if kind == "mask_all" else k) + 2 * p) % len(sliceable)]
                out.append(Case(d, kind, op, post, plan, slice_width=64, misaligned=("X", "Y") if mis else ()))
    # E: each alignment trigger alone at d = 64, everything else aligned
    for trig in TRIGGERS:
        for kind in ("pattern_rs", "val_cs", "mask_some"):
            op = {"Z": "z", "S": "softmax_bwd"}.get(trig, "none")
            out.append(Case(64, kind, op, kind == "val_cs", "split" if trig == "partials" else "buckets", misaligned=(trig,)))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return tuple(uniq)


TABLE = _cases()


def family_cases(f: int):
    return tuple(c for c in TABLE if family_and_variant(c)[0] == f)
