"""The yardstick of tests/test_gpu_bpr_families.py for the BPR + prune loss kernels of llmrec_amd/csrc/bpr.hip (scores, rank / select,
reduce, pack, the deterministic run scatter bpr_bwd_runs_kernel<VEC, NV>, bpr_bwd_rows_kernel, bpr_zero_rows_kernel): the dispatch
restated, an fp64 reference written from the definition (oracle.bpr_loss and its closed-form derivative) with a bound PER ELEMENT, fp32
emulations of the kernels' own order with the mutants tests/test_bpr_ref_cpu.py uses, and the case table. numpy only; nothing here imports
llmrec_amd or torch.

DISPATCH (launch_bwd_runs and the entry points)
  The scatter takes the float4 rows (VEC) iff d % 4 == 0, ldu, ldi, lddu, lddi of EVERY problem are multiples of 4 and Eu, Ei, dEu, dEi of
  every problem are 16-byte aligned; else the scalar rows. NV = 1 iff d <= 64, else 2; a pass of a 16-lane group covers 64 NV columns. The
  first problem with a given target pointer owns it and sums, in ascending problem index, every later problem with that pointer; any_reg
  (the REG template axis) is per such group: some member's base = fl(fl(-4 decay / bsz) g_emb) != 0. A (problem, member) pair of a run
  becomes a record unless ds == 0 and cr == 0; the pairs are taken sixteen at a time, the records streamed four at a time.
  saved (LLMREC_BPR_SAVED_FLOATS(B) = 6 B + 8 floats per problem): [0, B) coefficient | [B .. B + 2] Su, Sp, Sq | [B + 3] k |
  [B + 4 + s B + b], s = 0 .. 4: m, sigmoid(-x) (after the selection: the kept m, 0 when dropped), |u|^2, |p|^2, |q|^2.
  gather block (LLMREC_BPR_GATHER_FLOATS(P, B) = P B + 4 P + 1): [P][B] m (+inf beyond n_valid) | [P][4] Su, Sp, Sq, k | n_valid.

BOUNDS (u = 2^-24, L = ceil(d / 16); every constant was fixed before the first device run)
  Every fp32 operation rounds once, relative error <= u. A rounding that stands alone is counted as one ulp = 2 u: it reaches u |value|
  just above a power of two, and tests/test_bpr_ref_cpu.py demands that the fp32 emulation of the kernels' own order stays below HALF of
  every bound. A chain of n roundings over positive or mixed terms is counted (n + 1) u sum|terms| (+ 1: second order).
  dot, squared norm   L fmaf steps per lane and four butterfly additions: (L + 5) u sum|terms|.
  x                   fl(fl(dp - dn) + 1e-8f): dx = (L + 5) u (sum|u p| + sum|u q|) + 2 u |dp - dn| + 2 u |x|.
  m = logsigmoid(x)   fminf(x, 0) - log1pf(expf(-|x|)), e = exp(-|x|): slope <= 1 on dx; expf E_EXP = 3 ulp -> 2 E_EXP u e / (1 + e) through
                      log1p's slope; log1pf E_LOG1P = 2 ulp -> 2 E_LOG1P u log1p(e); the subtraction 2 u |m|. E_EXP and E_LOG1P are OpenCL's
                      full-profile limits, which the ROCm device library is written to meet: published limits, not properties of this code.
  s = sigmoid(-x)     1 / (1 + expf(x)): s (1 - s) (dx + 2 E_EXP u) + 4 u s (the addition and the division; llmrec_amd/build.py passes no
                      flag that relaxes division or sqrt, so both are correctly rounded).
  coefficient         fl(fl(-1 / (float)k) s): (ds + 4 u s) / k; 0 exactly when dropped.
  Su, Sp, Sq          a thread's ceil(B / 1024) additions and the ten-level tree over positive terms: sum(d nu) + (T + 1) u S, T =
                      ceil(B / 1024) + 10 (+ n_ranks where the gathered layout's per-rank sums are added in rank order).
  mf                  the same tree over the kept m: (sum(dm) + (T + 1) u sum|m|) / k + 2 u |mf|.     k == 0: NaN on both sides.
  emb                 decay ((t_u + t_p + t_q) / bsz), t = 1 / (2 S + 1e-8f): rho_t = 2 dS / (2 S + 1e-8) + 4 u; + 8 u |emb| for the two
                      additions, the division and the product.
  c = cu, cp, cq      fl(fl(fl(-4 decay) / bsz) g_emb) / fl(den den), den = fl(2 S + 1e-8f): six roundings -> rho_c = 4 dS / den + 12 u.
  ds                  fl(g_mf coefficient): |ds| rho_ds = g_mf d(coefficient) + 2 u |ds|.
  gradient element    a record adds fmaf(ds, a - b | a, fl(c self)) = T1 + T2: |T1| (rho_ds + 4 u) + |T2| (rho_c + 4 u) - the subtraction, the
                      product and the fma, each 2 u on the term it rounds. The accumulator adds N records to what the target held:
                      (2 N + C_ACC) u (|old| + sum(|T1| + |T2|)), C_ACC = 1. A row no record reaches keeps its bits (bound 0).
                      (2 N and not N: a regulariser-only run adds the SAME value c self_c N times to a partial sum that |old| dominates, so
                      every addition leaves the same rounding residue and the worst case N u is approached - the emulation reached 0.57 of
                      (N + 1) u at N = 39 - while the emulation has to stay below half. So an accumulator rounding is counted as one ulp
                      = 2 u, like every other rounding that stands alone.)
  rows3               the record's value alone: no accumulator.

EMULATIONS (float32 numpy): emu_scores / emulate walk the 16-lane fma chains, the butterfly, the 1024-slot tree (tests/_tree_ref.py) and
the scatter's ascending problem-then-slot order, with np.exp / np.log1p in float32 standing in for the device functions. They exist to
check the bounds and to carry the mutants, not to be matched bit for bit.
"""
from __future__ import annotations

import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

from tests._dense_ref import fma32
from tests._select_ref import k_of
from tests._tree_ref import tree_lds

U = 2.0 ** -24
E_EXP, E_LOG1P = 3, 2                                 # ulp allowed to expf / log1pf (OpenCL full profile)
C_ACC = 1
EPS32 = float(np.float32(1e-8))                       # "1e-8f": both epsilons as the kernels hold them
SENTINEL = 12345.0
GUARD = 64
MAX_B, MAX_PROBLEMS = 4096, 8
SHARDED_MULTI_CAP, SHARDED_PRUNE_CAP = 4 * MAX_B, 3 * MAX_B
TREE = 1024
ROWS_BLOCKS, ROWS_PER_BLOCK = 2048, 16                # bpr_bwd_rows_kernel: grid_for(B_max, 16), sixteen rows per block
BIG_ROWS = ROWS_BLOCKS * ROWS_PER_BLOCK + 19
EUNSUPPORTED, EINVAL = -4, -1
f32, f64 = np.float32, np.float64


def ceil_div(a, b):
    return -(-a // b)


def _ceil4(x):
    return (x + 3) // 4 * 4


def saved_floats(B):
    return 6 * B + 8


def gather_floats(P, B):
    return P * B + 4 * P + 1


def plan_words(B):
    return 5 * B


class Saved:
    """views of one problem's `saved` block"""

    def __init__(self, flat, B):
        assert len(flat) == saved_floats(B)
        self.coef, self.S, self.k = flat[:B], flat[B:B + 3], flat[B + 3]
        self.m, self.sg, self.nu, self.np, self.nq = (flat[B + 4 + s * B:B + 4 + (s + 1) * B] for s in range(5))
        self.tail = flat[6 * B + 4:]                              # four floats no kernel names


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------------
def layout_spec(name, d):
    """(ld, first column, base address mod 16) of a [rows, d] view inside its allocation"""
    if name == "contig":
        return d, 0, 0
    if name == "pad":
        return _ceil4(d) + 4, 0, 0                               # ld > d, still float4 rows when d % 4 == 0
    if name == "odd":
        return (d + 1 if (d + 1) % 4 else d + 2), 0, 0           # ld % 4 != 0
    if name == "mis":
        return _ceil4(d) + 4, 1, 4                               # base 4 bytes past a 16-byte boundary, ld % 4 == 0
    raise KeyError(name)


OPERANDS = ("Eu", "Ei", "dEu", "dEi")


class Prob(NamedTuple):
    g_mf: float
    g_emb: float
    tu: int                                                       # target group of dEu (equal ids: the same buffer)
    ti: int
    lay: Tuple[str, str, str, str] = ("contig",) * 4              # per OPERANDS


def vec_of(d, probs):
    ok = d % 4 == 0
    for p in probs:
        for name in p.lay:
            ld, _, mod = layout_spec(name, d)
            ok = ok and ld % 4 == 0 and mod % 16 == 0
    return ok


def nv_of(d):
    return 1 if d <= 64 else 2


def passes_of(d):
    return ceil_div(d, 64 * nv_of(d))


def base_of(decay, flag, g_emb):
    return f32(f32(f32(-4.0) * f32(decay)) / f32(flag)) * f32(g_emb)


def groups(probs, side):
    """[(owner, [members ascending])] in launch order: the first problem with a target sums every later one with it"""
    key = [p.tu if side == "u" else p.ti for p in probs]
    return [(i, [j for j in range(i, len(probs)) if key[j] == key[i]]) for i in range(len(probs)) if key[i] not in key[:i]]


def any_reg(probs, members, decay, flag):
    return any(base_of(decay, flag, probs[j].g_emb) != 0 for j in members)


ALL_INSTANCES = {(v, n, item, reg) for v in (True, False) for n in (1, 2) for item in (False, True) for reg in (False, True)}
TRIGGERS = tuple((o, w) for w in ("odd", "mis") for o in OPERANDS)


# the refusal clauses (one restated rule each; the codes of include/llmrec_hip.h)
def refuse_cap(B_max):                                            # every forward / plan / select entry
    return EUNSUPPORTED if B_max > MAX_B else 0


def refuse_n_problems(n):
    return 0 if 1 <= n <= MAX_PROBLEMS else EINVAL


def refuse_ld(ld, d):
    return EINVAL if ld < d else 0


def refuse_null(ptr):
    return EINVAL if not ptr else 0


def refuse_same_target(dEu, dEi):                                 # llmrec_bpr_prune_bwd_f32
    return EINVAL if dEu == dEi else 0


def refuse_phase(phase):
    return 0 if phase in (1, 2) else EINVAL


def refuse_rank_stride(stride, P, B_max):
    return EINVAL if stride < gather_floats(P, B_max) else 0


def refuse_sharded_capacity(n_ranks, B_max):
    return EUNSUPPORTED if n_ranks * B_max > SHARDED_MULTI_CAP else 0


def refuse_global_batch(global_B):                                # llmrec_bpr_prune_fwd_sharded_f32
    return EUNSUPPORTED if global_B > SHARDED_PRUNE_CAP else 0


REFUSALS = ("B_max 4097", "n_problems 0", "n_problems 9", "ld < d", "null table", "dEu == dEi", "phase 3", "short rank_stride",
            "n_ranks B_max > 16384", "global_B > 3 4096")


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
FLOWS = {"prune": ("llmrec_bpr_prune_fwd_f32", "llmrec_bpr_prune_bwd_f32"),
         "multi": ("llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_bwd_f32"),
         "fused": ("llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_select_bwd_f32", "llmrec_bpr_multi_losses_f32"),
         "sharded": ("llmrec_bpr_multi_fwd_sharded_f32", "llmrec_bpr_multi_bwd_f32"),
         "prune_sharded": ("llmrec_bpr_prune_fwd_sharded_f32", "llmrec_bpr_prune_bwd_f32"),
         "rows": ("llmrec_bpr_prune_fwd_f32", "llmrec_bpr_prune_bwd_rows_f32"),
         "rows_big": ("llmrec_bpr_prune_bwd_rows_f32",),
         "zero": ("llmrec_bpr_multi_fwd_f32", "llmrec_bpr_multi_bwd_f32", "llmrec_bpr_multi_zero_rows_f32")}
ENTRY_POINTS = {e for v in FLOWS.values() for e in v}
REGIMES = ("mf", "reg", "bal")
G_MF = 0.7
RUN_EDGES = (1, 3, 4, 5, 15, 16, 17, 33)
RUN_LENS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33)                  # the crafted list: user id i occurs RUN_LENS[i] times
WIDTHS = (4, 16, 17, 20, 64, 65, 68, 100, 128, 129, 132, 200)
BATCHES = (1, 15, 16, 17, 33, 1023, 1024, 1025, 1126)


class Case(NamedTuple):
    name: str
    flow: str
    d: int
    B: Tuple[int, ...]                                            # B_max per rank
    n_valid: Tuple[Optional[int], ...]                            # per rank; None: no device count (the whole capacity)
    n_users: int
    n_items: int
    probs: Tuple[Prob, ...]
    regime: str
    remember: Optional[float]                                     # None: a tie case - inputs() places the threshold inside the tie group
    idx: str = "random"                                           # random | runs | self | triple
    seed: int = 0
    decay: float = 1.0
    flag: float = 1.0

    @property
    def P(self):
        return len(self.probs)

    def valid(self, r):
        n = self.n_valid[r]
        return self.B[r] if n is None else min(max(n, 0), self.B[r])    # bpr_batch's clamp

    def instances(self):
        vec, nv = vec_of(self.d, self.probs), nv_of(self.d)
        return {(vec, nv, side == "i", any_reg(self.probs, mem, self.decay, self.flag)) for side in "ui" for _, mem in groups(self.probs, side)}


def g_emb_for(B, d, k):
    """the regulariser's weight of the balanced regime: decay = flag = 1, tables x 0.3, so that |c self| is of the size of |ds (p - q)|
    (c = 4 g_emb / (2 S)^2, S ~ 0.09 B d; |ds| ~ 0.35 / k)"""
    return float(f32(0.004 * B * B * d * d / max(k, 1)))


def _probs(P, regime, B, d, k, tu=None, ti=None, lays=None, regimes=None):
    out = []
    for j in range(P):
        reg = regimes[j] if regimes else regime
        out.append(Prob(0.0 if reg == "reg" else G_MF * (1 + 0.25 * j), 0.0 if reg == "mf" else g_emb_for(B, d, k) * (1 + 0.5 * j),
                        tu[j] if tu else j, ti[j] if ti else j, lays[j] if lays else ("contig",) * 4))
    return tuple(out)


def _case(name, flow, d, B, regime, remember=0.29, P=1, n_valid=None, n_users=12, n_items=20, idx="random", seed=0, **kw):
    B = B if isinstance(B, tuple) else (B,)
    n_valid = n_valid if isinstance(n_valid, tuple) else (n_valid,) * len(B)
    total = sum(b if n is None else min(max(n, 0), b) for b, n in zip(B, n_valid))
    k = k_of(remember if remember is not None else 0.5, max(total, 1))
    B_S = max(total, 1) / (len(B) if flow == "prune_sharded" else 1)      # (the single-problem sharded form keeps LOCAL norm sums)
    probs = _probs(P, regime, B_S, d, k, **kw)
    return Case(name, flow, d, B, n_valid, n_users, n_items, probs, regime, remember, idx, seed)


def _lay(**kw):
    return tuple(kw.get(o, "contig") for o in OPERANDS)


def cases():
    out = []
    flows = ("multi", "fused", "prune")
    for i, d in enumerate(WIDTHS):                                # widths x regimes: the float4 instances where d % 4 == 0, else the scalar ones
        for j, regime in enumerate(REGIMES):
            out.append(_case("w%d_%s" % (d, regime), flows[(i + j) % 3], d, 40, regime))
    for d in (64, 128):                                           # ld > d keeps the float4 rows
        out.append(_case("pad%d" % d, "multi", d, 40, "bal", lays=[("pad",) * 4]))
    for d, ops in ((64, OPERANDS), (128, ("Ei", "dEu"))):         # each scalar trigger alone on an otherwise float4 shape
        for o in ops:
            for w in ("odd", "mis"):
                out.append(_case("%s_%s_%d" % (w, o, d), "multi" if o[0] == "d" else "fused", d, 40, "bal", lays=[_lay(**{o: w})]))
    out.append(_case("mis_p1_64", "multi", 64, 40, "bal", P=2, lays=[("contig",) * 4, _lay(Ei="mis")]))   # ... on the second problem only
    for B in BATCHES:                                             # the sixteen-sample blocks and both sides of the 1024-slot tree
        big = B > 1000
        out.append(_case("b%d" % B, "fused" if B % 2 else "multi", 16, B, "bal", n_users=24 if big else 12, n_items=40 if big else 20, seed=1))
    out.append(_case("b1126_mf", "prune", 16, 1126, "mf", n_users=24, n_items=40))
    out.append(_case("b1025_reg", "multi", 20, 1025, "reg", n_users=24, n_items=40))
    for name, nv in (("nv25", 25), ("nv0", 0), ("nv_over", 50), ("nv_neg", -3)):     # bpr_batch: clamped to [0, B_max]
        out.append(_case(name, "fused", 16, 40, "bal", n_valid=nv))
        out.append(_case(name + "_rows", "rows", 20, 40, "bal", n_valid=nv))
    out.append(_case("nv25_prune", "prune", 68, 40, "bal", n_valid=25))
    for regime in REGIMES:                                        # crafted runs, one problem: the run lengths themselves
        out.append(_case("runs_%s" % regime, "multi", 16, sum(RUN_LENS), regime, idx="runs"))
    out.append(_case("runs_scalar", "prune", 17, sum(RUN_LENS), "bal", idx="runs"))
    out.append(_case("runs_nv2", "fused", 132, sum(RUN_LENS), "bal", idx="runs"))
    out.append(_case("runs_p2", "multi", 16, sum(RUN_LENS), "bal", idx="runs", P=2, tu=[0, 0], ti=[0, 0]))             # totals 2 len: 16, 32
    out.append(_case("runs_step", "fused", 64, sum(RUN_LENS), "bal", idx="runs", P=5, tu=[0] * 5, seed=1))                     # the step: five share dEu
    out.append(_case("step_mf", "fused", 68, 70, "mf", P=5, tu=[0] * 5))
    out.append(_case("owner1", "multi", 20, 40, "bal", P=3, tu=[0, 1, 1], ti=[0, 1, 0]))                              # an owner that is not problem 0
    out.append(_case("mixed_reg", "multi", 64, 40, "bal", P=2, tu=[0, 0], ti=[0, 0], regimes=["mf", "bal"]))           # g_emb = 0 and != 0 in one group
    out.append(_case("p8", "fused", 100, 33, "bal", P=8, tu=[0, 0, 0, 0, 0, 1, 2, 3],
                     regimes=["bal", "mf", "bal", "reg", "bal", "mf", "reg", "bal"]))
    out.append(_case("p8_vec", "multi", 128, 17, "bal", P=8, tu=[0, 0, 0, 0, 0, 1, 2, 3], regimes=["bal"] * 5 + ["mf", "reg", "bal"]))
    out.append(_case("k0", "prune", 64, 40, "reg", remember=0.001))      # k == 0: mf is NaN, the gradient is the regulariser alone
    out.append(_case("k0_bal", "multi", 17, 40, "bal", remember=0.001))
    out.append(_case("k0_rows", "rows", 16, 40, "bal", remember=0.001))
    out.append(_case("keep_all", "multi", 16, 40, "bal", remember=1.0))
    for flow, d in (("prune", 16), ("fused", 65)):                # exact ties, the threshold inside the tie group
        out.append(_case("self_%s" % flow, flow, d, 40, "bal", remember=None, idx="self"))
        out.append(_case("triple_%s" % flow, flow, d, 40, "bal", remember=None, idx="triple"))
    out.append(_case("sharded", "sharded", 64, (40, 40, 40), "bal", P=2, n_valid=(25, 0, 40), tu=[0, 0]))
    out.append(_case("sharded_self", "sharded", 20, (24, 24, 24), "bal", remember=None, n_valid=(20, 0, 24), idx="self"))
    out.append(_case("prune_sharded", "prune_sharded", 16, (17, 16, 24), "bal"))
    out.append(_case("prune_sharded_triple", "prune_sharded", 68, (17, 16, 24), "bal", remember=None, idx="triple"))
    for d, regime in ((16, "bal"), (129, "bal"), (64, "mf"), (200, "reg")):
        out.append(_case("rows%d_%s" % (d, regime), "rows", d, 70, regime, n_valid=61))
    out.append(_case("rows_big", "rows_big", 4, BIG_ROWS, "bal", n_valid=BIG_ROWS - 40, n_users=24, n_items=40))
    out.append(_case("zero", "zero", 68, 40, "bal", P=2, n_valid=25, tu=[0, 0], n_users=24, n_items=40))
    assert len({c.name for c in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
class Inputs(NamedTuple):
    case: Case
    Eu: list                                                      # per problem [n_users, d] float32
    Ei: list
    idx: list                                                     # per rank (users, pos, neg) int64 [B_max]
    init_u: dict                                                  # target group -> [n_users, d] float32: what the target holds before
    init_i: dict
    remember: float
    tie: list                                                     # per rank int64 [B_max]: the exact-tie class of a sample, -1 - b: none


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _indices(case, r):
    B, n_u, n_i = case.B[r], case.n_users, case.n_items
    rng = _rng("idx", case.name, case.seed, r)
    u, p, q = rng.integers(0, n_u, B), rng.integers(0, n_i, B), rng.integers(0, n_i, B)
    tie = -1 - np.arange(B, dtype=np.int64)
    if case.idx == "runs":
        assert B == sum(RUN_LENS) and n_u >= len(RUN_LENS) and n_i >= len(RUN_LENS) + 4
        u = np.repeat(np.arange(len(RUN_LENS)), RUN_LENS)
        p = np.repeat(np.arange(len(RUN_LENS))[::-1], RUN_LENS[::-1])     # the same run lengths on other samples
        q = rng.integers(len(RUN_LENS), n_i, B)                           # negatives: ids no positive has
        perm = rng.permutation(B)
        u, p, q = u[perm], p[perm], q[perm]
        a = int(np.flatnonzero(p == RUN_LENS.index(2))[0])                # an item positive here ...
        b = int(np.flatnonzero(p == RUN_LENS.index(3))[0])
        q[b] = p[a]                                                       # ... and negative there: its run is 2 + 1
        c = int(np.flatnonzero(p == RUN_LENS.index(7))[1])
        q[c] = p[c]                                                       # positive and negative are the same item: its run is 7 + 1
    elif case.idx == "self":
        sel = np.arange(B) % 5 == 2 if len(case.B) > 1 else (np.arange(B) >= 5) & (np.arange(B) < 13)
        q = np.where(sel, p, q)
        q = np.where(~sel & (q == p), (q + 1) % n_i, q)
    elif case.idx == "triple":
        sel = np.arange(B) % 6 == 1 if len(case.B) > 1 else (np.arange(B) >= 20) & (np.arange(B) < 26)
        u, p, q = np.where(sel, 3, u), np.where(sel, 7, p), np.where(sel, 11, q)
    self_tie = p == q                                                 # dp and dn are computed identically: x = fl(1e-8) exactly
    key = (u * n_i + p) * n_i + q
    tie = np.where(self_tie, 1 << 40, key)                            # equal class <=> bit-equal m on any device
    return u.astype(np.int64), p.astype(np.int64), q.astype(np.int64), tie.astype(np.int64)


def inputs(case):
    d = case.d
    Eu = [(_rng("Eu", case.name, j).standard_normal((case.n_users, d)) * 0.3).astype(f32) for j in range(case.P)]
    Ei = [(_rng("Ei", case.name, j).standard_normal((case.n_items, d)) * 0.3).astype(f32) for j in range(case.P)]
    idx, tie = [], []
    for r in range(len(case.B)):
        u, p, q, t = _indices(case, r)
        idx.append((u, p, q)); tie.append(t)
    init_u = {g: (_rng("du", case.name, g).standard_normal((case.n_users, d)) * 0.01).astype(f32) for g in {p.tu for p in case.probs}}
    init_i = {g: (_rng("di", case.name, g).standard_normal((case.n_items, d)) * 0.01).astype(f32) for g in {p.ti for p in case.probs}}
    remember = case.remember
    if remember is None:                                              # the threshold goes inside the tie group (decided from the fp64 scores alone)
        ms, ts = [], []
        for r in range(len(case.B)):
            n = case.valid(r)
            ms.append(scores(Eu[0], Ei[0], *(a[:n] for a in idx[r]), d)["m"][0]); ts.append(tie[r][:n])
        m, t = np.concatenate(ms), np.concatenate(ts)
        cls, cnt = np.unique(t, return_counts=True)
        grp = t == cls[np.argmax(cnt)]
        assert grp.sum() >= 4 and np.ptp(m[grp]) == 0
        k = int((m < m[grp][0]).sum()) + int(grp.sum()) // 2
        remember = (k + 0.5) / len(m)
        assert k_of(remember, len(m)) == k
    return Inputs(case, Eu, Ei, idx, init_u, init_i, float(remember), tie)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b), (c) the fp64 reference and its bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def scores(Eu, Ei, users, pos, neg, d):
    """name -> (value, bound) over the samples: x, m, sg, nu, np, nq"""
    u, p, q = Eu[users].astype(f64), Ei[pos].astype(f64), Ei[neg].astype(f64)
    L = ceil_div(d, 16)
    dp, dn = (u * p).sum(1), (u * q).sum(1)
    x = dp - dn + EPS32
    dx = (L + 5) * U * (np.abs(u * p).sum(1) + np.abs(u * q).sum(1)) + 2 * U * np.abs(dp - dn) + 2 * U * np.abs(x)
    e = np.exp(-np.abs(x))
    m = np.minimum(x, 0) - np.log1p(e)
    dm = dx + 2 * E_EXP * U * e / (1 + e) + 2 * E_LOG1P * U * np.log1p(e) + 2 * U * np.abs(m)
    sg = np.where(x >= 0, e / (1 + e), 1 / (1 + e))
    dsg = sg * ((1 - sg) * (dx + 2 * E_EXP * U) + 4 * U)
    out = {"x": (x, dx), "m": (m, dm), "sg": (sg, dsg)}
    for k, v in (("nu", u), ("np", p), ("nq", q)):
        n = (v * v).sum(1)
        out[k] = (n, (L + 5) * U * n)
    return out


def _select(m32, k, tie_low=True, shift=False):
    """bool: the k smallest, ties by lower index (mutants: by higher index; the (k + 1)-th in place of the k-th)"""
    n = len(m32)
    canon = np.where(m32 == 0, f32(0), m32)
    order = np.lexsort((np.arange(n) if tie_low else -np.arange(n), canon))
    keep = np.zeros(n, dtype=bool)
    k = min(max(k, 0), n)
    keep[order[:k]] = True
    if shift and 0 < k < n:
        keep[order[k - 1]], keep[order[k]] = False, True
    return keep


def reference(inp, local_S=None):
    """per rank a dict name -> (value, bound); what the device must hold after the case's flow. The selection is over the concatenation of
    the ranks' valid samples; the norm sums are global for the multi-problem gathered layout and local for the single-problem one."""
    case = inp.case
    d, P, R = case.d, case.P, len(case.B)
    local_S = case.flow == "prune_sharded" if local_S is None else local_S
    dec, flag = float(f32(case.decay)), float(f32(case.flag))
    nval = [case.valid(r) for r in range(R)]
    Bg = sum(nval)
    k = k_of(inp.remember, Bg)
    sc = [[scores(inp.Eu[j], inp.Ei[j], *(a[:nval[r]] for a in inp.idx[r]), d) for j in range(P)] for r in range(R)]
    off = np.concatenate([[0], np.cumsum(nval)])
    Tadd = max(ceil_div(max(n, 1), TREE) for n in nval) + 10
    keep_g, S_g, dS_g = [], [], []
    for j in range(P):
        mg = np.concatenate([sc[r][j]["m"][0] for r in range(R)])
        keep_g.append(_select(mg.astype(f32), k))
        S = np.array([[sc[r][j][n][0].sum() for n in ("nu", "np", "nq")] for r in range(R)])
        dS = np.array([[sc[r][j][n][1].sum() for n in ("nu", "np", "nq")] for r in range(R)]) + (Tadd + 1) * U * S
        S_g.append((S, dS))
    res = []
    for r in range(R):
        n, B = nval[r], case.B[r]
        users, pos, neg = (a[:n] for a in inp.idx[r])
        out = {"k": k, "n": n}
        for name in ("m", "sg", "nu", "np", "nq"):
            out[name] = (np.stack([sc[r][j][name][0] for j in range(P)]), np.stack([sc[r][j][name][1] for j in range(P)]))
        keep = np.stack([keep_g[j][off[r]:off[r + 1]] for j in range(P)])
        out["keep"] = keep
        sg, dsg = out["sg"]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["coef"] = (np.where(keep, -sg / k, 0.0), np.where(keep, (dsg + 4 * U * sg) / k, 0.0))
            m, dm = out["m"]
            out["kept_m"] = (np.where(keep, m, 0.0), np.where(keep, dm, 0.0))
            mf = -(np.where(keep, m, 0.0).sum(1)) / k if k > 0 else np.full(P, np.nan)
            out["mf"] = (mf, (np.where(keep, dm, 0.0).sum(1) + (Tadd + 1) * U * np.where(keep, np.abs(m), 0.0).sum(1)) / max(k, 1) + 2 * U * np.abs(mf))
        S = np.stack([S_g[j][0][r] if local_S else S_g[j][0].sum(0) for j in range(P)])
        dS = np.stack([S_g[j][1][r] if local_S else S_g[j][1].sum(0) + R * U * S_g[j][0].sum(0) for j in range(P)])
        out["S"] = (S, dS)
        out["S_local"] = (np.stack([S_g[j][0][r] for j in range(P)]), np.stack([S_g[j][1][r] for j in range(P)]))
        den = 2 * S + EPS32
        t = 1 / den
        rho_t = 2 * dS / den + 4 * U
        emb = dec * t.sum(1) / flag
        out["emb"] = (emb, dec / flag * (t * rho_t).sum(1) + 8 * U * np.abs(emb))
        # the gradient: dense targets and compact rows
        dense = case.flow not in ("rows", "rows_big")
        rho_c = 4 * dS / den + 12 * U
        c = np.stack([float(base_of(case.decay, case.flag, case.probs[j].g_emb)) / den[j] ** 2 for j in range(P)])      # [P, 3]: cu, cp, cq
        coef, dcoef = out["coef"]
        for side, init, n_rows in (("u", inp.init_u, case.n_users), ("i", inp.init_i, case.n_items)):
            for owner, mem in groups(case.probs, side) if dense else ():
                gid = case.probs[owner].tu if side == "u" else case.probs[owner].ti
                G, E, M1, M2, N = [np.zeros((n_rows, d)) for _ in range(4)] + [np.zeros(n_rows)]
                for j in mem:
                    g_mf = float(f32(case.probs[j].g_mf))
                    ds, dds = g_mf * coef[j], g_mf * dcoef[j] + 2 * U * np.abs(g_mf * coef[j])
                    uu, pp, qq = inp.Eu[j][users].astype(f64), inp.Ei[j][pos].astype(f64), inp.Ei[j][neg].astype(f64)
                    parts = [(users, ds, pp - qq, 0, uu)] if side == "u" else [(pos, ds, uu, 1, pp), (neg, -ds, uu, 2, qq)]
                    for ids, s, a, ci, self_ in parts:
                        T1, T2 = s[:, None] * a, c[j, ci] * self_
                        err = dds[:, None] * np.abs(a) + 4 * U * np.abs(T1) + np.abs(T2) * (rho_c[j, ci] + 4 * U)
                        act = ~((s == 0) & (c[j, ci] == 0))
                        np.add.at(G, ids, T1 + T2); np.add.at(E, ids, err)
                        np.add.at(M1, ids, np.abs(T1)); np.add.at(M2, ids, np.abs(T2)); np.add.at(N, ids, act.astype(f64))
                old = init[gid].astype(f64)
                bound = np.where(N[:, None] > 0, E + (2 * N[:, None] + C_ACC) * U * (np.abs(old) + M1 + M2), 0.0)
                out["dE%s%d" % (side, gid)] = (old + G, bound)
                out["mag_%s%d" % (side, gid)] = (M1, M2)
        if P == 1:
            rows = rows3_ref(inp.Eu[0], inp.Ei[0], users, pos, neg, float(f32(case.probs[0].g_mf)), coef[0], dcoef[0], c[0], rho_c[0])
            val, bnd = np.zeros((3, B, d)), np.zeros((3, B, d))
            val[:, :n], bnd[:, :n] = rows
            out["rows3"] = (val, bnd)
        res.append(out)
    return res


def rows3_ref(Eu, Ei, users, pos, neg, g_mf, coef, dcoef, c, rho_c):
    """(value, bound) [3, n, d]: d/dEu[u_b], d/dEi[p_b], d/dEi[q_b] of every sample on its own"""
    uu, pp, qq = Eu[users].astype(f64), Ei[pos].astype(f64), Ei[neg].astype(f64)
    ds, dds = g_mf * coef, g_mf * dcoef + 2 * U * np.abs(g_mf * coef)
    val, bnd = [], []
    for s, a, ci, self_ in ((ds, pp - qq, 0, uu), (ds, uu, 1, pp), (-ds, uu, 2, qq)):
        T1, T2 = s[:, None] * a, c[ci] * self_
        val.append(T1 + T2)
        bnd.append(dds[:, None] * np.abs(a) + 4 * U * np.abs(T1) + np.abs(T2) * (rho_c[ci] + 4 * U))
    return np.stack(val), np.stack(bnd)


def selection_margin(inp, ref=None):
    """the smallest (fp64 gap at the threshold) / (m bound) over the problems, exact ties excepted: >= 4 means no fp32 evaluation inside the
    bounds can decide differently from the reference. inf: nothing to decide (k <= 0, k >= Bg, or the threshold lies inside a tie class)."""
    case = inp.case
    ref = ref or reference(inp)
    worst = np.inf
    tie = np.concatenate([inp.tie[r][:ref[r]["n"]] for r in range(len(ref))])
    k = ref[0]["k"]
    for j in range(case.P):
        m = np.concatenate([o["m"][0][j] for o in ref])
        dm = np.concatenate([o["m"][1][j] for o in ref])
        if not 0 < k < len(m):
            continue
        order = np.lexsort((np.arange(len(m)), m))
        a, b = order[k - 1], order[k]
        if tie[a] == tie[b]:
            assert m[a] == m[b]
            lo = order[:k][tie[order[:k]] != tie[a]]                  # the neighbours outside the class must be clear of it too
            hi = order[k:][tie[order[k:]] != tie[a]]
            gaps = [(m[a] - m[i]) / max(dm[a], dm[i]) for i in lo[-1:]] + [(m[i] - m[a]) / max(dm[a], dm[i]) for i in hi[:1]]
            worst = min([worst] + gaps)
            continue
        worst = min(worst, (m[b] - m[a]) / max(dm[a], dm[b]))
    return worst


def balance(ref_rank, probs):
    """(min, max) over the destination rows that receive both shares of sum|c self| / sum|ds (.)|"""
    lo, hi = np.inf, 0.0
    for key, val in ref_rank.items():
        if key.startswith("mag_"):
            M1, M2 = val[0].sum(1), val[1].sum(1)
            both = (M1 > 0) & (M2 > 0)
            if both.any():
                r = M2[both] / M1[both]
                lo, hi = min(lo, r.min()), max(hi, r.max())
    return lo, hi


# ------------------------------------------------------------------------------------------------------------------------------------
# (g) the fp32 emulations of the kernels' own order, and the mutants
# ------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("reg_deleted", "reg_sign", "reg_x10", "cp_cq_swap", "neg_ds_sign", "keep_next", "tie_high", "no_eps", "drop_17th", "overwrite",
           "rows3_swap")


def _butterfly(v):
    lanes = np.arange(16)
    for off in (8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, 0]


def emu_scores(Eu, Ei, users, pos, neg, d, mutant=None):
    n, L = len(users), ceil_div(d, 16)
    pad = lambda a: np.concatenate([a, np.zeros((n, 16 * L - d), dtype=f32)], axis=1)
    u, p, q = pad(Eu[users]), pad(Ei[pos]), pad(Ei[neg])
    acc = [np.zeros((n, 16), dtype=f32) for _ in range(5)]
    for i in range(L):
        sl = slice(16 * i, 16 * i + 16)
        for a, (x, y) in enumerate(((u, p), (u, q), (u, u), (p, p), (q, q))):
            acc[a] = fma32(x[:, sl], y[:, sl], acc[a])
    dp, dn, nu, np_, nq = (_butterfly(a) for a in acc)
    x = dp - dn
    if mutant != "no_eps":
        x = x + f32(1e-8)
    with np.errstate(over="ignore"):
        m = np.minimum(x, f32(0)) - np.log1p(np.exp(-np.abs(x)))
        sg = f32(1) / (f32(1) + np.exp(x))
    return {"m": m.astype(f32), "sg": sg.astype(f32), "nu": nu, "np": np_, "nq": nq}


def emulate(inp, mutant=None):
    """reference()'s dict, in float32 and in the kernels' order (values only)"""
    case = inp.case
    d, P, R = case.d, case.P, len(case.B)
    local_S = case.flow == "prune_sharded"
    nval = [case.valid(r) for r in range(R)]
    Bg = sum(nval)
    k = k_of(inp.remember, Bg)
    off = np.concatenate([[0], np.cumsum(nval)])
    sc = [[emu_scores(inp.Eu[j], inp.Ei[j], *(a[:nval[r]] for a in inp.idx[r]), d, mutant) for j in range(P)] for r in range(R)]
    keep_g = [_select(np.concatenate([sc[r][j]["m"] for r in range(R)]), k, mutant != "tie_high", mutant == "keep_next") for j in range(P)]
    S_loc = [[[f32(tree_lds(sc[r][j][nm])) for nm in ("nu", "np", "nq")] for j in range(P)] for r in range(R)]
    res = []
    for r in range(R):
        n, B = nval[r], case.B[r]
        users, pos, neg = (a[:n] for a in inp.idx[r])
        out = {"k": k, "n": n}
        for name in ("m", "sg", "nu", "np", "nq"):
            out[name] = np.stack([sc[r][j][name] for j in range(P)])
        keep = np.stack([keep_g[j][off[r]:off[r + 1]] for j in range(P)])
        out["keep"] = keep
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(keep, (f32(-1.0) / f32(k)) * out["sg"], f32(0)).astype(f32)
            kept_m = np.where(keep, out["m"], f32(0)).astype(f32)
            out["mf"] = np.array([-(f32(tree_lds(kept_m[j])) / f32(k)) for j in range(P)], dtype=f32)
        out["coef"], out["kept_m"] = coef, kept_m
        S = np.zeros((P, 3), dtype=f32)
        for j in range(P):
            for i in range(3):
                if local_S or R == 1:
                    S[j, i] = S_loc[r][j][i]
                else:
                    acc = f32(0)
                    for rr in range(R):
                        acc = f32(acc + S_loc[rr][j][i])
                    S[j, i] = acc
        out["S"] = S
        out["S_local"] = np.array(S_loc[r], dtype=f32)
        dec, flag, one, two, eps = f32(case.decay), f32(case.flag), f32(1), f32(2), f32(1e-8)
        den = (two * S + eps).astype(f32)
        t = (one / den).astype(f32)
        out["emb"] = (dec * (((t[:, 0] + t[:, 1]).astype(f32) + t[:, 2]).astype(f32) / flag).astype(f32)).astype(f32)
        c = np.stack([(base_of(case.decay, case.flag, case.probs[j].g_emb) / (den[j] * den[j]).astype(f32)).astype(f32) for j in range(P)])
        if mutant == "reg_deleted":
            c = c * f32(0)
        elif mutant == "reg_sign":
            c = -c
        elif mutant == "reg_x10":
            c = c * f32(10)
        elif mutant == "cp_cq_swap":
            c = c[:, [0, 2, 1]]
        nsign = f32(1) if mutant == "neg_ds_sign" else f32(-1)
        for side, init in (("u", inp.init_u), ("i", inp.init_i)):
            for owner, mem in groups(case.probs, side) if case.flow not in ("rows", "rows_big") else ():
                gid = case.probs[owner].tu if side == "u" else case.probs[owner].ti
                T = init[gid].copy()
                if side == "u":
                    keys = [(int(users[b]), b) for b in range(n)]
                else:
                    keys = [(int(pos[b]), b) for b in range(n)] + [(int(neg[b]), B + b) for b in range(n)]
                runs = {}
                for id_, slot in sorted(keys):
                    runs.setdefault(id_, []).append(slot)
                for id_, slots in runs.items():
                    acc = np.zeros(d, dtype=f32) if mutant == "overwrite" else T[id_].copy()
                    pairs = [(j, s) for j in mem for s in slots]          # ascending problem, then ascending slot
                    if mutant == "drop_17th" and len(pairs) == 17:
                        pairs = pairs[:-1]
                    for j, slot in pairs:
                        is_neg = slot >= B
                        b = slot - B if is_neg else slot
                        ds = f32(case.probs[j].g_mf) * coef[j, b]
                        if side == "u":
                            s_, cr, a, self_ = ds, c[j, 0], inp.Ei[j][pos[b]] - inp.Ei[j][neg[b]], inp.Eu[j][id_]
                        else:
                            s_, cr, a, self_ = (nsign * ds if is_neg else ds), (c[j, 2] if is_neg else c[j, 1]), inp.Eu[j][users[b]], inp.Ei[j][id_]
                        if ds == 0 and cr == 0:
                            continue
                        acc = acc + fma32(np.full(d, s_, dtype=f32), a.astype(f32), (cr * self_).astype(f32))
                    T[id_] = acc
                out["dE%s%d" % (side, gid)] = T
        if P == 1:
            rows = np.zeros((3, B, d), dtype=f32)
            uu, pp, qq = inp.Eu[0][users], inp.Ei[0][pos], inp.Ei[0][neg]
            ds = (f32(case.probs[0].g_mf) * coef[0]).astype(f32)[:, None] * np.ones((1, d), dtype=f32)
            rows[0, :n] = fma32(ds, pp - qq, c[0, 0] * uu)
            rows[1, :n] = fma32(ds, uu, c[0, 1] * pp)
            rows[2, :n] = fma32(nsign * ds, uu, c[0, 2] * qq)
            if mutant == "rows3_swap":
                rows = rows[[0, 2, 1]]
            out["rows3"] = rows
        res.append(out)
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison (shared by the CPU soundness test and the device test)
# ------------------------------------------------------------------------------------------------------------------------------------
GROUPS = {"m": "scores", "sg": "scores", "nu": "norms", "np": "norms", "nq": "norms", "coef": "coef", "kept_m": "scores", "S": "S",
          "S_local": "S", "mf": "mf", "emb": "emb", "rows3": "rows3"}


def group_of(key):
    return GROUPS.get(key) or ("dEu" if key.startswith("dEu") else "dEi")


def ratio(got, want, bound):
    """the worst |got - want| / bound; where the bound is 0 the values must be equal; NaN must meet NaN"""
    got, want, bound = np.broadcast_arrays(np.asarray(got, dtype=f64), np.asarray(want, dtype=f64), np.asarray(bound, dtype=f64))
    if got.size == 0:
        return 0.0
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(both_nan, 0.0, np.where(np.isfinite(r), r, np.inf))
    return float(r.max())


def ratios(got, ref, keys=None):
    """group -> the worst error / bound of what `got` (one rank: name -> values) holds, against reference()'s dict of that rank"""
    out = {}
    for key, val in got.items():
        if key not in ref or not isinstance(ref[key], tuple) or key.startswith("mag_") or (keys and key not in keys):
            continue
        g = group_of(key)
        out[g] = max(out.get(g, 0.0), ratio(val, *ref[key]))
    return out
