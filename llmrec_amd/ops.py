"""Host side of the C ABI: device-CSR operands and torch.autograd Functions over the HIP kernels.

Everything here is plumbing: tensors stay torch-owned, kernels receive ``tensor.data_ptr()`` and
the hipStream_t of torch's current stream (so launches are ordered with torch's own work and can
be captured in a HIP graph). No function in this module computes on the CPU or falls back to
torch math: if the HIP library is missing or a tensor is not on the GPU, it raises.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib

CONST = _lib.CONST
_c = ctypes


def _stream():
    return _c.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else _c.c_void_p(t.data_ptr())


def _ptr(t: Optional[torch.Tensor]):
    """a tensor's address for a pointer field of a ctypes struct (None = NULL)"""
    return None if t is None else t.data_ptr()


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("llmrec_amd: the HIP path needs GPU tensors; got a %s tensor "
                               "(there is no CPU fallback)" % t.device)


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    """2-D fp32 view whose inner stride is 1 (copy only if it is not)."""
    if t.dtype != torch.float32:
        raise RuntimeError("llmrec_amd: fp32 expected, got %s" % t.dtype)
    if t.dim() != 2:
        raise RuntimeError("llmrec_amd: 2-D tensor expected")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


# ---------------------------------------------------------------------------------------------
# R1: CSR operands
# ---------------------------------------------------------------------------------------------
# The argument blocks of include/llmrec_hip.h, bound from the header itself (_lib.parse_structs): fields in the header's order, every pointer
# a c_void_p (an int address, None, a ctypes array or addressof)
SpmmPlanC = _lib.STRUCT["llmrec_spmm_plan_t"]
SpmmEpilogueC = _lib.STRUCT["llmrec_spmm_epilogue_t"]
SpmmProblemC = _lib.STRUCT["llmrec_spmm_problem_t"]              # the arguments of one llmrec_spmm_f32 call, for llmrec_spmm_multi_f32
GuestSamplerC = _lib.STRUCT["llmrec_guest_sampler_t"]            # the arguments of llmrec_sample_batch_wide
GuestPlanReachC = _lib.STRUCT["llmrec_guest_plan_reach_t"]       # the arguments of llmrec_bpr_scatter_plan_reach_mark
GuestLossesC = _lib.STRUCT["llmrec_guest_losses_t"]              # the arguments of llmrec_bpr_multi_losses_assemble_f32


class SpmmGuestC(_lib.STRUCT["llmrec_spmm_guest_t"]):
    """llmrec_spmm_guest_t: the tagged guest of llmrec_spmm_multi_guest_f32. keep: host arrays the descriptor points into."""
    keep = None


GUEST_SAMPLER, GUEST_PLAN_REACH, GUEST_LOSSES = (CONST["LLMREC_SPMM_GUEST_" + k] for k in ("SAMPLER", "PLAN_REACH", "LOSSES"))
EPI_NONE, EPI_SOFTMAX, EPI_SOFTMAX_BWD = (CONST["LLMREC_SPMM_EPI_" + k] for k in ("NONE", "SOFTMAX", "SOFTMAX_BWD"))
SPMM_LATENCY_NNZ = 4_000_000      # below: the graph is L2-resident and a step is launch-bound (Netflix scale)


def spmm_shape(d: int, nnz: int, whole_row: bool = False):
    """(slice_width, (t_wave, t_block, segment)) for llmrec_spmm_f32: the latency / throughput policy.
    Launch-bound graphs (nnz < SPMM_LATENCY_NNZ): the longest dependent gather chain of any wave sets a kernel's
    duration, so a lane group gets at most 32 nnz (wavefront bucket) / 64 nnz (block bucket), and wide operands whose
    width is a multiple of 64 are cut into 64-column slices ((row, slice) tasks) unless an epilogue needs the whole row.
    HBM-bound graphs: 128 / 512 nnz per lane group (fewer, longer pieces; partial sums only for hubs)."""
    small = nnz < SPMM_LATENCY_NNZ
    sw = 64 if (small and not whole_row and d > 64 and d % 64 == 0) else 0
    w = sw or d
    lpr = 4
    while lpr < 64 and lpr * 4 < w:
        lpr *= 2
    groups = 64 // lpr
    if small:
        t_wave, t_block = max(32, 32 * groups), 8 * groups * 64
    else:
        t_wave, t_block = 128 * groups, 8 * groups * 512
    return sw, (t_wave, t_block, t_block)


@dataclass
class SpmmPlan:
    """Row buckets of one rowptr for one threshold triple (include/llmrec_hip.h, llmrec_spmm_plan_*)."""
    t_wave: int = 128
    t_block: int = 2048
    segment: int = 2048
    n_wave: int = 0
    n_block: int = 0
    n_split: int = 0
    n_seg: int = 0
    wave_rows: Optional[torch.Tensor] = None
    block_rows: Optional[torch.Tensor] = None
    split_rows: Optional[torch.Tensor] = None
    split_seg_begin: Optional[torch.Tensor] = None
    seg_split: Optional[torch.Tensor] = None
    # the permuted CSR (llmrec_spmm_plan_t.slot_row): rows stored in visiting order, slot -> output row; None = the operand's own CSR
    n_short: int = 0
    slot_row: Optional[torch.Tensor] = None
    p_rowptr: Optional[torch.Tensor] = None
    p_colidx: Optional[torch.Tensor] = None
    colidx_src: int = 0               # data_ptr of the colidx the permuted copy was made from

    def csr_of(self, a: "Csr"):
        """(rowptr, colidx) llmrec_spmm_f32 gets with this plan: the permuted copy when the plan has one (made from THIS operand's pattern)."""
        if self.slot_row is None:
            return a.rowptr, a.colidx
        if a.val is not None or a.colidx.data_ptr() != self.colidx_src:
            raise RuntimeError("SpmmPlan: the permuted CSR of this plan belongs to another pattern (plans are shared by operands over ONE pattern)")
        return self.p_rowptr, self.p_colidx

    @property
    def n_long(self) -> int:
        return self.n_wave + self.n_block + self.n_split

    def c_struct(self) -> SpmmPlanC:
        c = getattr(self, "_c", None)
        if c is None:
            dp = lambda t, n: t.data_ptr() if n else None
            c = self._c = SpmmPlanC(self.t_wave, self.t_block, self.segment, self.n_wave, dp(self.wave_rows, self.n_wave),
                                    self.n_block, dp(self.block_rows, self.n_block), self.n_split, dp(self.split_rows, self.n_split),
                                    dp(self.split_seg_begin, self.n_split), self.n_seg, dp(self.seg_split, self.n_split),
                                    self.n_short if self.slot_row is not None else 0, dp(self.slot_row, self.slot_row is not None))
        return c

    def scratch(self, d: int, device) -> Optional[torch.Tensor]:
        """The plan's own partial-sum scratch for width d, one per (d, current stream): plans are shared by the operands over
        one rowptr (ui.fwd / iu.bwd, iu.fwd / ui.bwd), and two SpMMs over such operands issued on different streams must
        not share the partial sums of their split rows."""
        if not self.n_seg:
            return None
        cache = self.__dict__.setdefault("_scratch", {})
        key = (d, torch.cuda.current_stream().cuda_stream)
        if key not in cache:
            cache[key] = torch.empty(self.n_seg * d, dtype=torch.float32, device=device)
        return cache[key]

    @staticmethod
    def by_length_class(rows: torch.Tensor, deg: torch.Tensor) -> torch.Tensor:
        """`rows` (ascending ids) reordered by descending length class - the power-of-two bucket of the row's nnz, empty rows last - and
        ascending id within a class (stable): rows that share a wavefront / a round of blocks then take (almost) equally long."""
        cls = torch.where(deg > 0, torch.floor(torch.log2(deg.clamp(min=1).to(torch.float64))).to(torch.int64) + 1, torch.zeros_like(deg, dtype=torch.int64))
        return rows[torch.sort(-cls, stable=True).indices].to(torch.int32).contiguous()

    @staticmethod
    def build(rowptr: torch.Tensor, t_wave: int = 128, t_block: int = 2048, segment: int = 2048, colidx: Optional[torch.Tensor] = None,
              order_rows: bool = True) -> "SpmmPlan":
        """colidx (pattern-only operands) + order_rows: the plan carries a PERMUTED copy of the CSR - every bucket's rows stored in the order
        they are visited, by descending length class (by_length_class); order_rows=False: the operand's own CSR in row order. Measured
        (profiles/experiments/r06_spmm_order.md): 2 M x 1 M x 40 M edges, d = 64: 1.65 -> 1.39 ms (rows = users), 1.14 -> 0.99 ms
        (rows = items); cfg 4 whole 57.2 -> 53.5 ms per step; the Netflix-shaped step 0.460 -> 0.447 ms. Results never
        depend on the order (bit-identical: tests/test_gpu_ops.py)."""
        n_rows = rowptr.numel() - 1
        dev = rowptr.device
        order_rows = bool(order_rows) and colidx is not None and n_rows > 0
        scratch = torch.zeros(4, dtype=torch.int32, device=dev)
        counts = (_c.c_int32 * 4)()
        _lib.call("llmrec_spmm_plan_count", n_rows, _p(rowptr), t_wave, t_block, segment, _p(scratch), counts, _stream())
        nw, nb, nsp, nseg = (int(x) for x in counts)
        wr = br = sr = sb = ss = None
        if nw + nb + nsp:
            i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            wr, br, sr, sb, ss = i32(nw), i32(nb), i32(nsp), i32(nsp), i32(nseg)
            _lib.call("llmrec_spmm_plan_fill", n_rows, _p(rowptr), t_wave, t_block, segment, _p(scratch), _p(wr), _p(br), _p(sr), _p(sb), _p(ss), _stream())
            # the fill compacts with atomics: sort the two independent row lists so that the plan (and the order rows are
            # visited in) is reproducible run to run; results never depend on the order
            wr = torch.sort(wr[:nw]).values.contiguous() if nw else None
            br = torch.sort(br[:nb]).values.contiguous() if nb else None
            sr, sb, ss = (sr, sb, ss) if nsp else (None, None, None)
        if not order_rows:
            torch.cuda.current_stream().synchronize()                  # (see below: the lists are read by every stream)
            return SpmmPlan(t_wave, t_block, segment, nw, nb, nsp, nseg, wr, br, sr, sb, ss)
        deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
        ids = torch.nonzero(deg <= CONST["LLMREC_SPMM_LONG_ROW"]).flatten()
        parts = [SpmmPlan.by_length_class(ids, deg[ids])]
        if nw:
            parts.append(SpmmPlan.by_length_class(wr.long(), deg[wr.long()]))
        if nb:
            parts.append(SpmmPlan.by_length_class(br.long(), deg[br.long()]))
        if nsp:
            parts.append(sr[:nsp])
        n_short = parts[0].numel()
        slot_row = torch.cat(parts).contiguous()                       # slot -> row
        assert slot_row.numel() == n_rows
        p_rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(deg[slot_row.long()], 0, out=p_rowptr[1:])
        p_rowptr = p_rowptr.to(torch.int32)
        p_colidx = torch.empty_like(colidx)
        _lib.call("llmrec_csr_permute_rows", n_rows, _p(rowptr), _p(colidx), _p(slot_row), _p(p_rowptr), _p(p_colidx), _stream())
        ar = lambda lo, n: torch.arange(lo, lo + n, dtype=torch.int32, device=dev) if n else None     # the lists hold slots
        lists = (ar(n_short, nw), ar(n_short + nw, nb), ar(n_short + nw + nb, nsp))
        # A plan is built lazily, on whatever stream runs the first product over its operand (a SIDE stream of the fused step's warm-up), and
        # is then shared by every stream: its arrays must be complete before any other stream reads them. (Round 6: four replica processes
        # on one GPU faulted in the first captured step - the chain's stream read a permuted CSR the profile stream was still writing.)
        torch.cuda.current_stream().synchronize()
        return SpmmPlan(t_wave, t_block, segment, nw, nb, nsp, nseg, lists[0], lists[1], lists[2], sb, ss,
                        n_short, slot_row, p_rowptr, p_colidx, colidx.data_ptr())


@dataclass
class Csr:
    """One SpMM operand: Y = diag(row_scale) (P . val) diag(col_scale) X."""
    n_rows: int
    n_cols: int
    rowptr: torch.Tensor            # int32 [n_rows + 1]
    colidx: torch.Tensor            # int32 [nnz]
    val: Optional[torch.Tensor]     # fp32 [nnz] or None (pattern only)
    row_scale: Optional[torch.Tensor]
    col_scale: Optional[torch.Tensor]
    plans: Optional[dict] = None    # {(t_wave, t_block, segment): SpmmPlan}, shared by the operands that share this rowptr

    def __post_init__(self):
        if not isinstance(self.plans, dict):
            self.plans = {}

    @property
    def nnz(self) -> int:
        return self.colidx.numel()

    def plan_for(self, d: int, whole_row: bool = False):
        """(slice_width, SpmmPlan) for an operand of width d."""
        sw, key = spmm_shape(d, self.nnz, whole_row)
        pl = self.plans.get(key)
        if pl is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                # building a plan synchronises (llmrec_spmm_plan_count returns counts to the host) - illegal under capture
                raise RuntimeError("Csr.plan_for: no row plan for (d = %d, whole_row = %s) yet and the stream is being captured; "
                                   "run the same product once eagerly (a warm-up step) before capturing" % (d, whole_row))
            pl = self.plans[key] = SpmmPlan.build(self.rowptr, *key, colidx=self.colidx if self.val is None else None)
        return sw, pl

    @property
    def plan(self) -> SpmmPlan:
        return self.plan_for(64)[1]


def csr_from_coo(rows: torch.Tensor, cols: torch.Tensor, vals: Optional[torch.Tensor], n_rows: int, n_cols: int):
    """Device COO (int64) -> (rowptr, colidx, val) with ascending columns per row."""
    _need_gpu(rows, cols, vals)
    nnz = rows.numel()
    dev = rows.device
    rows = rows.to(torch.int64).contiguous()
    cols = cols.to(torch.int64).contiguous()
    if vals is not None:
        vals = vals.to(torch.float32).contiguous()
    rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev) if vals is not None else None
    ws_bytes = _lib.query("llmrec_csr_build_workspace_bytes", n_rows, nnz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call("llmrec_csr_build", n_rows, n_cols, nnz, _p(rows), _p(cols), _p(vals), _p(rowptr), _p(colidx), _p(val),
              _p(ws), ws_bytes, _stream())
    return rowptr, colidx, val


def degree_scale(rowptr: torch.Tensor) -> torch.Tensor:
    out = torch.empty(rowptr.numel() - 1, dtype=torch.float32, device=rowptr.device)
    _lib.call("llmrec_degree_scale", out.numel(), _p(rowptr), _p(out), _stream())
    return out


@dataclass
class SparseOperand:
    """A sparse matrix A prepared for Y = A X (``fwd``) and dX = A^T dY (``bwd``)."""
    fwd: Csr
    bwd: Csr

    @property
    def shape(self):
        return (self.fwd.n_rows, self.fwd.n_cols)

    @staticmethod
    def from_coo(rows, cols, vals, n_rows: int, n_cols: int) -> "SparseOperand":
        """General path (any values). If every row's values are one constant - the reference's
        normalised adjacency diag(s) R, main.py:123-126 - the 4 B/nnz value stream is dropped."""
        rowptr, colidx, val = csr_from_coo(rows, cols, vals, n_rows, n_cols)
        t_rowptr, t_colidx, t_val = csr_from_coo(cols, rows, vals, n_cols, n_rows)
        row_const = None
        if val is not None:
            rc = torch.empty(n_rows, dtype=torch.float32, device=rowptr.device)
            flag = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
            _lib.call("llmrec_csr_row_constant", n_rows, _p(rowptr), _p(val), _p(rc), _p(flag), _stream())
            if int(flag.item()) == 1:
                row_const = rc
        plan_f, plan_b = {}, {}                                  # built lazily per piece length, shared by the operands below
        if val is None or row_const is not None:
            fwd = Csr(n_rows, n_cols, rowptr, colidx, None, row_const, None, plan_f)
            bwd = Csr(n_cols, n_rows, t_rowptr, t_colidx, None, None, row_const, plan_b)
        else:
            fwd = Csr(n_rows, n_cols, rowptr, colidx, val, None, None, plan_f)
            bwd = Csr(n_cols, n_rows, t_rowptr, t_colidx, t_val, None, None, plan_b)
        return SparseOperand(fwd, bwd)


_operand_cache = {}


def operand_from_sparse_tensor(t: torch.Tensor) -> SparseOperand:
    """Drop-in entry: accepts the torch sparse COO tensor the reference passes to
    MM_Model.forward (reference main.py:128-134) and caches the device CSR on tensor identity."""
    key = id(t)
    hit = _operand_cache.get(key)
    if hit is not None and hit[0]() is t:
        return hit[1]
    if not t.is_sparse:
        raise RuntimeError("llmrec_amd: expected a torch sparse COO tensor")
    _need_gpu(t)
    idx = t._indices()
    op = SparseOperand.from_coo(idx[0], idx[1], t._values(), t.shape[0], t.shape[1])
    _operand_cache[key] = (weakref.ref(t), op)
    return op


@dataclass
class BipartiteGraph:
    """User-item interaction pattern R with the reference's one-sided normalisation:
    A_ui = diag(s_u) R, A_iu = diag(s_i) R^T (reference main.py:84-91). Holds two pattern-only
    CSRs (by user, by item) shared by the four SpMM directions."""
    n_users: int
    n_items: int
    ui: SparseOperand
    iu: SparseOperand
    by_user: Csr            # pattern of R (train items per user, ascending) - also the eval mask
    s_u: torch.Tensor
    s_i: torch.Tensor

    @staticmethod
    def from_edges(users: torch.Tensor, items: torch.Tensor, n_users: int, n_items: int) -> "BipartiteGraph":
        ru, cu, _ = csr_from_coo(users, items, None, n_users, n_items)
        ri, ci, _ = csr_from_coo(items, users, None, n_items, n_users)
        s_u, s_i = degree_scale(ru), degree_scale(ri)
        pu, pi = {}, {}                                          # plan caches shared by the operands over ru / ri
        ui = SparseOperand(Csr(n_users, n_items, ru, cu, None, s_u, None, pu), Csr(n_items, n_users, ri, ci, None, None, s_u, pi))
        iu = SparseOperand(Csr(n_items, n_users, ri, ci, None, s_i, None, pi), Csr(n_users, n_items, ru, cu, None, None, s_i, pu))
        return BipartiteGraph(n_users, n_items, ui, iu, ui.fwd, s_u, s_i)


# ---------------------------------------------------------------------------------------------
# R2: SpMM
# ---------------------------------------------------------------------------------------------
def spmm_epilogue(op: int = EPI_NONE, alpha: float = 0.0, Z: Optional[torch.Tensor] = None, S: Optional[torch.Tensor] = None,
                  post_scale: Optional[torch.Tensor] = None, x_row_mask: Optional[torch.Tensor] = None, x_mask_active: int = 0,
                  y_row_flag: Optional[torch.Tensor] = None, z_row_flag: Optional[torch.Tensor] = None,
                  y_row_gate: Optional[torch.Tensor] = None, y_row_needed: Optional[torch.Tensor] = None, rows_listed_only: bool = False,
                  x_mask_stamp: Optional[torch.Tensor] = None, mask_from_slice: int = 0):
    """llmrec_spmm_epilogue_t: Y = post_scale . op(alpha * Z + A X); S = forward softmax rows for EPI_SOFTMAX_BWD.
    x_row_mask (uint8 [n_cols]) / x_mask_active: X rows whose byte differs from the active value are promised all-zero and not read;
    y_row_flag (uint8 [n_rows]): receives the active value for rows whose result can be non-zero (z_row_flag: the non-zero rows of Z);
    y_row_gate (uint8 [n_rows]): rows without the active value are promised zero results and written as zeros unread;
    y_row_needed (uint8 [n_rows]): rows without the active value are neither computed nor written; rows_listed_only: compute the rows
    in the plan's lists only (spmm_listed).
    x_mask_stamp (int32 [1], device) / mask_from_slice: the slice-ranged mask - in the 64-column slices from mask_from_slice on, X rows
    whose x_row_mask byte differs from LLMREC_ROW_STAMP(x_mask_stamp[0]) are promised all-zero and not read; the in-place accumulate
    then leaves rows without an active neighbour untouched in those slices. The library refuses shapes it is not compiled for."""
    if x_mask_stamp is not None and (x_mask_stamp.dtype != torch.int32 or x_row_mask is None):
        raise RuntimeError("spmm_epilogue: x_mask_stamp is an int32 device counter and needs x_row_mask")
    for t in (x_row_mask, y_row_flag, z_row_flag, y_row_gate, y_row_needed):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous()):
            raise RuntimeError("spmm_epilogue: row masks / flags are contiguous uint8 tensors")
    return SpmmEpilogueC(op, float(alpha), Z.data_ptr() if Z is not None else None, _ld(Z) if Z is not None else 0,
                         S.data_ptr() if S is not None else None, _ld(S) if S is not None else 0,
                         post_scale.data_ptr() if post_scale is not None else None,
                         x_row_mask.data_ptr() if x_row_mask is not None else None, int(x_mask_active),
                         y_row_flag.data_ptr() if y_row_flag is not None else None,
                         z_row_flag.data_ptr() if z_row_flag is not None else None,
                         y_row_gate.data_ptr() if y_row_gate is not None else None,
                         y_row_needed.data_ptr() if y_row_needed is not None else None, 1 if rows_listed_only else 0,
                         x_mask_stamp.data_ptr() if x_mask_stamp is not None else None, int(mask_from_slice))


def listed_plan(a: Csr, rows: torch.Tensor, d: int, whole_row: bool = False) -> SpmmPlan:
    """A row plan over an explicit list of DISTINCT rows (int64 device tensor): every listed row lands in the wavefront, block or split
    list by its length - with rows_listed_only the launch computes exactly these rows. Built with torch ops on the device; reading the
    three list lengths back synchronises (once per call: the row-sharded training step, whose batch decides the list)."""
    _, (t_wave, t_block, segment) = spmm_shape(d, a.nnz, whole_row)
    rp = a.rowptr
    rows = rows.to(torch.int64)
    deg = (rp[rows + 1] - rp[rows]).to(torch.int64)
    i32 = lambda t: t.to(torch.int32).contiguous()
    w = i32(rows[deg <= t_wave]); b = i32(rows[(deg > t_wave) & (deg <= t_block)])
    big = deg > t_block
    sp = i32(rows[big])
    nseg = (deg[big] + segment - 1) // segment
    seg_begin = i32(torch.cumsum(nseg, 0) - nseg)
    seg_split = i32(torch.repeat_interleave(torch.arange(sp.numel(), device=rows.device), nseg))
    return SpmmPlan(t_wave, t_block, segment, w.numel(), b.numel(), sp.numel(), seg_split.numel(), w if w.numel() else None,
                    b if b.numel() else None, sp if sp.numel() else None, seg_begin if sp.numel() else None, seg_split if sp.numel() else None)


def spmm_listed(a: Csr, X: torch.Tensor, rows: torch.Tensor, out: torch.Tensor, epilogue=None) -> torch.Tensor:
    """out[r] = epilogue(A X)[r] for the listed DISTINCT rows r only (all other rows of out keep their contents): llmrec_spmm_f32 with a
    plan over the list and rows_listed_only."""
    d = X.shape[1]
    whole = epilogue is not None and epilogue.op != EPI_NONE
    pl = listed_plan(a, rows, d, whole_row=whole)
    if epilogue is None:
        epilogue = spmm_epilogue(EPI_NONE)
    epilogue.rows_listed_only = 1
    part = torch.empty(max(pl.n_seg, 1) * d, dtype=torch.float32, device=X.device)
    return spmm_raw(a, X, out=out, epilogue=epilogue, partials=part, plan=pl)


def sort_unique_ids(ids: torch.Tensor, out_list: torch.Tensor, out_n: torch.Tensor):
    """out_list[0 .. out_n[0]) = the distinct ids >= 0 of `ids`, ascending (int32), entirely on the device (llmrec_sort_unique_ids_i32:
    one block, <= 32 768 ids): the host never learns the count."""
    _need_gpu(ids, out_list, out_n)
    n = ids.numel()
    if out_list.dtype != torch.int32 or out_n.dtype != torch.int32 or out_list.numel() < n or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise RuntimeError("sort_unique_ids: ids int64 contiguous, out_list int32 with room for every id, out_n int32[1]")
    _lib.call("llmrec_sort_unique_ids_i32", n, _p(ids), _p(out_list), _p(out_n), _stream())


def spmm_rows_compact(a: Csr, X: torch.Tensor, row_list: torch.Tensor, n_list: torch.Tensor, out: torch.Tensor, ws: Optional[torch.Tensor] = None):
    """out[j] = (A X)[row_list[j]] for j < n_list[0] (device count), zeros for the other slots of out [capacity, d]: "these rows of A X" as a
    fixed-size compact block, no host read-back (llmrec_spmm_rows_compact_f32; pattern-only operands)."""
    _need_gpu(X, out, row_list, n_list)
    if a.val is not None or a.col_scale is not None:
        raise RuntimeError("spmm_rows_compact: pattern-only operands (A = diag(row_scale) P)")
    X = _rowmajor(X)
    cap, d = out.shape
    need = _lib.query("llmrec_spmm_rows_compact_workspace_bytes", cap, d)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=X.device)
    _lib.call("llmrec_spmm_rows_compact_f32", a.n_rows, a.n_cols, _p(a.rowptr), _p(a.colidx), _p(a.row_scale), _p(X), _ld(X), d, _p(row_list),
              _p(n_list), cap, _p(out), _ld(out), _p(ws), ws.numel(), _stream())
    return ws


def scatter_set_rows(row_list: torch.Tensor, n_list: torch.Tensor, src: torch.Tensor, dst: torch.Tensor):
    """dst[row_list[j]] = src[j] for j < n_list[0] (llmrec_scatter_set_rows_f32)."""
    _need_gpu(src, dst, row_list, n_list)
    _lib.call("llmrec_scatter_set_rows_f32", src.shape[0], _p(row_list), _p(n_list), src.shape[1], _p(src), _ld(src), _p(dst), _ld(dst), _stream())


def spmm_raw(a: Csr, X: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False, epilogue=None,
             partials: Optional[torch.Tensor] = None, plan: Optional[SpmmPlan] = None) -> torch.Tensor:
    """Y = epilogue(A X) through llmrec_spmm_f32. accumulate: Y += A X (epilogue Z = Y, alpha = 1). partials: scratch of
    plan.n_seg * d floats when the caller runs several SpMMs over this operand at once (default: the plan's own)."""
    _need_gpu(X, a.rowptr)
    X = _rowmajor(X)
    if X.shape[0] != a.n_cols:
        raise RuntimeError("spmm: X has %d rows, operand has %d columns" % (X.shape[0], a.n_cols))
    d = X.shape[1]
    Y = out if out is not None else torch.empty(a.n_rows, d, dtype=torch.float32, device=X.device)
    if plan is not None:                                       # (a caller-built plan, e.g. over a row list: whole rows, no column slices;
        sw, pl = 0, plan                                       #  the operand's own full plan is not built for it - ADVICE r03)
    else:
        sw, pl = a.plan_for(d, whole_row=epilogue is not None and epilogue.op != EPI_NONE)
    if partials is None:
        partials = pl.scratch(d, X.device)
    if accumulate:
        if epilogue is not None:
            raise RuntimeError("spmm: accumulate and an explicit epilogue are exclusive (pass Z = Y, alpha = 1)")
        epilogue = spmm_epilogue(EPI_NONE, 1.0, Y)
    col_scale = a.col_scale
    if col_scale is not None and a.val is None and a.nnz >= SPMM_LATENCY_NNZ:
        # HBM-bound graphs: A diag(c) X = A (c . X) - one dense pass over X (8 d bytes per row) instead of a second random 4-byte
        # gather per EDGE (PMC, 36.6 M edges: 9.9 GB of memory traffic per launch with the per-edge scale, 6.9 GB without)
        # (the scaled copy lives in a scratch cached per operand, shape and stream - as SpmmPlan.scratch is - so that a captured step does
        #  not add an X-sized block to the graph pool per product; rounding: acc += A (c x) instead of fma(c, x, acc), only in this regime)
        cache = a.plans.setdefault("_scaled_x", {})
        key = (tuple(X.shape), torch.cuda.current_stream().cuda_stream)
        Xs = cache.get(key)
        if Xs is None or Xs.device != X.device:
            Xs = cache[key] = torch.empty(X.shape, dtype=torch.float32, device=X.device)
        _lib.call("llmrec_scale_rows_f32", X.shape[0], d, _p(col_scale), _p(X), _ld(X), _p(Xs), _ld(Xs), _stream())
        X, col_scale = Xs, None
    rp, ci = pl.csr_of(a)
    _lib.call("llmrec_spmm_f32", a.n_rows, a.n_cols, _p(rp), _p(ci), _p(a.val), _p(a.row_scale),
              _p(col_scale), _p(X), _ld(X), _p(Y), _ld(Y), d, sw, _c.byref(pl.c_struct()), _p(partials),
              _c.byref(epilogue) if epilogue is not None else None, _stream())
    return Y


SPMM_BF16_MAX_D = 256             # llmrec_spmm_xbf16_f32: d % 4 == 0, d <= 256


def _bf16_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError("%s: a 2-D torch.bfloat16 tensor with unit inner stride expected, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t


def rows_to_bf16(X: torch.Tensor, out: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = bf16(row_scale[r] * X[r]), round to nearest even (llmrec_rows_to_bf16): the bf16 shadow an llmrec_spmm_xbf16_f32 product
    gathers from. One dense pass; X may be a strided row view."""
    _need_gpu(X, out, row_scale)
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1:
        raise RuntimeError("rows_to_bf16: a 2-D fp32 tensor with unit inner stride expected")
    if out is None:
        out = torch.empty(X.shape, dtype=torch.bfloat16, device=X.device)
    if _bf16_rows(out, "rows_to_bf16").shape != X.shape:
        raise RuntimeError("rows_to_bf16: out is %s, X is %s" % (tuple(out.shape), tuple(X.shape)))
    _lib.call("llmrec_rows_to_bf16", X.shape[0], X.shape[1], _p(row_scale), _p(X), _ld(X), _p(out), _ld(out), _stream())
    return out


def spmm_bf16(a: Csr, Xb: torch.Tensor, out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, epilogue=None,
              plan: Optional[SpmmPlan] = None) -> torch.Tensor:
    """Y = epilogue(A widen(Xb)) through llmrec_spmm_xbf16_f32: the gathered rows are torch.bfloat16, everything else fp32 - bit for bit
    spmm_raw(a, Xb.float(), plan=the same whole-row plan). out_bf16: also receives bf16(Y), written from the finished rows. The plan
    (whole rows: this product has no column slices) and its scratch are the operand's cached ones. Raises on anything the library refuses
    (masked epilogues, d % 4 != 0, d > 256)."""
    _need_gpu(Xb, a.rowptr, out, out_bf16)
    _bf16_rows(Xb, "spmm_bf16")
    if Xb.shape[0] != a.n_cols:
        raise RuntimeError("spmm_bf16: Xb has %d rows, operand has %d columns" % (Xb.shape[0], a.n_cols))
    d = Xb.shape[1]
    Y = out if out is not None else torch.empty(a.n_rows, d, dtype=torch.float32, device=Xb.device)
    if out_bf16 is not None and _bf16_rows(out_bf16, "spmm_bf16").shape != Y.shape:
        raise RuntimeError("spmm_bf16: out_bf16 is %s, the product is %s" % (tuple(out_bf16.shape), tuple(Y.shape)))
    pl = plan if plan is not None else a.plan_for(d, whole_row=True)[1]
    rp, ci = pl.csr_of(a)
    _lib.call("llmrec_spmm_xbf16_f32", a.n_rows, a.n_cols, _p(rp), _p(ci), _p(a.val), _p(a.row_scale), _p(a.col_scale), _p(Xb), _ld(Xb),
              _p(Y), _ld(Y), _p(out_bf16), _ld(out_bf16) if out_bf16 is not None else 0, d, _c.byref(pl.c_struct()), _p(pl.scratch(d, Xb.device)),
              _c.byref(epilogue) if epilogue is not None else None, _stream())
    return Y


def spmm_multi(problems: Sequence[SpmmProblemC]) -> bool:
    """Up to LLMREC_SPMM_MAX_PROBLEMS independent products in ONE llmrec_spmm_multi_f32 launch on the current stream (results bit-identical
    to separate llmrec_spmm_f32 calls). False: the library refused the group (LLMREC_EUNSUPPORTED - e.g. the problems resolve to different
    kernel instances), nothing was launched and the caller issues the products one by one."""
    arr = (SpmmProblemC * len(problems))(*problems)
    return _lib.call_unless_unsupported("llmrec_spmm_multi_f32", len(problems), arr, _stream())


def spmm_multi_guest(problems: Sequence[SpmmProblemC], guest: SpmmGuestC) -> bool:
    """spmm_multi with a guest (llmrec_spmm_multi_guest_f32): the guest's blocks lead the grouped launch; every result is bit-identical
    to the separate calls. False: refused (LLMREC_EUNSUPPORTED), nothing was launched - the caller issues the guest's own entry point
    and the products as before."""
    arr = (SpmmProblemC * len(problems))(*problems)
    return _lib.call_unless_unsupported("llmrec_spmm_multi_guest_f32", len(problems), arr, _c.byref(guest), _stream())


def guest_sampler(seed: int, step_dev: torch.Tensor, exist_users: torch.Tensor, n_items: int, train: Csr, B_global: int,
                  slice_begin: int, B: int, n_aug: int, aug_pos: Optional[torch.Tensor], aug_neg: Optional[torch.Tensor],
                  users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_valid: torch.Tensor, ticket: torch.Tensor) -> SpmmGuestC:
    """sample_batch_wide's call as a guest descriptor (the same buffer checks)."""
    _need_gpu(step_dev, exist_users, users, pos, neg, n_valid, ticket)
    if users.numel() < B + n_aug or step_dev.dtype != torch.int64 or n_valid.dtype != torch.int32 or ticket.dtype != torch.int32:
        raise RuntimeError("sample_batch_wide: buffers of B + n_aug int64 entries, int64 step counter, int32 n_valid and ticket expected")
    g = SpmmGuestC(kind=GUEST_SAMPLER)
    g.u.sampler = GuestSamplerC(seed, _ptr(step_dev), exist_users.numel(), _ptr(exist_users), n_items, _ptr(train.rowptr), _ptr(train.colidx),
                                B_global, slice_begin, B, n_aug, _ptr(aug_pos), _ptr(aug_neg), _ptr(users), _ptr(pos), _ptr(neg),
                                _ptr(n_valid), _ptr(ticket))
    return g


def guest_plan_reach(users, pos, neg, B_max: int, n_valid, plan, n_users: int, n_items: int, item_rowptr, item_colidx, flags) -> SpmmGuestC:
    """llmrec_bpr_scatter_plan_reach_mark's call as a guest descriptor."""
    g = SpmmGuestC(kind=GUEST_PLAN_REACH)
    g.u.plan_reach = GuestPlanReachC(_ptr(users), _ptr(pos), _ptr(neg), B_max, _ptr(n_valid), _ptr(plan), n_users, n_items, _ptr(item_rowptr),
                                     _ptr(item_colidx), _ptr(flags))
    return g


def guest_losses(n_problems: int, B_max: int, n_valid, remember_rate: float, decay: float, batch_size_flag: float, out, saved, w_mf,
                 sumsq_partial, n_partial: int, feat_reg_coef: float, scal4, running_sums3) -> SpmmGuestC:
    """llmrec_bpr_multi_losses_assemble_f32's call as a guest descriptor; w_mf: the host weights (kept alive by the descriptor)."""
    g = SpmmGuestC(kind=GUEST_LOSSES)
    g.keep = w = (_c.c_float * n_problems)(*w_mf)
    g.u.losses = GuestLossesC(n_problems, B_max, _ptr(n_valid), remember_rate, decay, batch_size_flag, _ptr(out), _ptr(saved),
                              _c.cast(w, _c.c_void_p), _ptr(sumsq_partial), n_partial, feat_reg_coef, _ptr(scal4), _ptr(running_sums3))
    return g


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op: SparseOperand, X):
        ctx.op = op
        return spmm_raw(op.fwd, X)

    @staticmethod
    def backward(ctx, dY):
        return None, spmm_raw(ctx.op.bwd, dY)


def spmm(op, X: torch.Tensor) -> torch.Tensor:
    """Y = A X with autograd (dX = A^T dY). ``op``: SparseOperand or a torch sparse COO tensor."""
    if isinstance(op, torch.Tensor):
        op = operand_from_sparse_tensor(op)
    return _SpMM.apply(op, X)


# ---------------------------------------------------------------------------------------------
# R4: projection
# ---------------------------------------------------------------------------------------------
def linear_fwd_raw(X, W, b, out=None):
    _need_gpu(X, W, b)
    X, W = _rowmajor(X), _rowmajor(W)
    M, K = X.shape
    N = W.shape[0]
    Y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=X.device)
    _lib.call("llmrec_linear_fwd_f32", M, N, K, _p(X), _ld(X), _p(W), _ld(W), _p(b), _p(Y), _ld(Y), _stream())
    return Y


def linear_wgrad_raw(dY, X, dW, db, accumulate: bool):
    dY, X = _rowmajor(dY), _rowmajor(X)
    M, K = X.shape
    N = dY.shape[1]
    ws_bytes = _lib.query("llmrec_linear_wgrad_workspace_bytes", M, N, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device)
    _lib.call("llmrec_linear_wgrad_f32", M, N, K, _p(dY), _ld(dY), _p(X), _ld(X), _p(dW), _ld(dW), _p(db),
              1 if accumulate else 0, _p(ws), ws_bytes, _stream())


class _Linear(torch.autograd.Function):
    """Y = X W^T + b for CONSTANT X (the reference's feature matrices): no dX."""

    @staticmethod
    def forward(ctx, X, W, b):
        ctx.save_for_backward(X)
        return linear_fwd_raw(X, W, b)

    @staticmethod
    def backward(ctx, dY):
        (X,) = ctx.saved_tensors
        dW = torch.empty(dY.shape[1], X.shape[1], dtype=torch.float32, device=X.device)
        db = torch.empty(dY.shape[1], dtype=torch.float32, device=X.device)
        linear_wgrad_raw(dY, X, dW, db, accumulate=False)
        return None, dW, db


def linear(X, W, b):
    return _Linear.apply(X, W, b)


class _LinearMulti(torch.autograd.Function):
    """Several constant inputs through ONE shared Linear (the reference's item_trans for its 5
    attribute keys, Models.py:33,150): n outputs, one accumulated weight gradient."""

    @staticmethod
    def forward(ctx, W, b, *Xs):
        ctx.Xs = Xs
        return tuple(linear_fwd_raw(X, W, b) for X in Xs)

    @staticmethod
    def backward(ctx, *dYs):
        Xs = ctx.Xs
        N = Xs and dYs[0].shape[1]
        dW = torch.empty(N, Xs[0].shape[1], dtype=torch.float32, device=dYs[0].device)
        db = torch.empty(N, dtype=torch.float32, device=dYs[0].device)
        for k, (X, dY) in enumerate(zip(Xs, dYs)):
            linear_wgrad_raw(dY, X, dW, db, accumulate=k > 0)
        return (dW, db) + (None,) * len(Xs)


def linear_multi(W, b, Xs: Sequence[torch.Tensor]):
    return _LinearMulti.apply(W, b, *Xs)


# ---------------------------------------------------------------------------------------------
# R3: softmax over d
# ---------------------------------------------------------------------------------------------
class _SoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z):
        _need_gpu(Z)
        Z = _rowmajor(Z)
        Y = torch.empty(Z.shape, dtype=torch.float32, device=Z.device)
        _lib.call("llmrec_softmax_rows_fwd_f32", Z.shape[0], Z.shape[1], _p(Z), _ld(Z), _p(Y), _ld(Y), _stream())
        ctx.save_for_backward(Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        (Y,) = ctx.saved_tensors
        dY = _rowmajor(dY)
        dZ = torch.empty_like(Y)
        _lib.call("llmrec_softmax_rows_bwd_f32", Y.shape[0], Y.shape[1], _p(Y), _ld(Y), _p(dY), _ld(dY), _p(dZ), _ld(dZ), _stream())
        return dZ


def softmax_rows(Z):
    return _SoftmaxRows.apply(Z)


# ---------------------------------------------------------------------------------------------
# R6: fusion
# ---------------------------------------------------------------------------------------------
def _ptr_table(ts: Sequence[torch.Tensor]):
    n = len(ts)
    return (_c.c_void_p * max(n, 1))(*[t.data_ptr() for t in ts]), (_c.c_int64 * max(n, 1))(*[_ld(t) for t in ts])


class _Fuse(torch.autograd.Function):
    """out = mean_scale * sum(mean_terms) + sum_t rate_t * normalize(norm_terms[t])."""

    @staticmethod
    def forward(ctx, mean_scale, n_mean, rates, *terms):
        _need_gpu(*terms)
        terms = [_rowmajor(t) for t in terms]
        mean_terms, norm_terms = terms[:n_mean], terms[n_mean:]
        rows, d = terms[0].shape
        out = torch.empty(rows, d, dtype=torch.float32, device=terms[0].device)
        mp, ml = _ptr_table(mean_terms)
        npt, nl = _ptr_table(norm_terms)
        r = (_c.c_float * max(len(rates), 1))(*rates)
        _lib.call("llmrec_fuse_fwd_f32", rows, d, float(mean_scale), len(mean_terms), mp, ml, len(norm_terms), npt, nl, r,
                  _p(out), _ld(out), _stream())
        ctx.mean_scale, ctx.n_mean, ctx.rates = float(mean_scale), n_mean, list(rates)
        ctx.save_for_backward(*norm_terms)
        return out

    @staticmethod
    def backward(ctx, dOut):
        norm_terms = ctx.saved_tensors
        dOut = _rowmajor(dOut)
        rows, d = dOut.shape
        d_mean = None
        if ctx.n_mean:
            d_mean = torch.empty(rows, d, dtype=torch.float32, device=dOut.device)
            _lib.call("llmrec_axpy_f32", rows, d, ctx.mean_scale, None, _p(dOut), _ld(dOut), _p(d_mean), _ld(d_mean), 0, _stream())
        d_terms = [torch.empty(rows, d, dtype=torch.float32, device=dOut.device) for _ in norm_terms]
        if norm_terms:
            npt, nl = _ptr_table(norm_terms)
            dp, dl = _ptr_table(d_terms)
            r = (_c.c_float * len(ctx.rates))(*ctx.rates)
            _lib.call("llmrec_fuse_bwd_f32", rows, d, _p(dOut), _ld(dOut), len(norm_terms), npt, nl, r, dp, dl, 0, 0, 0.0, _stream())
        return (None, None, None) + (d_mean,) * ctx.n_mean + tuple(d_terms)


def fuse(mean_terms: List[torch.Tensor], norm_terms: List[torch.Tensor], rates: List[float]):
    """Layer mean + normalise-and-add (reference Models.py:185-197)."""
    if len(mean_terms) > CONST["LLMREC_MAX_TERMS"] or len(norm_terms) > CONST["LLMREC_MAX_TERMS"]:
        raise RuntimeError("fuse: too many terms")
    return _Fuse.apply(1.0 / max(len(mean_terms), 1), len(mean_terms), list(rates), *mean_terms, *norm_terms)


# ---------------------------------------------------------------------------------------------
# R7: BPR + prune
# ---------------------------------------------------------------------------------------------
def bpr_saved_floats(B: int) -> int:
    """LLMREC_BPR_SAVED_FLOATS(B) of include/llmrec_hip.h."""
    return 6 * B + 8


def bpr_plan_words(B: int) -> int:
    """LLMREC_BPR_PLAN_WORDS(B): 3 B sorted keys + 3 B int32 run lengths."""
    return 5 * B


def bpr_scatter_plan(users, pos, neg, n_valid=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The deterministic scatter plan of one batch (llmrec_bpr_scatter_plan): sorted (id, slot) keys of the user side and of the item
    side + the run lengths, LLMREC_BPR_PLAN_WORDS(B) 64-bit words. Every BPR backward entry point takes it - rows that several samples share are added in one fixed order,
    as the reference's CPU index_put does (main.py:232-254), never with float atomics."""
    _need_gpu(users, pos, neg)
    B = users.numel()
    if out is None:
        out = torch.empty(max(bpr_plan_words(B), 1), dtype=torch.int64, device=users.device)
    elif out.numel() < bpr_plan_words(B) or out.dtype != torch.int64:
        raise RuntimeError("bpr_scatter_plan: plan buffer needs %d int64 words" % bpr_plan_words(B))
    _lib.call("llmrec_bpr_scatter_plan", _p(users), _p(pos), _p(neg), B, _p(n_valid), _p(out), _stream())
    return out


BprProblem = _lib.STRUCT["llmrec_bpr_problem_t"]
LinearProblem = _lib.STRUCT["llmrec_linear_problem_t"]
ZeroTensor = _lib.STRUCT["llmrec_zero_tensor_t"]
FuseFwdProblem = _lib.STRUCT["llmrec_fuse_fwd_problem_t"]
FuseBwdProblem = _lib.STRUCT["llmrec_fuse_bwd_problem_t"]
WgradProblem = _lib.STRUCT["llmrec_wgrad_problem_t"]
WgradTarget = _lib.STRUCT["llmrec_wgrad_target_t"]
WgradUpdate = _lib.STRUCT["llmrec_wgrad_update_t"]


def _wgrad_problem(pr, pair):
    """Fill one llmrec_wgrad_problem_t from (dY, X[, db_row_weight[, (row_list, n_rows, rows_expected)]]); row_list = the rows of dY that
    can be non-zero (served by the bf16x3 128-wide organisation only, else refused)."""
    dY, X = pair[:2]
    _need_gpu(dY, X)
    pr.dY, pr.lddy, pr.X, pr.ldx, pr.M = dY.data_ptr(), _ld(dY), X.data_ptr(), _ld(X), X.shape[0]
    pr.db_row_weight = pair[2].data_ptr() if len(pair) > 2 and pair[2] is not None else None
    if len(pair) > 3 and pair[3] is not None:
        pr.row_list, pr.n_rows, pr.rows_expected = pair[3][0].data_ptr(), pair[3][1].data_ptr(), int(pair[3][2] or 0)


def _wgrad_targets(targets, block_budget: int = 0):
    """targets: [(pairs, dW, db, accumulate)] -> (ctypes array, keep-alive list, N); block_budget: llmrec_wgrad_target_t.block_budget"""
    arr = (WgradTarget * len(targets))()
    arr[0].block_budget = int(block_budget)
    keep = []
    N = targets[0][1].shape[0]
    for i, (pairs, dW, db, accumulate) in enumerate(targets):
        probs = (WgradProblem * len(pairs))()
        for j, pair in enumerate(pairs):
            _wgrad_problem(probs[j], pair)
            if len(pair) > 3 and pair[3] is not None:
                rl, nr, _ = pair[3]
                if rl.dtype != torch.int32 or nr.dtype != torch.int32 or rl.numel() < pair[1].shape[0] + 32:
                    raise RuntimeError("linear_wgrad_multi: row_list must be int32 with M + 32 entries, n_rows an int32 device scalar")
                keep.append((rl, nr))
        keep.append(probs)
        arr[i].n_problems, arr[i].problems, arr[i].K = len(pairs), _c.cast(probs, _c.c_void_p), dW.shape[1]
        arr[i].dW, arr[i].lddw, arr[i].db, arr[i].accumulate = dW.data_ptr(), _ld(dW), (db.data_ptr() if db is not None else None), 1 if accumulate else 0
    return arr, keep, N


def batch_reach_rows(users, pos, neg, n_valid, by_item: "Csr", flags: torch.Tensor, row_list: torch.Tensor, n_rows: torch.Tensor):
    """llmrec_batch_reach_rows: the ascending list of the user rows a batch reaches (its users + every user adjacent to one of its
    positive / negative items; by_item = the CSR whose rows are items and whose columns are users). flags: [n_users] uint8 scratch,
    all-zero on entry and on return; row_list: int32 [n_users + 32]; n_rows: int32 [1]. Two launches, no host sync."""
    _need_gpu(users, pos, neg, flags, row_list, n_rows)
    n_users, n_items = by_item.n_cols, by_item.n_rows
    if flags.numel() < n_users or row_list.numel() < n_users + 32 or flags.dtype != torch.uint8 or row_list.dtype != torch.int32:
        raise RuntimeError("batch_reach_rows: flags [n_users] uint8, row_list [n_users + 32] int32")
    _lib.call("llmrec_batch_reach_rows", n_users, n_items, _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid), _p(by_item.rowptr),
              _p(by_item.colidx), _p(flags), _p(row_list), _p(n_rows), _stream())


def linear_wgrad_multi_workspace(targets, block_budget: int = 0) -> int:
    """Bytes of workspace llmrec_linear_wgrad_multi_bf16x3 needs for these targets; -1 = outside its fast path."""
    arr, keep, N = _wgrad_targets(targets, block_budget)
    return _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", len(targets), arr, N)


def linear_wgrad_multi(targets, ws: Optional[torch.Tensor] = None, update=None, block_budget: int = 0, host_spmm=None):
    """The bf16x3 weight gradients of several Linears in one launch + one reduction launch (llmrec_linear_wgrad_multi_bf16x3).
    targets: [(pairs, dW, db, accumulate)], pairs = [(dY, X)] as in linear_wgrad_grouped; all dW have N rows.
    update = (FusedAdamW, [(W, b)] per target): the AdamW update of those parameters rides in the reduction launch
    (llmrec_linear_wgrad_multi_adamw_bf16x3; the optimizer's step counter has been advanced already).
    block_budget: resident blocks per round the launch is laid out for (0 = 256: one per CU).
    host_spmm = (llmrec_spmm_problem_t, the device's CU count), with update only: the independent product runs in the CUs the launch
    leaves free (llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3). Returns whether the pair was accepted; False: NOTHING was launched,
    and the caller issues the product and this call without it. (Without host_spmm: None.)"""
    arr, keep, N = _wgrad_targets(targets, block_budget)
    need = _lib.query("llmrec_linear_wgrad_multi_workspace_bytes", len(targets), arr, N)
    if need < 0:
        raise RuntimeError("linear_wgrad_multi: shapes outside the fast path (use linear_wgrad_grouped per target)")
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=targets[0][1].device)
    if host_spmm is not None and update is None:
        raise RuntimeError("linear_wgrad_multi: host_spmm needs update (the hosting entry point carries the AdamW update)")
    if update is None:
        _lib.call("llmrec_linear_wgrad_multi_bf16x3", len(targets), arr, N, _p(ws), ws.numel(), _stream())
        return
    opt, params = update
    if opt.dev_state is None:
        raise RuntimeError("linear_wgrad_multi: the optimizer's step counter has not been advanced (FusedAdamW.advance())")
    upd = (WgradUpdate * len(targets))()
    for i, (W, b) in enumerate(params):
        stW = opt.moments(W)
        upd[i].W, upd[i].m_W, upd[i].v_W = W.data_ptr(), stW[0].data_ptr(), stW[1].data_ptr()
        if b is not None:
            stb = opt.moments(b)
            upd[i].b, upd[i].m_b, upd[i].v_b = b.data_ptr(), stb[0].data_ptr(), stb[1].data_ptr()
        gs = float(opt.grad_scale.get(W, 1.0))
        if b is not None and float(opt.grad_scale.get(b, 1.0)) != gs:
            raise RuntimeError("linear_wgrad_multi: W and b of one target need the same grad_scale")
        upd[i].g_scale = gs
    if host_spmm is not None:
        problem, n_cu = host_spmm
        return _lib.call_unless_unsupported("llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3", len(targets), arr, N, _p(ws), ws.numel(), upd,
                                            _p(opt.dev_state), opt.lr, opt.betas[0], opt.betas[1], opt.eps, opt.wd, _c.byref(problem),
                                            int(n_cu), _stream())
    _lib.call("llmrec_linear_wgrad_multi_adamw_bf16x3", len(targets), arr, N, _p(ws), ws.numel(), upd, _p(opt.dev_state), opt.lr, opt.betas[0],
              opt.betas[1], opt.eps, opt.wd, _stream())


def linear_wgrad_grouped(pairs, dW, db, accumulate: bool, ws: Optional[torch.Tensor] = None, precision: str = "f32"):
    """dW (+)= sum_p dY_p^T X_p for several (dY, X) pairs sharing one weight (one launch + reduce).
    precision "bf16x3": llmrec_linear_wgrad_grouped_bf16x3 (three-term bf16 split, fp32-class error)."""
    arr = (WgradProblem * len(pairs))()
    M_total = 0
    for i, pair in enumerate(pairs):
        _wgrad_problem(arr[i], pair)
        M_total += pair[1].shape[0]
    N, K = dW.shape
    need = _lib.query("llmrec_linear_wgrad_workspace_bytes", M_total, N, K)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dW.device)
    _lib.call("llmrec_linear_wgrad_grouped_bf16x3" if precision == "bf16x3" else "llmrec_linear_wgrad_grouped_f32",
              len(pairs), arr, N, K, _p(dW), _ld(dW), _p(db), 1 if accumulate else 0, _p(ws), ws.numel(), _stream())


def linear_problems(jobs):
    """The llmrec_linear_problem_t array of [(X, W, bias, out, bias_scale)] (bias / bias_scale: a tensor or None)."""
    arr = (LinearProblem * len(jobs))()
    for i, (X, W, b, out, bscale) in enumerate(jobs):
        arr[i].X, arr[i].ldx, arr[i].M, arr[i].K = X.data_ptr(), _ld(X), X.shape[0], X.shape[1]
        arr[i].W, arr[i].ldw, arr[i].bias = W.data_ptr(), _ld(W), _ptr(b)
        arr[i].Y, arr[i].ldy = out.data_ptr(), _ld(out)
        arr[i].bias_scale = _ptr(bscale)
    return arr


def linear_fwd_grouped(jobs, N: int, precision: str = "f32"):
    """jobs: list of (X, W, bias, out) or (X, W, bias, out, bias_scale) - one launch. precision "f32": exact fp32 MFMA
    (llmrec_linear_fwd_grouped_f32); "bf16x3": three-term bf16 split, six bf16 MFMAs, fp32-class
    error (llmrec_linear_fwd_grouped_bf16x3). bias_scale [M]: out[r] = X[r] W^T + bias_scale[r] * bias."""
    for job in jobs:
        _need_gpu(*job[:4])
    arr = linear_problems([tuple(job[:4]) + (job[4] if len(job) > 4 else None,) for job in jobs])
    name = {"f32": "llmrec_linear_fwd_grouped_f32", "bf16x3": "llmrec_linear_fwd_grouped_bf16x3"}[precision]
    _lib.call(name, len(jobs), arr, N, _stream())


class _BprPrune(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Eu, Ei, users, pos, neg, remember_rate, decay, batch_size_flag, n_valid):
        _need_gpu(Eu, Ei, users, pos, neg)
        Eu, Ei = _rowmajor(Eu), _rowmajor(Ei)
        B = users.numel()
        d = Eu.shape[1]
        out = torch.empty(2, dtype=torch.float32, device=Eu.device)
        saved = torch.empty(bpr_saved_floats(B), dtype=torch.float32, device=Eu.device)
        _lib.call("llmrec_bpr_prune_fwd_f32", _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), d, _p(users), _p(pos), _p(neg), B, _p(n_valid),
                  float(remember_rate), float(decay), float(batch_size_flag), _p(out), _p(saved), _stream())
        ctx.save_for_backward(Eu, Ei, users, pos, neg, saved)
        ctx.n_valid, ctx.decay, ctx.bsz = n_valid, float(decay), float(batch_size_flag)
        return out

    @staticmethod
    def backward(ctx, g):
        Eu, Ei, users, pos, neg, saved = ctx.saved_tensors
        g = g.contiguous()
        dEu, dEi = torch.zeros_like(Eu), torch.zeros_like(Ei)
        plan = bpr_scatter_plan(users, pos, neg, ctx.n_valid)
        _lib.call("llmrec_bpr_prune_bwd_f32", _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), Eu.shape[1], _p(users), _p(pos), _p(neg),
                  users.numel(), _p(ctx.n_valid), ctx.decay, ctx.bsz, _p(saved), _p(g), _p(dEu), _ld(dEu), _p(dEi), _ld(dEi), _p(plan), _stream())
        return dEu, dEi, None, None, None, None, None, None, None


def bpr_wide_workspace(global_B: int, device) -> torch.Tensor:
    """A workspace of llmrec_bpr_prune_wide_workspace_bytes(global_B) bytes for llmrec_bpr_prune_fwd_wide_f32 (uninitialised: the
    entry point's own launches initialise it)."""
    need = _lib.query("llmrec_bpr_prune_wide_workspace_bytes", int(global_B))
    if need < 0:
        raise RuntimeError("bpr_wide_workspace: batch of %d exceeds LLMREC_BPR_WIDE_MAX_B" % global_B)
    return torch.empty(need, dtype=torch.uint8, device=device)


def bpr_plan_wide_workspace(B_max: int, device) -> torch.Tensor:
    """A workspace of llmrec_bpr_scatter_plan_wide_workspace_bytes(B_max) bytes for llmrec_bpr_scatter_plan_wide (uninitialised)."""
    need = _lib.query("llmrec_bpr_scatter_plan_wide_workspace_bytes", int(B_max))
    if need < 0:
        raise RuntimeError("bpr_plan_wide_workspace: batch of %d exceeds LLMREC_BPR_WIDE_MAX_B" % B_max)
    return torch.empty(need, dtype=torch.uint8, device=device)


def bpr_multi_wide_workspace(n_problems: int, B_max: int, device) -> torch.Tensor:
    """A workspace of llmrec_bpr_multi_wide_workspace_bytes(n_problems, B_max) bytes for llmrec_bpr_multi_select_bwd_wide_f32
    (uninitialised: the entry point's own launches initialise it)."""
    need = _lib.query("llmrec_bpr_multi_wide_workspace_bytes", int(n_problems), int(B_max))
    if need < 0:
        raise RuntimeError("bpr_multi_wide_workspace: %d problems / a batch of %d exceed LLMREC_BPR_MAX_PROBLEMS / LLMREC_BPR_WIDE_MAX_B"
                           % (n_problems, B_max))
    return torch.empty(need, dtype=torch.uint8, device=device)


def bpr_scatter_plan_wide(users, pos, neg, n_valid, out: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """llmrec_bpr_scatter_plan_wide: bpr_scatter_plan's words for a batch of any size up to LLMREC_BPR_WIDE_MAX_B (ws: bpr_plan_wide_workspace)."""
    _need_gpu(users, pos, neg, out, ws)
    B = users.numel()
    if out.numel() < bpr_plan_words(B) or out.dtype != torch.int64:
        raise RuntimeError("bpr_scatter_plan_wide: plan buffer needs %d int64 words" % bpr_plan_words(B))
    _lib.call("llmrec_bpr_scatter_plan_wide", _p(users), _p(pos), _p(neg), B, _p(n_valid), _p(out), _p(ws), ws.numel(), _stream())
    return out


def bpr_multi_scores_wide(problems, d: int, users, pos, neg, n_valid, saved, row_stamp=None, adamw_state=None, lr: float = 0.0,
                          beta1: float = 0.0, beta2: float = 0.0):
    """llmrec_bpr_multi_scores_wide_f32 over a ctypes array of BprProblem (adamw_state None: the row stamp only)."""
    _lib.call("llmrec_bpr_multi_scores_wide_f32", len(problems), problems, d, _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid), _p(saved),
              _p(row_stamp), _p(adamw_state), float(lr), float(beta1), float(beta2), _stream())


def bpr_multi_select_bwd_wide(problems, d: int, users, pos, neg, n_valid, remember_rate: float, decay: float, batch_size_flag: float, saved,
                              flag_u, flag_i, row_stamp, plan, ws):
    """llmrec_bpr_multi_select_bwd_wide_f32 (ws: bpr_multi_wide_workspace; plan: bpr_scatter_plan_wide or, up to the cap, bpr_scatter_plan)."""
    _lib.call("llmrec_bpr_multi_select_bwd_wide_f32", len(problems), problems, d, _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid),
              float(remember_rate), float(decay), float(batch_size_flag), _p(saved), _p(flag_u), _p(flag_i), _p(row_stamp), _p(plan),
              _p(ws), 0 if ws is None else ws.numel(), _stream())


def bpr_multi_losses_wide(n_problems: int, B_max: int, n_valid, remember_rate: float, decay: float, batch_size_flag: float, out, saved,
                          w_mf=None, partial=None, n_partial: int = 0, reg_coef: float = 0.0, scal=None, running=None):
    """llmrec_bpr_multi_losses_wide_f32 (scal None: the loss values only)."""
    w = None if w_mf is None else (_c.c_float * n_problems)(*w_mf)
    _lib.call("llmrec_bpr_multi_losses_wide_f32", n_problems, B_max, _p(n_valid), float(remember_rate), float(decay), float(batch_size_flag),
              _p(out), _p(saved), w, _p(partial), int(n_partial), float(reg_coef), _p(scal), _p(running), _stream())


_scatter_ws = {}                                                   # device -> the sorted scatter's workspace (grown, never shrunk)


def _scatter_rows(ids, rows, dst):
    """dst[ids[j]] += rows[j], rows of one id in ascending j (llmrec_scatter_rows_f32: deterministic). Calls on one device share one
    workspace: they are ordered by the stream they are issued on."""
    n = ids.numel()
    need = _lib.query("llmrec_scatter_rows_workspace_bytes", n)
    ws = _scatter_ws.get(dst.device)
    if ws is None or ws.numel() < need:
        ws = _scatter_ws[dst.device] = torch.empty(need, dtype=torch.uint8, device=dst.device)
    _lib.call("llmrec_scatter_rows_f32", n, _p(ids), _p(rows), _ld(rows), rows.shape[1], 1.0, _p(dst), _ld(dst), _p(ws), ws.numel(), _stream())


class _BprPruneWide(torch.autograd.Function):
    """_BprPrune beyond LLMREC_BPR_MAX_B: the multi-block selection forward; the backward writes compact rows and scatters them sorted -
    the scatter plan's order (ascending slot, positives before negatives) without its LDS-sized rank-counting sort."""
    @staticmethod
    def forward(ctx, Eu, Ei, users, pos, neg, remember_rate, decay, batch_size_flag, n_valid):
        _need_gpu(Eu, Ei, users, pos, neg)
        Eu, Ei = _rowmajor(Eu), _rowmajor(Ei)
        B = users.numel()
        out = torch.empty(2, dtype=torch.float32, device=Eu.device)
        saved = torch.empty(bpr_saved_floats(B), dtype=torch.float32, device=Eu.device)
        ws = bpr_wide_workspace(B, Eu.device)
        _lib.call("llmrec_bpr_prune_fwd_wide_f32", _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), Eu.shape[1], _p(users), _p(pos), _p(neg), B,
                  float(remember_rate), float(decay), float(batch_size_flag), None, 0, 0, 0, _p(out), _p(saved), _p(n_valid),
                  _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(Eu, Ei, users, pos, neg, saved)
        ctx.n_valid, ctx.decay, ctx.bsz = n_valid, float(decay), float(batch_size_flag)
        return out

    @staticmethod
    def backward(ctx, g):
        Eu, Ei, users, pos, neg, saved = ctx.saved_tensors
        g = g.contiguous()
        B, d = users.numel(), Eu.shape[1]
        dEu, dEi = torch.zeros_like(Eu), torch.zeros_like(Ei)
        rows3 = torch.empty(3, B, d, dtype=torch.float32, device=Eu.device)
        _lib.call("llmrec_bpr_prune_bwd_rows_f32", _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), d, _p(users), _p(pos), _p(neg), B, _p(ctx.n_valid),
                  ctx.decay, ctx.bsz, _p(saved), _p(g), _p(rows3), _stream())
        # rows of samples b >= n_valid are zeros: their (padded, in-range) ids add nothing, no mask and no host read
        _scatter_rows(users, rows3[0], dEu)
        _scatter_rows(torch.cat([pos, neg]), rows3[1:].view(-1, d), dEi)
        return dEu, dEi, None, None, None, None, None, None, None


def bpr_prune(Eu, Ei, users, pos, neg, drop_rate: float, decay: float, batch_size_flag: float, n_valid=None):
    """Returns a 2-vector [mf_loss, emb_loss] (reference main.py:330-342 with prune_loss :158-165).
    users/pos/neg: int64 device vectors indexing rows of Eu / Ei. Batches above LLMREC_BPR_MAX_B (up to LLMREC_BPR_WIDE_MAX_B) take
    the multi-block selection (llmrec_bpr_prune_fwd_wide_f32); the routing is by size only."""
    if users.dtype != torch.int64 or pos.dtype != torch.int64 or neg.dtype != torch.int64:
        raise RuntimeError("bpr_prune: int64 index tensors expected")
    if users.numel() > CONST["LLMREC_BPR_WIDE_MAX_B"]:
        raise RuntimeError("bpr_prune: batch of %d exceeds LLMREC_BPR_WIDE_MAX_B" % users.numel())
    remember = 1 - drop_rate                                       # python float, as main.py:161
    fn = _BprPruneWide if users.numel() > CONST["LLMREC_BPR_MAX_B"] else _BprPrune
    return fn.apply(Eu, Ei, users, pos, neg, remember, decay, batch_size_flag, n_valid)


# ---------------------------------------------------------------------------------------------
# R8: regulariser
# ---------------------------------------------------------------------------------------------
class _SumSq(torch.autograd.Function):
    """coef * sum_t ||X_t||_F^2 as a 1-element tensor."""

    @staticmethod
    def forward(ctx, coef, *Xs):
        _need_gpu(*Xs)
        Xs = [_rowmajor(x) for x in Xs]
        out = torch.empty(1, dtype=torch.float32, device=Xs[0].device)
        ws_bytes = _lib.query("llmrec_sumsq_workspace_bytes", 0, 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Xs[0].device)
        for k, x in enumerate(Xs):
            _lib.call("llmrec_sumsq_f32", x.shape[0], x.shape[1], _p(x), _ld(x), float(coef), 1 if k else 0, _p(out), _p(ws), ws_bytes, _stream())
        ctx.coef = float(coef)
        ctx.save_for_backward(*Xs)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        outs = []
        for x in ctx.saved_tensors:
            dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            _lib.call("llmrec_axpy_f32", x.shape[0], x.shape[1], 2.0 * ctx.coef, _p(g), _p(x), _ld(x), _p(dx), _ld(dx), 0, _stream())
            outs.append(dx)
        return (None,) + tuple(outs)


def sumsq(coef: float, Xs: Sequence[torch.Tensor]):
    return _SumSq.apply(coef, *Xs)


# ---------------------------------------------------------------------------------------------
# R8: AdamW
# ---------------------------------------------------------------------------------------------
AdamwTensor = _lib.STRUCT["llmrec_adamw_tensor_t"]
ZeroRowsJob = _lib.STRUCT["llmrec_zero_rows_job_t"]


class FusedAdamW:
    """torch.optim.AdamW(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01) semantics as built
    at reference main.py:100-104, one HIP launch per parameter, bias corrections kept on device
    (graph-capturable). Parameters without a gradient are skipped, as torch does."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self.params = [p for p in params]
        self.lr, self.betas, self.eps, self.wd = float(lr), betas, float(eps), float(weight_decay)
        self.state = {}
        self.dev_state = None
        self.grad_scale = {}                    # {param: s}: the gradient of that parameter is s * param.grad (default 1)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def advance(self):
        """Advance the device step counter / bias corrections (the first half of step()). A fused step calls it
        early on a side stream so that only the multi-tensor update itself remains on the critical path."""
        if self.dev_state is None:
            dev = next(p for p in self.params if p.grad is not None).device
            self.dev_state = torch.zeros(3, dtype=torch.float32, device=dev)
        _lib.call("llmrec_adamw_advance", _p(self.dev_state), self.lr, self.betas[0], self.betas[1], _stream())

    @torch.no_grad()
    def step_params(self, params, sources=None, zero_rows=None):
        """The update of a SUBSET of the parameters (their gradients are final), the step counter having been advanced already
        (advance()): a fused step updates its embedding tables while the weight-gradient GEMM of the Linears is still running.
        sources: {param: (G, scale)} - the gradient of that parameter is scale * G (another buffer); it is ALSO stored into param.grad by the
        same launch (llmrec_adamw_tensor_t.g_out: no separate scaling pass). zero_rows: (jobs [(ids int64, dst [rows, width])], B_cap, n_valid_dev) -
        the row-wise clean-up of the step's scatter targets rides in the same launch (llmrec_adamw_multi_zero_rows_f32)."""
        self._update([p for p in params if p.grad is not None], sources=sources, zero_rows=zero_rows)

    @torch.no_grad()
    def step(self, advanced: bool = False):
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        if not advanced:
            self.advance()
        self._update(live)

    def moments(self, p):
        """(exp_avg, exp_avg_sq) of a parameter, created on first use."""
        st = self.state.get(p)
        if st is None:
            if not p.is_contiguous():
                raise RuntimeError("FusedAdamW: contiguous parameters expected")
            st = self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
        return st

    def _tensor_array(self, group, sources=None):
        """(llmrec_adamw_tensor_t array, tensors to keep alive) of one launch's parameters."""
        arr = (AdamwTensor * max(len(group), 1))()
        keep = []
        for i, p in enumerate(group):
            st = self.state.get(p)
            if st is None:
                st = self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
            if not p.is_contiguous():
                raise RuntimeError("FusedAdamW: contiguous parameters expected")
            src = sources.get(p) if sources else None
            if src is not None:
                g, scale = src
                if not g.is_contiguous() or g.numel() != p.numel() or not p.grad.is_contiguous():
                    raise RuntimeError("FusedAdamW: a gradient source is a contiguous tensor of the parameter's size")
                arr[i].g_scale, arr[i].g_out = float(scale) * float(self.grad_scale.get(p, 1.0)), p.grad.data_ptr()
            else:
                g = p.grad.contiguous()
                arr[i].g_scale, arr[i].g_out = float(self.grad_scale.get(p, 1.0)), None
            keep.append(g)
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p.data_ptr(), g.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), p.numel()
        return arr, keep

    def _update(self, live, sources=None, zero_rows=None):
        if not live and zero_rows is None:
            return
        _need_gpu(*live)
        cap = CONST["LLMREC_ADAMW_MAX_TENSORS"]
        if zero_rows is not None and len(live) > cap:
            raise RuntimeError("FusedAdamW: the clean-up rides with at most %d tensors" % cap)
        for lo in range(0, max(len(live), 1), cap):
            group = live[lo:lo + cap]
            arr, keep = self._tensor_array(group, sources)
            if zero_rows is None:
                _lib.call("llmrec_adamw_multi_f32", len(group), arr, _p(self.dev_state), self.lr, self.betas[0], self.betas[1],
                          self.eps, self.wd, _stream())
            else:
                jobs, b_cap, n_valid = zero_rows
                if len(jobs) > CONST["LLMREC_ZERO_ROWS_MAX_JOBS"]:
                    raise RuntimeError("FusedAdamW: %d clean-up jobs exceed LLMREC_ZERO_ROWS_MAX_JOBS" % len(jobs))
                jarr = (ZeroRowsJob * max(len(jobs), 1))()
                for j, (ids, dst) in enumerate(jobs):
                    jarr[j].ids, jarr[j].dst, jarr[j].ldd, jarr[j].d = ids.data_ptr(), dst.data_ptr(), _ld(dst), dst.shape[1]
                if self.dev_state is None:
                    raise RuntimeError("FusedAdamW: advance() first")
                _lib.call("llmrec_adamw_multi_zero_rows_f32", len(group), arr, _p(self.dev_state), self.lr, self.betas[0], self.betas[1],
                          self.eps, self.wd, len(jobs), jarr, int(b_cap), _p(n_valid), _stream())

    def state_tensors(self):
        """[(name, tensor)] of everything the optimiser keeps on the device between steps: the step counter with its two bias
        corrections (dev_state) and both moments of EVERY parameter, by the parameter's position - created here where they do not
        exist yet (a checkpoint is loaded before the first step; a parameter that never gets a gradient keeps all-zero moments). A new
        piece of device state of the optimiser is one more line here."""
        if self.dev_state is None:
            self.dev_state = torch.zeros(3, dtype=torch.float32, device=self.params[0].device)
        out = [("adamw/dev_state", self.dev_state)]
        for i, p in enumerate(self.params):
            m, v = self.moments(p)
            out += [("adamw/m/%d" % i, m), ("adamw/v/%d" % i, v)]
        return out

    def state_dict(self):
        """The per-op path's form of state_tensors(): host copies by name, and the hyper-parameters the state was formed under."""
        return {"state": {name: t.detach().cpu().clone() for name, t in self.state_tensors()},
                "hyper": {"lr": self.lr, "betas": list(self.betas), "eps": self.eps, "weight_decay": self.wd}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Copies a state_dict() INTO the existing tensors (never rebinds one: a captured graph holds their addresses)."""
        mine = dict(self.state_tensors())
        theirs = sd["state"]
        bad = sorted(set(mine) ^ set(theirs)) + [k for k in mine if k in theirs and (mine[k].shape != theirs[k].shape or mine[k].dtype != theirs[k].dtype)]
        if bad:
            raise RuntimeError("FusedAdamW.load_state_dict: the state does not fit this optimiser: %s" % bad[:8])
        for k, t in mine.items():
            t.copy_(theirs[k])

    @torch.no_grad()
    def step_params_rows_group(self, params, sources, fuse_problems, d, softmax_bwd) -> bool:
        """step_params(params, sources) in ONE launch with two row sweeps that are independent of it (llmrec_step_rows_group_f32):
        fuse_problems = the FuseBwdProblem array of llmrec_fuse_bwd_src_multi_f32 (or None), softmax_bwd = (Y, dY, dZ, alpha) of
        llmrec_softmax_rows_bwd_scaled_f32 (or None). False: the library refused the group (nothing was launched) - the caller issues
        the three launches itself."""
        live = [p for p in params if p.grad is not None]
        if len(live) > CONST["LLMREC_ADAMW_MAX_TENSORS"]:
            return False
        _need_gpu(*live)
        if live and self.dev_state is None:
            raise RuntimeError("FusedAdamW: advance() first")
        arr, keep = self._tensor_array(live, sources)
        if softmax_bwd is not None:
            Y, dY, dZ, alpha = softmax_bwd
            sm = (Y.shape[0], Y.shape[1], float(alpha), _p(Y), _ld(Y), _p(dY), _ld(dY), _p(dZ), _ld(dZ))
        else:
            sm = (0, 0, 1.0, None, 0, None, 0, None, 0)
        return _lib.call_unless_unsupported("llmrec_step_rows_group_f32", len(fuse_problems) if fuse_problems is not None else 0, fuse_problems,
                                            int(d), len(live), arr, _p(self.dev_state), self.lr, self.betas[0], self.betas[1], self.eps,
                                            self.wd, *sm, _stream())


# ---------------------------------------------------------------------------------------------
# R9/R10: scoring + top-K, R11: sampler
# ---------------------------------------------------------------------------------------------
TOPK_MODES = {"exact": CONST["LLMREC_TOPK_MODE_EXACT_SWEEP"], "prefilter": CONST["LLMREC_TOPK_MODE_PREFILTER"]}


def topk_mode(mode=None, n_items: int = 0, d: int = 64, K: int = 50) -> int:
    """llmrec_score_topk_mode_f32's mode: "exact" = every score by the exact-fp32 MFMA chain; "prefilter" = bf16 sweep keeping the 64 best
    by approximate score, exact re-ranking + verification, exact sweep for the tiles that fail it (bit-identical lists and scores);
    "auto" (default; LLMREC_TOPK_MODE overrides) = prefilter whenever K leaves room to verify. Measured on MI355X at 16 384 users, d = 64
    (profiles/r06_topk_crossover.json): 1.41 x (10 K items), 1.96 x (33 K), 2.09 x (66 K), 2.03 x (131 K), 1.93 x (262 K), 1.96 x (524 K),
    1.99 x (10^6); 65 536 users x 10^6 items 107.7 -> 46.4 ms, d = 128 50.2 -> 29.7 ms. Up to round 5 the mode stopped paying at 524 K
    items (0.84 x at 10^6: every 16-user tile streamed the 256 MB fragment table through the L2-miss path); since round 6 tables beyond
    131 072 items are swept in item PARTS of 8 MB of fragments with part-major block ids (csrc/topk.hip plan_parts), so that the blocks
    resident at one time share each part through the L2."""
    if mode is None:
        mode = os.environ.get("LLMREC_TOPK_MODE", "auto")
    if mode == "auto":
        mode = "prefilter" if K <= CONST["LLMREC_TOPK_PREFILTER_MAX_K"] else "exact"
    if mode not in TOPK_MODES:
        raise RuntimeError("top-K mode %r (auto | exact | prefilter)" % (mode,))
    return TOPK_MODES[mode]


def topk_set_part_items(items: int = 0):
    """llmrec_topk_set_part_items: the bf16 sweep's item parts (0 = the library's policy, -1 = never, else items per part). Process-wide;
    workspaces sized before a change are stale."""
    _lib.call("llmrec_topk_set_part_items", int(items))


def _wide_train_nnz(train: Optional[Csr], q: torch.Tensor) -> int:
    """llmrec_score_topk_wide_f32's train_nnz: the sum of the train-row lengths of the listed users, a user listed twice counted twice
    (one device read; callers that capture size their workspace with it beforehand)."""
    if train is None or q.numel() == 0:
        return 0
    rp = train.rowptr
    return int((rp[q + 1].to(torch.int64) - rp[q].to(torch.int64)).sum().item())


def _train_ptrs(train: Optional[Csr]):
    """(train_rowptr, train_colidx) of a top-K entry: NULL, NULL without a train CSR."""
    return (_p(train.rowptr), _p(train.colidx)) if train is not None else (None, None)


def topk_wide_mode(mode=None, n_items: int = 0, d: int = 64, K: int = 50) -> int:
    """The mode of a call at K > LLMREC_TOPK_MAX (rounds of the single-sweep call, llmrec_score_topk_wide_f32): "auto" = the bf16 sweep, 56
    ranks per pass - a pass asks for at most LLMREC_TOPK_PREFILTER_MAX_K items, so the prefilter always has room to verify, and
    ceil(K / 56) of its calls cost less than ceil(K / 64) exact sweeps. K <= LLMREC_TOPK_MAX: topk_mode's answer."""
    return topk_mode(mode, n_items, d, min(K, CONST["LLMREC_TOPK_PREFILTER_MAX_K"]) if K > CONST["LLMREC_TOPK_MAX"] else K)


def score_topk(Eu, Ei, query_users: torch.Tensor, train: Optional[Csr], K: int, mode=None, stats: Optional[dict] = None,
               train_nnz: Optional[int] = None):
    """Masked top-K item ids (int32 [n_query, K], -1 = none) and scores for the listed users. K <= LLMREC_TOPK_MAX (64): one sweep
    (llmrec_score_topk_mode_f32); up to LLMREC_TOPK_WIDE_MAX (1024): rounds of it (llmrec_score_topk_wide_f32), same ranking rule and bits.
    K > 64 with a train CSR sizes its mask from the queried train rows, which is ONE HOST READ of the device (a synchronisation the K <= 64
    call does not have; not capturable). train_nnz: an upper bound the caller knows - train.colidx.numel() when the query users are
    distinct - replaces that read (a bound that is too small returns empty lists, see include/llmrec_hip.h).
    stats (a dict; synchronises; at K > 64 the words describe single passes and are reported as None): receives
    "fallback_tiles" / "tiles" - the user tiles the bf16 mode's verification sent to the exact sweep -, "drains" - the pool drains of the bf16
    sweep, summed over its blocks - and "bitmap_rows" - the train rows its blocks swept as bitmaps (None outside the bf16 mode)."""
    _need_gpu(Eu, Ei, query_users)
    Eu, Ei = _rowmajor(Eu.detach()), _rowmajor(Ei.detach())
    q = query_users.to(torch.int64).contiguous()
    n = q.numel()
    if K > CONST["LLMREC_TOPK_WIDE_MAX"]:
        raise RuntimeError("score_topk: K = %d exceeds LLMREC_TOPK_WIDE_MAX = %d" % (K, CONST["LLMREC_TOPK_WIDE_MAX"]))
    idx = torch.empty(n, K, dtype=torch.int32, device=Eu.device)
    sc = torch.empty(n, K, dtype=torch.float32, device=Eu.device)
    if K > CONST["LLMREC_TOPK_MAX"]:
        nnz = (int(train_nnz) if train is not None else 0) if train_nnz is not None else _wide_train_nnz(train, q)
        ws = topk_workspace(n, Ei.shape[0], Eu.device, Eu.shape[1], K, nnz)
        _lib.call("llmrec_score_topk_wide_f32", n, _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), Ei.shape[0], Eu.shape[1],
                  *_train_ptrs(train), K, _p(idx), _p(sc), _p(ws), ws.numel(), topk_wide_mode(mode, Ei.shape[0], Eu.shape[1], K), nnz, _stream())
        if stats is not None:                                                                          # (the words describe single passes)
            stats.update(tiles=(n + 15) // 16, fallback_tiles=None, drains=None, bitmap_rows=None)
        return idx, sc
    ws = topk_workspace(n, Ei.shape[0], Eu.device, Eu.shape[1])
    _lib.call("llmrec_score_topk_mode_f32", n, _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), Ei.shape[0], Eu.shape[1],
              *_train_ptrs(train), K, _p(idx), _p(sc), _p(ws), ws.numel() if ws is not None else 0, topk_mode(mode, Ei.shape[0], Eu.shape[1], K), _stream())
    if stats is not None:
        off = _lib.query("llmrec_score_topk_stats_offset", n, Ei.shape[0])
        stats["tiles"] = (n + 15) // 16
        pre = topk_mode(mode, Ei.shape[0], Eu.shape[1], K) == TOPK_MODES["prefilter"] and K <= CONST["LLMREC_TOPK_PREFILTER_MAX_K"]
        stats["fallback_tiles"] = int(ws[off + 4:off + 8].view(torch.int32).item()) if pre else 0
        stats["drains"] = int(ws[off:off + 4].view(torch.int32).item()) if pre else None                # pool drains of the bf16 sweep, summed over its blocks
        stats["bitmap_rows"] = int(ws[off + 8:off + 12].view(torch.int32).item()) if pre else None     # long train rows swept as per-block bitmaps (bf16 mode's launch)
    return idx, sc


def topk_workspace(n_query: int, n_items: int, device, d: int = 64, K: Optional[int] = None, train_nnz: int = 0) -> Optional[torch.Tensor]:
    """Scratch for llmrec_score_topk_ws_f32: the item table in fragment order + the part lists of the left-over user tiles. K beyond
    LLMREC_TOPK_MAX (with train_nnz, see _wide_train_nnz): the larger workspace of llmrec_score_topk_wide_f32."""
    if K is not None and K > CONST["LLMREC_TOPK_MAX"]:
        nbytes = _lib.query("llmrec_score_topk_wide_workspace_bytes", n_query, n_items, d, K, train_nnz)
        if nbytes < 0:
            raise RuntimeError("topk_workspace: bad sizes (K <= %d, train_nnz + n_query * K < 2^31)" % CONST["LLMREC_TOPK_WIDE_MAX"])
    else:
        nbytes = _lib.query("llmrec_score_topk_workspace_bytes", n_query, n_items, d)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes > 0 else None


class ItemFilter:
    """The id maps of an item allow mask (llmrec_item_filter_build): new_id int32 [n_items] = the rank of an item among the eligible ones or
    -1, old_id int32 [n_items] = the r-th eligible item (the entries from n_kept on are unspecified), n_kept_dev int32 [1] and the host's n_kept.
    allow: uint8 or bool [n_items] on the GPU, any non-zero byte = eligible. The build is three launches without atomics; the constructor
    then reads n_kept, which is ONE HOST READ of the device (the count sizes the compact table and the launches of every filtered call - the
    trade-off of _wide_train_nnz: pay it once per filter, not per call; not capturable)."""

    def __init__(self, allow: torch.Tensor):
        _need_gpu(allow)
        if allow.dtype == torch.bool:
            allow = allow.view(torch.uint8)
        if allow.dtype != torch.uint8 or allow.dim() != 1:
            raise RuntimeError("ItemFilter: a 1-D uint8 / bool mask expected, got %s %s" % (allow.dtype, tuple(allow.shape)))
        allow = allow.contiguous()
        n = self.n_items = allow.numel()
        dev = allow.device
        self.new_id = torch.empty(n, dtype=torch.int32, device=dev)
        self.old_id = torch.empty(n, dtype=torch.int32, device=dev)
        self.n_kept_dev = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.query("llmrec_item_filter_workspace_bytes", n), dtype=torch.uint8, device=dev)
        _lib.call("llmrec_item_filter_build", n, _p(allow), _p(self.new_id), _p(self.old_id), _p(self.n_kept_dev), _p(ws), ws.numel(), _stream())
        self.n_kept = int(self.n_kept_dev.item())


def topk_filtered_workspace(n_query: int, n_items: int, n_kept: int, device, d: int = 64, K: int = 50, train_nnz: int = 0) -> torch.Tensor:
    """Scratch for llmrec_score_topk_filtered_f32 (include/llmrec_hip.h gives the formula)."""
    nbytes = _lib.query("llmrec_score_topk_filtered_workspace_bytes", n_query, n_items, n_kept, d, K, train_nnz)
    if nbytes < 0:
        raise RuntimeError("topk_filtered_workspace: bad sizes (1 <= d <= 128, K <= %d, train_nnz + n_query * K < 2^31)" % CONST["LLMREC_TOPK_WIDE_MAX"])
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def _served(name: str, Eu, Ei, query_users, K: int, filt, wide_max: bool = True):
    """What every served wrapper starts with: (Eu, Ei row-major and detached, q int64 contiguous, n, I, d, idx int32 [n, K], scores float32
    [n, K]), K checked against LLMREC_TOPK_WIDE_MAX (wide_max: the entry has that limit) and the filter's size against the table."""
    _need_gpu(Eu, Ei, query_users)
    Eu, Ei = _rowmajor(Eu.detach()), _rowmajor(Ei.detach())
    q = query_users.to(torch.int64).contiguous()
    n, I, d = q.numel(), Ei.shape[0], Eu.shape[1]
    if wide_max and K > CONST["LLMREC_TOPK_WIDE_MAX"]:
        raise RuntimeError("%s: K = %d exceeds LLMREC_TOPK_WIDE_MAX = %d" % (name, K, CONST["LLMREC_TOPK_WIDE_MAX"]))
    if filt is not None and filt.n_items != I:
        raise RuntimeError("%s: the filter covers %d items, the table has %d" % (name, filt.n_items, I))
    return Eu, Ei, q, n, I, d, torch.empty(n, K, dtype=torch.int32, device=Eu.device), torch.empty(n, K, dtype=torch.float32, device=Eu.device)


def _score_topk_served(name: str, Eu, Ei, query_users, train, K, filt, mode, train_nnz, ws, exclude=None):
    """What score_topk_filtered and score_topk_excluded share: _served, train_nnz, the workspace and the filter's pointer triple around
    llmrec_<name>_f32. exclude: the checked (rowptr, colidx) of the excluded entry, whose three arguments go between train_nnz and the
    maps."""
    Eu, Ei, q, n, I, d, idx, sc = _served(name, Eu, Ei, query_users, K, filt)
    kept = filt.n_kept if filt is not None else I
    nnz = (int(train_nnz) if train is not None else 0) if train_nnz is not None else _wide_train_nnz(train, q)
    excl = ()
    if exclude is not None:
        excl_nnz = exclude[1].numel()
        excl = (_p(exclude[0]), _p(exclude[1]) if excl_nnz else None, excl_nnz)
    if ws is None:
        ws = (topk_filtered_workspace(n, I, kept, Eu.device, d, K, nnz) if exclude is None else
              topk_excluded_workspace(n, I, kept, Eu.device, d, K, nnz, excl_nnz))
    maps = (_p(filt.new_id), _p(filt.old_id), _p(filt.n_kept_dev)) if filt is not None else (None, None, None)
    _lib.call("llmrec_%s_f32" % name, n, _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), I, d, *_train_ptrs(train),
              K, _p(idx), _p(sc), _p(ws), ws.numel(), topk_wide_mode(mode, kept, d, K), nnz, *excl, *maps, kept, _stream())
    return idx, sc


def score_topk_filtered(Eu, Ei, query_users: torch.Tensor, train: Optional[Csr], K: int, filt: Optional[ItemFilter], mode=None,
                        train_nnz: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """score_topk among the items an ItemFilter keeps: (idx int32 [n, K] in ORIGINAL item ids, -1 = none, scores) - for every listed user the
    first K of {eligible items not in the user's train row} by (score desc, item id asc), the score bits of ops.scores
    (llmrec_score_topk_filtered_f32: the eligible rows as a dense table, the train rows in its numbering, the wide call, the ids mapped
    back; a filter that keeps a tenth of the catalogue sweeps a tenth of it). filt=None forwards to score_topk.
    train_nnz: as for score_topk - an upper bound of the queried train-row lengths that replaces the one host read (here it is needed at
    every K, because the compact mask rows are sized by it); a bound that is too small returns empty lists. With it, and a workspace `ws`
    of topk_filtered_workspace, the call is capturable."""
    if filt is None:
        return score_topk(Eu, Ei, query_users, train, K, mode=mode, train_nnz=train_nnz)
    return _score_topk_served("score_topk_filtered", Eu, Ei, query_users, train, K, filt, mode, train_nnz, ws)


def topk_excluded_workspace(n_query: int, n_items: int, n_kept: int, device, d: int = 64, K: int = 50, train_nnz: int = 0,
                            excl_nnz: int = 0) -> torch.Tensor:
    """Scratch for llmrec_score_topk_excluded_f32 (include/llmrec_hip.h gives the formula); n_kept = n_items without a filter."""
    nbytes = _lib.query("llmrec_score_topk_excluded_workspace_bytes", n_query, n_items, n_kept, d, K, train_nnz, excl_nnz)
    if nbytes < 0:
        raise RuntimeError("topk_excluded_workspace: bad sizes (1 <= d <= 128, K <= %d, train_nnz + excl_nnz + n_query * K < 2^31)"
                           % CONST["LLMREC_TOPK_WIDE_MAX"])
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def score_topk_excluded(Eu, Ei, query_users: torch.Tensor, train: Optional[Csr], K: int, exclude, filt: Optional[ItemFilter] = None, mode=None,
                        train_nnz: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """score_topk_filtered with one more exclusion list PER QUERY: (idx int32 [n, K] in ORIGINAL item ids, -1 = none, scores) - for query q
    the first K of {eligible items} minus {train row of its user} minus {exclusion row q} by (score desc, item id asc), the score bits of
    ops.scores (llmrec_score_topk_excluded_f32: the rows are sorted and merged with the train rows on the device, the unchanged sweeps run
    over the merged mask). exclude: (rowptr int32 [n + 1], colidx int32) on the device, a CSR over the QUERIES of this call - a user listed
    twice may carry two rows; entries in any order, repeats allowed, entries < 0 or >= n_items ignored (-1 padding), ineligible items
    ignored. colidx.numel() must be rowptr[n] (the device checks it; a mismatch returns empty lists). exclude=None forwards to
    score_topk_filtered: the same launches and bits as without this call. filt=None: no filter, Ei is swept in place.
    train_nnz / ws (topk_excluded_workspace): as for score_topk_filtered; with both the call is capturable."""
    if exclude is None:
        return score_topk_filtered(Eu, Ei, query_users, train, K, filt, mode=mode, train_nnz=train_nnz, ws=ws)
    name = "score_topk_excluded"
    return _score_topk_served(name, Eu, Ei, query_users, train, K, filt, mode, train_nnz, ws, exclude=_query_csr(name, "exclude", exclude, query_users.numel()))


def _query_csr(name: str, what: str, csr, n: int):
    """A checked (rowptr int32 [n + 1], colidx int32) device CSR over the n queries of a call."""
    rowptr, colidx = csr
    _need_gpu(rowptr, colidx)
    if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32 or rowptr.dim() != 1 or colidx.dim() != 1 or rowptr.numel() != n + 1:
        raise RuntimeError("%s: %s = (rowptr int32 [%d], colidx int32 [nnz]) expected, got %s %s and %s %s"
                           % (name, what, n + 1, rowptr.dtype, tuple(rowptr.shape), colidx.dtype, tuple(colidx.shape)))
    return rowptr.contiguous(), colidx.contiguous()


def score_topk_candidates_workspace(n_query: int, K: int, cand_nnz: int, excl_nnz: int = 0, device="cuda") -> torch.Tensor:
    """Scratch for llmrec_score_topk_candidates_f32 (include/llmrec_hip.h gives the formula)."""
    nbytes = _lib.query("llmrec_score_topk_candidates_workspace_bytes", n_query, K, cand_nnz, excl_nnz)
    if nbytes < 0:
        raise RuntimeError("score_topk_candidates_workspace: bad sizes (K >= 1, n_query * K < 2^31, cand_nnz and excl_nnz in [0, 2^31))")
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def _score_topk_candidates(name: str, Eu, Ei, query_users, train, K, candidates, exclude, filt, ws, quota=None):
    """Both candidate wrappers around llmrec_<name>_f32. quota: the capped entry's four arguments behind new_id (item_group, n_groups,
    group_cap, cap) - with them K has the limit LLMREC_TOPK_WIDE_MAX."""
    Eu, Ei, q, n, I, d, idx, sc = _served(name, Eu, Ei, query_users, K, filt, wide_max=quota is not None)
    crp, cci = _query_csr(name, "candidates", candidates, n)
    erp, eci = _query_csr(name, "exclude", exclude, n) if exclude is not None else (None, None)
    cand_nnz, excl_nnz = cci.numel(), eci.numel() if eci is not None else 0
    if ws is None:
        ws = score_topk_candidates_workspace(n, K, cand_nnz, excl_nnz, Eu.device)
    _lib.call("llmrec_%s_f32" % name, n, _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), I, d, *_train_ptrs(train),
              K, _p(idx), _p(sc), _p(ws), ws.numel(), _p(crp), _p(cci) if cand_nnz else None, cand_nnz,
              _p(erp), _p(eci) if excl_nnz else None, excl_nnz, _p(filt.new_id) if filt is not None else None, *(quota or ()), _stream())
    return idx, sc


def score_topk_candidates(Eu, Ei, query_users: torch.Tensor, train: Optional[Csr], K: int, candidates, exclude=None,
                          filt: Optional[ItemFilter] = None, ws: Optional[torch.Tensor] = None):
    """Exact top-K among PER-QUERY candidate lists: (idx int32 [n, K] in item ids, -1 = none, scores float32 [n, K]) - for query q the first
    K of {ids of candidate row q, as a set} minus {train row of its user} minus {exclusion row q} by (score desc, item id asc), the score
    bits of ops.scores (llmrec_score_topk_candidates_f32, csrc/candidates.hip: only the listed pairs are scored, two radix sorts select).
    candidates / exclude: (rowptr int32 [n + 1], colidx int32) on the device, CSRs over the QUERIES of this call - a user listed twice may
    carry two rows; entries in any order, repeats allowed, entries < 0 or >= n_items ignored, as are items a filter does not keep (only
    filt.new_id is read). colidx.numel() must be rowptr[n] (the device checks it; a mismatch returns empty lists). Any K >= 1 with
    n * K < 2^31. Nothing is read back: with a workspace `ws` of score_topk_candidates_workspace the call is capturable."""
    return _score_topk_candidates("score_topk_candidates", Eu, Ei, query_users, train, K, candidates, exclude, filt, ws)


def score_topk_candidates_capped(Eu, Ei, query_users: torch.Tensor, train: Optional[Csr], K: int, candidates, item_group: torch.Tensor, cap,
                                 exclude=None, filt: Optional[ItemFilter] = None, ws: Optional[torch.Tensor] = None, n_groups: Optional[int] = None):
    """score_topk_candidates under per-group quotas: (idx int32 [n, K], scores float32 [n, K]) - query q's survivors ranked as there, and of
    every group only the first cap(g) of them kept; the list is the first K kept items (llmrec_score_topk_candidates_capped_f32,
    csrc/quota.hip: the uncapped call's launches up to the sorted pairs, then one wave per query walks the ranking).
    item_group: int32 [n_items] on the device; a value outside [0, n_groups) means no group (never capped). cap: an int >= 1 for every group,
    or an int32 device tensor [n_groups] of caps >= 0 (0 removes the group; n_groups is then its length). n_groups with an int cap:
    int(item_group.max()) + 1 unless given - giving it keeps the call free of host reads. K <= LLMREC_TOPK_WIDE_MAX (1024).
    candidates / exclude / filt: as for score_topk_candidates; ws: its workspace (score_topk_candidates_workspace) - with it (and n_groups
    or a cap tensor) the call is capturable."""
    name = "score_topk_candidates_capped"
    _need_gpu(item_group)
    if item_group.dtype != torch.int32 or item_group.dim() != 1 or item_group.numel() != Ei.shape[0]:
        raise RuntimeError("%s: item_group int32 [%d] expected, got %s %s" % (name, Ei.shape[0], item_group.dtype, tuple(item_group.shape)))
    item_group = item_group.contiguous()
    if isinstance(cap, torch.Tensor):
        _need_gpu(cap)
        if cap.dtype != torch.int32 or cap.dim() != 1 or cap.numel() < 1 or (n_groups is not None and int(n_groups) != cap.numel()):
            raise RuntimeError("%s: cap = int32 [n_groups >= 1] expected, got %s %s (n_groups = %s)" % (name, cap.dtype, tuple(cap.shape), n_groups))
        caps, one, groups = cap.contiguous(), 0, cap.numel()
    else:
        if int(cap) != cap or cap < 1:
            raise RuntimeError("%s: an integer cap >= 1 or an int32 tensor [n_groups] expected, got %r" % (name, cap))
        caps, one = None, int(cap)
        groups = int(n_groups) if n_groups is not None else max(int(item_group.max()) + 1, 1)
        if groups < 1:
            raise RuntimeError("%s: n_groups = %d, at least 1 expected" % (name, groups))
    return _score_topk_candidates(name, Eu, Ei, query_users, train, K, candidates, exclude, filt, ws, quota=(_p(item_group), groups, _p(caps), one))


def export_candidates(Eu, Ei, k: int = 10, query_users: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stage-1 candidate export: the top-k item ids per user WITHOUT masking, i.e. what the reference
    README's `torch.topk(user_emb @ item_emb.T, k=10)` snippet (README.md:243-247) produces for
    `candidate_indices`, as an int64 [n, k] tensor - computed by the scoring kernel, never
    materialising U x I. Ties are broken by ascending item id. k <= LLMREC_TOPK_WIDE_MAX (1024)."""
    q = torch.arange(Eu.shape[0], device=Eu.device) if query_users is None else query_users
    idx, _ = score_topk(Eu, Ei, q, None, k)
    return idx.to(torch.int64)


def scores(Eu, Ei, query_users: torch.Tensor):
    _need_gpu(Eu, Ei, query_users)
    Eu, Ei = _rowmajor(Eu.detach()), _rowmajor(Ei.detach())
    q = query_users.to(torch.int64).contiguous()
    S = torch.empty(q.numel(), Ei.shape[0], dtype=torch.float32, device=Eu.device)
    _lib.call("llmrec_scores_f32", q.numel(), _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), Ei.shape[0], Eu.shape[1], _p(S), _ld(S), _stream())
    return S


# ---------------------------------------------------------------------------------------------
# Serving: fold-in of users who are not rows of the graph (csrc/foldin.hip)
# ---------------------------------------------------------------------------------------------
@dataclass
class FoldInTables:
    """The item side of a trained model in the form llmrec_fold_in_users_f32 gathers: ONE fp32 table T [n_items, C * d], C = L + 2 +
    n_attr + 1 slices of d columns - chain I_0 .. I_{L-1} | image | text | attributes (the model's key order) | profile -, so that one
    gathered item is one contiguous read; and what the kernel needs beside it: L, n_attr, d and the three rates (model_cat_rate,
    user_cat_rate, item_cat_rate)."""
    T: torch.Tensor
    L: int
    n_attr: int
    d: int
    c_m: float
    c_u: float
    c_a: float

    @property
    def C(self) -> int:
        return self.L + 3 + self.n_attr

    @property
    def n_items(self) -> int:
        return self.T.shape[0]

    def slice(self, c: int) -> torch.Tensor:
        """slice c of T as a column view [n_items, d]"""
        return self.T[:, c * self.d:(c + 1) * self.d]

    @staticmethod
    def from_model(model, ui, iu, rates) -> "FoldInTables":
        """The tables of `model` (MM_Model) as it stands, without dropout or masking whatever its mode: the projections and products of
        MM_Model.forward's item side, by the kernels that forward runs (llmrec_linear_fwd_f32, llmrec_spmm_f32), written straight into
        the column views of T. ui / iu: the normalised adjacency and its transpose (SparseOperand or the torch sparse tensors the
        forward takes); rates: (model_cat_rate, user_cat_rate, item_cat_rate). Paid once per loaded checkpoint."""
        ui = operand_from_sparse_tensor(ui) if isinstance(ui, torch.Tensor) else ui
        iu = operand_from_sparse_tensor(iu) if isinstance(iu, torch.Tensor) else iu
        keys = list(model.item_feats.keys())
        L, d = int(model.n_ui_layers), model.item_id_embedding.weight.shape[1]
        n_items = model.item_id_embedding.weight.shape[0]
        if L < 1:
            raise RuntimeError("FoldInTables: a model without a propagation layer has no user side to fold into")
        c_m, c_u, c_a = (float(r) for r in rates)
        with torch.no_grad():
            t = FoldInTables(torch.empty(n_items, (L + 3 + len(keys)) * d, dtype=torch.float32, device=model.item_id_embedding.weight.device),
                             L, len(keys), d, c_m, c_u, c_a)
            t.slice(0).copy_(model.item_id_embedding.weight.detach())
            for l in range(1, L):                                  # intermediate layers: no softmax
                spmm_raw(iu.fwd, spmm_raw(ui.fwd, t.slice(l - 1)), out=t.slice(l))
            lin = lambda feats, m, c: linear_fwd_raw(feats, m.weight.detach(), m.bias.detach(), out=t.slice(c))
            lin(model.image_feats, model.image_trans, L)
            lin(model.text_feats, model.text_trans, L + 1)
            for k, key in enumerate(keys):
                lin(model.item_feats[key], model.item_trans, L + 2 + k)
            spmm_raw(iu.fwd, linear_fwd_raw(model.user_feats, model.user_trans.weight.detach(), model.user_trans.bias.detach()), out=t.slice(t.C - 1))
        return t


def fold_in_workspace(n: int, nnz: int, tables: FoldInTables, device) -> Optional[torch.Tensor]:
    """Scratch for llmrec_fold_in_users_f32 (None where it needs none: no row can exceed one segment)."""
    nbytes = _lib.query("llmrec_fold_in_users_workspace_bytes", n, nnz, tables.L, tables.n_attr, tables.d)
    if nbytes < 0:
        raise RuntimeError("fold_in_workspace: bad sizes (n, nnz < 2^31)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def fold_in_row_scale(rowptr: torch.Tensor) -> torch.Tensor:
    """float32((float64(deg) + 1e-8) ** -0.5) per row, on the device: csr_norm's row constant for the lengths of `rowptr`."""
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.float64)
    return (deg + 1e-8).pow(-0.5).to(torch.float32)


def fold_in_users(tables: FoldInTables, rowptr: torch.Tensor, colidx: torch.Tensor, row_scale: Optional[torch.Tensor] = None,
                  id_rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, d]: the embeddings the model behind `tables` gives n users who are not rows of its graph, from their item histories
    (llmrec_fold_in_users_f32; include/llmrec_hip.h states the formula and the order of the sums). rowptr int32 [n + 1], colidx int32
    [rowptr[n]] on the device: entries in the order to add them, repeats count, entries < 0 or >= n_items add nothing.
    row_scale float32 [n]: D^-1/2 of each row - None: fold_in_row_scale(rowptr), i.e. from the row LENGTHS (padding included: it is
    the caller's to pass rows without it, or the scale). id_rows [n, d]: the users' own id rows (None: zeros).
    With row_scale, out and ws (fold_in_workspace) given the call allocates nothing and reads nothing back: capturable."""
    _need_gpu(tables.T, rowptr, colidx, row_scale, id_rows, out, ws)
    if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32 or rowptr.dim() != 1 or colidx.dim() != 1 or rowptr.numel() < 1:
        raise RuntimeError("fold_in_users: rowptr int32 [n + 1] and colidx int32 [nnz] expected, got %s %s and %s %s"
                           % (rowptr.dtype, tuple(rowptr.shape), colidx.dtype, tuple(colidx.shape)))
    rowptr, colidx = rowptr.contiguous(), colidx.contiguous()
    n, nnz, d = rowptr.numel() - 1, colidx.numel(), tables.d
    T = tables.T
    if T.dtype != torch.float32 or T.dim() != 2 or T.stride(1) != 1 or T.shape[1] != tables.C * d:
        raise RuntimeError("fold_in_users: T must be fp32 [n_items, %d] with unit inner stride" % (tables.C * d))
    if row_scale is None:
        row_scale = fold_in_row_scale(rowptr)
    if row_scale.dtype != torch.float32 or row_scale.numel() != n or not row_scale.is_contiguous():
        raise RuntimeError("fold_in_users: row_scale must be contiguous fp32 [%d]" % n)
    if id_rows is not None:
        if id_rows.dtype != torch.float32 or tuple(id_rows.shape) != (n, d) or id_rows.stride(1) != 1:
            raise RuntimeError("fold_in_users: id_rows must be fp32 [%d, %d] with unit inner stride" % (n, d))
        id_rows = id_rows.detach()
    if out is None:
        out = torch.empty(n, d, dtype=torch.float32, device=T.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, d) or out.stride(1) != 1:
        raise RuntimeError("fold_in_users: out must be fp32 [%d, %d] with unit inner stride" % (n, d))
    if ws is None:
        ws = fold_in_workspace(n, nnz, tables, T.device)
    _lib.call("llmrec_fold_in_users_f32", n, _p(rowptr), _p(colidx) if nnz else None, nnz, _p(row_scale),
              _p(id_rows), _ld(id_rows) if id_rows is not None else 0, _p(T), _ld(T), T.shape[0],
              tables.L, tables.n_attr, d, tables.c_m, tables.c_u, tables.c_a, _p(out), _ld(out),
              _p(ws), ws.numel() if ws is not None else 0, _stream())
    return out


def topk_hits(topk_idx: torch.Tensor, query_users: torch.Tensor, test_rowptr: torch.Tensor, test_colidx: torch.Tensor):
    q = query_users.to(torch.int64).contiguous()
    hits = torch.empty(topk_idx.shape, dtype=torch.uint8, device=topk_idx.device)
    _lib.call("llmrec_topk_hits", q.numel(), _p(q), topk_idx.shape[1], _p(topk_idx), _p(test_rowptr), _p(test_colidx), _p(hits), _stream())
    return hits


def topk_eval_sums(idx: torch.Tensor, query_users: torch.Tensor, test_rowptr: torch.Tensor, test_colidx: torch.Tensor, Ks,
                   out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[4, len(Ks)] float64: the sums over the query users of precision / recall / ndcg / hit-ratio at every cut-off (llmrec_topk_eval_sums:
    hits, per-user metrics and their sums in two launches; lists of up to LLMREC_TOPK_WIDE_MAX = 1024 columns). out: a device tensor or a
    PINNED host tensor (written by the kernel itself)."""
    _need_gpu(idx, query_users, test_rowptr, test_colidx)
    n, K = idx.shape
    Ks = [int(k) for k in Ks]
    if out is None:
        out = torch.empty(4, len(Ks), dtype=torch.float64, device=idx.device)
    need = _lib.query("llmrec_topk_eval_sums_workspace_bytes", n, len(Ks))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=idx.device)
    arr = (_c.c_int32 * len(Ks))(*Ks)
    _lib.call("llmrec_topk_eval_sums", n, _p(query_users.to(torch.int64).contiguous()), K, _p(idx.contiguous()), _p(test_rowptr), _p(test_colidx),
              len(Ks), arr, _p(ws), ws.numel(), _c.c_void_p(out.data_ptr()), _stream())
    return out


def _rows(csr):
    """(rowptr, colidx) of an ops.Csr or of a (rowptr, colidx) pair."""
    return (csr.rowptr, csr.colidx) if hasattr(csr, "rowptr") else (csr[0], csr[1])


def auc_workspace(n_query: int, n_items: int, device, d: int = 64) -> torch.Tensor:
    """Scratch for llmrec_score_auc_f32 (per-user integer counts and the partial sums; independent of the held-out rows)."""
    return torch.empty(_lib.query("llmrec_score_auc_workspace_bytes", n_query, n_items, d), dtype=torch.uint8, device=device)


def score_auc(Eu, Ei, query_users: torch.Tensor, train, held, counts: bool = False, out: Optional[torch.Tensor] = None,
              ws: Optional[torch.Tensor] = None):
    """Full-rank AUC per query user on the device (llmrec_score_auc_f32; the contract is in include/llmrec_hip.h): float64 [n], and with
    counts=True also int64 [n, 3] = (c2, |P|, |N|). train / held: ops.Csr or (rowptr, colidx) (train may be None). out: a float64 tensor of
    one element - device or PINNED host memory - that receives the sum of the per-user AUCs (fixed-order tree; a pinned one is valid after
    a stream synchronisation)."""
    _need_gpu(Eu, Ei, query_users)
    Eu, Ei = _rowmajor(Eu.detach()), _rowmajor(Ei.detach())
    q = query_users.to(torch.int64).contiguous()
    n, I, d = q.numel(), Ei.shape[0], Eu.shape[1]
    hr, hc = _rows(held)
    tr, tc = _rows(train) if train is not None else (None, None)
    _need_gpu(hr, hc, tr, tc)
    if out is not None and (out.dtype != torch.float64 or out.numel() < 1):
        raise RuntimeError("score_auc: out must be a float64 tensor of one element")
    need = _lib.query("llmrec_score_auc_workspace_bytes", n, I, d)
    if ws is None or ws.numel() < need:
        ws = auc_workspace(n, I, Eu.device, d)
    auc = torch.empty(n, dtype=torch.float64, device=Eu.device)
    cnt = torch.empty(n, 3, dtype=torch.int64, device=Eu.device) if counts else None
    _lib.call("llmrec_score_auc_f32", n, _p(q), _p(Eu), _ld(Eu), _p(Ei), _ld(Ei), I, d, _p(tr), _p(tc), _p(hr), _p(hc),
              _p(auc), _p(cnt), _c.c_void_p(out.data_ptr()) if out is not None else None, _p(ws), ws.numel(), _stream())
    return (auc, cnt) if counts else auc


def sample_bpr(seed: int, step: int, exist_users: torch.Tensor, n_items: int, train: Csr, B: int):
    dev = exist_users.device
    u = torch.empty(B, dtype=torch.int64, device=dev)
    p = torch.empty(B, dtype=torch.int64, device=dev)
    n = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("llmrec_sample_bpr", seed, step, exist_users.numel(), _p(exist_users), n_items, _p(train.rowptr), _p(train.colidx),
              B, _p(u), _p(p), _p(n), _stream())
    return u, p, n


def sample_batch(seed: int, step_dev: torch.Tensor, exist_users: torch.Tensor, n_items: int, train: Csr, B_global: int,
                 slice_begin: int, B: int, n_aug: int, aug_pos: Optional[torch.Tensor], aug_neg: Optional[torch.Tensor],
                 users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_valid: torch.Tensor):
    """llmrec_sample_batch: this rank's slice of the step's BPR triples + the LLM-augmented triples, written
    into the given (static) buffers; step_dev (int64[1], device) is the step counter the launch advances."""
    _need_gpu(step_dev, exist_users, users, pos, neg, n_valid)
    if users.numel() < B + n_aug or step_dev.dtype != torch.int64 or n_valid.dtype != torch.int32:
        raise RuntimeError("sample_batch: buffers of B + n_aug int64 entries, int64 step counter, int32 n_valid expected")
    _lib.call("llmrec_sample_batch", seed, _p(step_dev), exist_users.numel(), _p(exist_users), n_items, _p(train.rowptr), _p(train.colidx),
              B_global, slice_begin, B, n_aug, _p(aug_pos), _p(aug_neg), _p(users), _p(pos), _p(neg), _p(n_valid), _stream())


def sample_batch_wide(seed: int, step_dev: torch.Tensor, exist_users: torch.Tensor, n_items: int, train: Csr, B_global: int,
                      slice_begin: int, B: int, n_aug: int, aug_pos: Optional[torch.Tensor], aug_neg: Optional[torch.Tensor],
                      users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_valid: torch.Tensor, ticket: torch.Tensor):
    """llmrec_sample_batch_wide: sample_batch's outputs by several blocks; ticket (int32[1], device, zero before the first call) is the
    word the blocks count themselves off on - the launch leaves it at zero."""
    _need_gpu(step_dev, exist_users, users, pos, neg, n_valid, ticket)
    if users.numel() < B + n_aug or step_dev.dtype != torch.int64 or n_valid.dtype != torch.int32 or ticket.dtype != torch.int32:
        raise RuntimeError("sample_batch_wide: buffers of B + n_aug int64 entries, int64 step counter, int32 n_valid and ticket expected")
    _lib.call("llmrec_sample_batch_wide", seed, _p(step_dev), exist_users.numel(), _p(exist_users), n_items, _p(train.rowptr), _p(train.colidx),
              B_global, slice_begin, B, n_aug, _p(aug_pos), _p(aug_neg), _p(users), _p(pos), _p(neg), _p(n_valid), _p(ticket), _stream())


# the tensor tags of llmrec_dropout_rows_f32 the fused step uses (a tag names a tensor: tensors of one step draw independent masks)
DROPOUT_TAG_ITEM_STREAMS = 0      # the [I, S d] projected item-side streams (image, text, attributes): column = slice * d + j
DROPOUT_TAG_USER_PROFILE = 1      # P_usr, the projected user profile


def dropout_rows_(X: torch.Tensor, p: float, seed: int, step_dev: torch.Tensor, tag: int, ticket: Optional[torch.Tensor] = None):
    """llmrec_dropout_rows_f32: inverted dropout of the 2-D fp32 view X IN PLACE (inner stride 1, any row stride) with the counter-based mask
    of (seed, step_dev[0], tag, row, column) the header states. step_dev: one 64-bit integer on the device; ticket (int32[1], device, zero
    before the first call): the launch also advances step_dev by 1 - without it the counter is only read. Returns X."""
    _need_gpu(X, step_dev, ticket)
    if X.dtype != torch.float32 or X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1) or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        raise RuntimeError("dropout_rows_: a 2-D fp32 view with inner stride 1 expected (the launch writes in place)")
    if step_dev.dtype not in (torch.int64, torch.uint64) or step_dev.numel() < 1 or (ticket is not None and ticket.dtype != torch.int32):
        raise RuntimeError("dropout_rows_: a 64-bit integer step counter and an int32 ticket expected")
    _lib.call("llmrec_dropout_rows_f32", X.shape[0], X.shape[1], _p(X), _ld(X), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(tag),
              _p(ticket), _stream())
    return X


# R13: feature masking and attribute restoration (include/llmrec_hip.h states every contract)
K_MASK = 0x6A09E667F3BCC908           # the node lists' key: seed ^ K_MASK
MASK_SIDE_USERS, MASK_SIDE_ITEMS = CONST["LLMREC_MASK_SIDE_USERS"], CONST["LLMREC_MASK_SIDE_ITEMS"]
MASK_ROW_LANES = CONST["LLMREC_MASK_ROW_LANES"]
RESTORE_LOSS_TYPES = {"sce": CONST["LLMREC_RESTORE_SCE"], "mse": CONST["LLMREC_RESTORE_MSE"]}


def _views(ts: Sequence[torch.Tensor], what: str, width: Optional[int] = None):
    """(host array of the views' addresses, their common leading dimension): 2-D fp32 GPU views of one shape with inner stride 1."""
    _need_gpu(*ts)
    t0 = ts[0]
    for t in ts:
        if (t.dtype != torch.float32 or t.dim() != 2 or t.shape != t0.shape or (t.shape[1] > 1 and t.stride(1) != 1) or _ld(t) != _ld(t0)
                or (width is not None and t.shape[1] != width)):
            raise RuntimeError("%s: 2-D fp32 views of one shape and row stride with inner stride 1 expected" % what)
    return (_c.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), _ld(t0)


def mask_nodes(N: int, m: int, seed: int, step_dev: torch.Tensor, side: int, out: Optional[torch.Tensor] = None,
               ticket: Optional[torch.Tensor] = None) -> torch.Tensor:
    """llmrec_mask_nodes: the m distinct masked ids of [0, N) of round step_dev[0] and `side` as int64 [m]; with a ticket (int32[1],
    zero before the first call) the launch also advances the round."""
    _need_gpu(step_dev, out, ticket)
    if step_dev.dtype not in (torch.int64, torch.uint64) or (ticket is not None and ticket.dtype != torch.int32):
        raise RuntimeError("mask_nodes: a 64-bit integer round counter and an int32 ticket expected")
    if out is None:
        out = torch.empty(max(int(m), 1), dtype=torch.int64, device=step_dev.device)
    if out.dtype != torch.int64 or out.numel() < m or not out.is_contiguous():
        raise RuntimeError("mask_nodes: a contiguous int64 buffer of at least m entries expected")
    _lib.call("llmrec_mask_nodes", int(N), int(m), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(side), _p(out), _p(ticket), _stream())
    return out[:m]


def _sums_table(sums: Sequence[torch.Tensor], cols: int, what: str):
    _need_gpu(*sums)
    if any(s.dtype != torch.float64 or s.numel() != cols or not s.is_contiguous() for s in sums):
        raise RuntimeError("%s: one contiguous float64 [cols] tensor of sums per view expected" % what)
    return (_c.c_void_p * len(sums))(*[s.data_ptr() for s in sums])


def col_sums(Xs: Sequence[torch.Tensor], sums: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """llmrec_col_sums_f64: the fp64 column sums of the equally shaped views Xs, from scratch, by the header's fixed tree."""
    xp, ldx = _views(Xs, "col_sums")
    N, cols = Xs[0].shape
    if sums is None:
        sums = [torch.empty(cols, dtype=torch.float64, device=Xs[0].device) for _ in Xs]
    _lib.call("llmrec_col_sums_f64", len(Xs), xp, ldx, _sums_table(sums, cols, "col_sums"), N, cols, _stream())
    return list(sums)


def mask_rows_(Xs: Sequence[torch.Tensor], sums: Sequence[torch.Tensor], nodes: torch.Tensor):
    """llmrec_mask_rows_f32: one masking round IN PLACE - rows `nodes` (int64, distinct, device) of every view become the column mean
    taken from the running sums, which follow."""
    xp, ldx = _views(Xs, "mask_rows_")
    N, cols = Xs[0].shape
    _need_gpu(nodes)
    if nodes.dtype != torch.int64 or not nodes.is_contiguous() or len(sums) != len(Xs):
        raise RuntimeError("mask_rows_: a contiguous int64 node list and one sums tensor per view expected")
    _lib.call("llmrec_mask_rows_f32", len(Xs), xp, ldx, _sums_table(sums, cols, "mask_rows_"), N, cols, _p(nodes), nodes.numel(), _stream())


def restore_loss(Xs: Sequence[torch.Tensor], Ts: Sequence[torch.Tensor], nodes: torch.Tensor, W: torch.Tensor, b: torch.Tensor,
                 loss_type: str, alpha: float, row_loss: torch.Tensor, loss_out: torch.Tensor, dXs: Optional[Sequence[torch.Tensor]] = None,
                 scale: float = 1.0, row_flags: Optional[torch.Tensor] = None, row_stamp: Optional[torch.Tensor] = None):
    """llmrec_restore_loss_f32: per stream s, loss_out[s] = the restoration loss of decoder(Xs[s][nodes]) against Ts[s][nodes] and, with
    dXs, dXs[s][nodes] += scale * its gradient. row_loss: fp32 [len(Xs) * len(nodes)] scratch (the per-row terms stay readable)."""
    d, F = W.shape[1], W.shape[0]
    xp, ldx = _views(Xs, "restore_loss", d)
    tp, ldt = _views(Ts, "restore_loss", F)
    dp, lddx = _views(dXs, "restore_loss", d) if dXs is not None else (None, 0)
    _need_gpu(nodes, W, b, row_loss, loss_out, row_flags, row_stamp)
    m, n = nodes.numel(), len(Xs)
    if (len(Ts) != n or (dXs is not None and len(dXs) != n) or nodes.dtype != torch.int64 or not nodes.is_contiguous()
            or W.dtype != torch.float32 or W.stride(1) != 1 or b.dtype != torch.float32 or b.numel() != F or not b.is_contiguous()
            or row_loss.dtype != torch.float32 or row_loss.numel() < n * m or loss_out.dtype != torch.float32 or loss_out.numel() < n
            or not row_loss.is_contiguous() or not loss_out.is_contiguous()):
        raise RuntimeError("restore_loss: mismatched streams, node list, decoder or output buffers")
    _lib.call("llmrec_restore_loss_f32", n, xp, ldx, tp, ldt, dp, lddx, _p(nodes), m, d, F, _p(W), _ld(W), _p(b), RESTORE_LOSS_TYPES[loss_type],
              float(alpha), float(scale), _p(row_loss), _p(loss_out), _p(row_flags), _p(row_stamp), _stream())


def restore_finish(values: Optional[torch.Tensor], rate: float, scal: Optional[torch.Tensor], running: Optional[torch.Tensor],
                   views: Sequence[torch.Tensor] = (), nodes: Optional[torch.Tensor] = None):
    """llmrec_restore_finish_f32: scal[1] += rate * sum(values) (and running[0], in double); rows `nodes` of `views` become zero."""
    vp, ld = _views(views, "restore_finish") if len(views) else (None, 0)
    _need_gpu(values, scal, running, nodes)
    _lib.call("llmrec_restore_finish_f32", 0 if values is None else values.numel(), _p(values), float(rate), _p(scal), _p(running), len(views), vp,
              ld, views[0].shape[1] if len(views) else 0, _p(nodes), nodes.numel() if nodes is not None else 0, _stream())


def topk_metrics(idx: torch.Tensor, hits: torch.Tensor, query_users: torch.Tensor, test_rowptr: torch.Tensor, Ks) -> torch.Tensor:
    """Per-user [n, 4, len(Ks)] float64 (precision, recall, ndcg, hit_ratio) on the device (llmrec_topk_metrics)."""
    _need_gpu(idx, hits, query_users, test_rowptr)
    n, K = idx.shape
    Ks = [int(k) for k in Ks]
    out = torch.empty(n, 4, len(Ks), dtype=torch.float64, device=idx.device)
    arr = (_c.c_int32 * len(Ks))(*Ks)
    _lib.call("llmrec_topk_metrics", n, _p(query_users.to(torch.int64).contiguous()), K, _p(hits.contiguous()), _p(idx.contiguous()),
              _p(test_rowptr), len(Ks), arr, _p(out), _stream())
    return out


# ---------------------------------------------------------------------------------------------
# Checkpoint snapshot: many tensors <-> one arena in one launch (csrc/snapshot.hip)
# ---------------------------------------------------------------------------------------------
PACK_MAX_SEGMENTS, PACK_ALIGN = CONST["LLMREC_PACK_MAX_SEGMENTS"], CONST["LLMREC_PACK_ALIGN"]


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def pack_layout(nbytes: Sequence[int]):
    """(offsets, arena_bytes) of an arena that holds segments of these sizes in this order, each at a multiple of PACK_ALIGN
    (llmrec_pack_arena_bytes: host arithmetic, no device)."""
    n = len(nbytes)
    b, o = (_c.c_int64 * max(n, 1))(*[int(x) for x in nbytes]), (_c.c_int64 * max(n, 1))()
    total = _lib.query("llmrec_pack_arena_bytes", n, b, o)
    if total < 0:
        raise ValueError("pack_layout: a negative size, or a total beyond 2^63")
    return [int(x) for x in o[:n]], total


def pack_segments(tensors: Sequence[torch.Tensor], offsets: Sequence[int], arena: torch.Tensor, direction: int):
    """direction 0: arena[offsets[i] ...] = the bytes of tensors[i], every other byte of the arena = 0; direction 1: the bytes of
    tensors[i] = arena[offsets[i] ...] (llmrec_pack_segments, on the current stream; no synchronisation). The tensors are contiguous
    device tensors of any dtype and alignment; the arena is a contiguous uint8 device tensor. One launch per PACK_MAX_SEGMENTS
    tensors: each launch owns the slice of the arena from its first segment's offset to the next launch's (the first from 0, the last to
    the arena's end), so the offsets of more than PACK_MAX_SEGMENTS tensors ascend (pack_layout's do). Returns the number of launches."""
    n = len(tensors)
    if len(offsets) != n or arena.dtype != torch.uint8 or not arena.is_contiguous():
        raise RuntimeError("pack_segments: one offset per tensor and a contiguous uint8 arena expected")
    _need_gpu(arena, *tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise RuntimeError("pack_segments: contiguous tensors expected")
    if n > PACK_MAX_SEGMENTS and any(offsets[i] > offsets[i + 1] for i in range(n - 1)):
        raise RuntimeError("pack_segments: more than %d segments need ascending offsets" % PACK_MAX_SEGMENTS)
    total, launches = arena.numel(), 0
    for lo in range(0, max(n, 1), PACK_MAX_SEGMENTS):
        group = range(lo, min(lo + PACK_MAX_SEGMENTS, n))
        base = int(offsets[lo]) if lo > 0 else 0
        end = int(offsets[lo + PACK_MAX_SEGMENTS]) if lo + PACK_MAX_SEGMENTS < n else total
        k = max(len(group), 1)
        ptrs = (_c.c_void_p * k)(*[tensors[i].data_ptr() for i in group])
        size = (_c.c_int64 * k)(*[_nbytes(tensors[i]) for i in group])
        offs = (_c.c_int64 * k)(*[int(offsets[i]) - base for i in group])
        _lib.call("llmrec_pack_segments", len(group), ptrs, size, offs, _c.c_void_p(arena.data_ptr() + base), end - base, int(direction), _stream())
        launches += 1
    return launches
