"""Fused training step: the whole Stage-2 step - sampler included - as a fixed sequence of HIP launches over preallocated buffers (16 at
the benchmark's shape on one stream, FusedStep.entry_point_calls_per_step; more on four streams, where nothing is grouped), with the
backward pass written out by hand (no autograd graph), captured into one HIP graph; likewise an evaluation (forward + scoring + top-K).

Same arithmetic as the modular path (Models.MM_Model.forward + llmrec_amd.engine.train_step, i.e. reference Models.py:127-199 +
main.py:228-278); what changes is the organisation:
  * the seven item-side streams (image, text, 5 attributes) travel as ONE [rows, 7d] operand, so the 16 side-feature SpMMs of the
    reference (Models.py:152-167) become 4 (+4 in backward) - 2 + 2 when the constant products A_ui F_k are pre-propagated at set-up -
    and the adjacency indices are read once per direction instead of seven times;
  * the 8 BPR + prune losses (main.py:232-254) are two launches on the critical path (scores - which also begin the step on the device:
    row stamp, AdamW's counter - and selection + gradient rows) and one beside it (the loss values, the feature regulariser from the
    fusion launch's partial sums, the logged scalars);
  * projections and weight gradients of the constant feature matrices are grouped launches (8 projections in one; all four Linears'
    gradients, row-listed, in one, with their AdamW in the reduction launch) in split-precision bf16x3 arithmetic (LLMREC_GEMM=f32: exact);
  * independent products share grouped SpMM launches on ONE stream - the sampler, the scatter plan with the reach marks and the loss
    values ride three of them as guests (_Rider), and the ID chain's first product rides the projection launch as its trailing blocks
    (host_chain), and the first product of its backward without a partner runs in the CUs the weight-gradient launch leaves free
    (host_wgrad) - or run as chains on four HIP streams (LLMREC_STREAMS=1: fork/join = graph edges);
  * the embedding tables' AdamW reads its gradient where it is formed (the user table's is inv * dE_u) and the row-wise clean-up of the
    scatter targets rides in the item table's AdamW launch;
  * nothing allocates or synchronises, so the step replays from a HIP graph (``capture()``): no per-launch host cost, which dominates here.
Falls outside its scope (use the modular path) unless the step is built for it: dropout > 0 (drop_rate=: the project's own counter-based
masks on the device, llmrec_dropout_rows_f32 - step_options.resolve, "DROPOUT") and --mask / --mask_rate > 0 (mask_rate=, mask_items=, the
decoder and targets: llmrec_mask_nodes' lists, running column sums, the restoration launches - _mask_round, _restore).
Schedule switches that remain: LLMREC_STREAMS=1 (four streams), LLMREC_FOLD=0 (the separate small launches) and LLMREC_HOST_CHAIN=0 / fwd (no hosted
product: the chain's products in SpMM launches of their own / the forward's hosted only) are the A/B references of the default schedule; LLMREC_PREPROPAGATE, LLMREC_GEMM and LLMREC_WGRAD_ROWS choose the arithmetic's organisation. The class switches
FOLD = False, INLINE_ADAMW = False and WGRAD_ROWS = False are DataParallelStep's (llmrec_amd/dp.py: its replicas all-reduce the
gradients before AdamW). Every switch is decided in ONE place, llmrec_amd/step_options.py (resolve(): a pure function of the variables,
the shapes and the class switches, with each switch's rationale and measured figures); FusedStep.__init__ copies its record and allocates.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
from collections import namedtuple
from itertools import zip_longest
from typing import Callable, Optional

import torch

from . import _lib, ops, step_options
from .engine import Hyper

_p, _ld, _c = ops._p, ops._ld, ctypes


def _call(name, *a):
    _lib.call(name, *a, ops._stream())


def _raw(args):
    """An argument tuple as an entry point takes it: tensors (and None) as pointers. The same tuple builds the guest descriptor (ops.guest_*)."""
    return [_p(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]


@contextlib.contextmanager
def _capture_without_gc(graph, multi_branch: bool):
    """torch.cuda.graph(g) with Python's cyclic garbage collector held off for the duration of the capture. torch.cuda.graph collects
    garbage once, on entry; the body of a captured step then creates tens of thousands of container objects (ctypes argument arrays,
    tuples), so generation-0/1/2 collections run INSIDE the capture and may finalise whatever cyclic garbage exists by then - a
    previously imported drop-in module with its device tensors, an older step object with its graph executables - i.e. free device
    memory and destroy executables in the middle of a stream capture. Hygiene, not a fix for anything observed: the host fault round 4
    chased through the GPU suite turned out to be hipGraphLaunch's own (llmrec_amd/__init__.py)."""
    from . import require_graph_replay
    require_graph_replay("llmrec_amd: stream capture", multi_branch)   # single-branch graphs only (llmrec_amd/__init__.py)
    capture = torch.cuda.graph(graph, capture_error_mode="thread_local")   # other threads (the RCCL watchdog) may touch the runtime
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        with capture:
            yield
    finally:
        if was_enabled:
            gc.enable()


class _Rider:
    """A launch of the step that may ride in a grouped SpMM launch. run(): the launch by its own entry point(s), on the current stream;
    guest: None, or a callable returning the same launch as a guest descriptor (ops.SpmmGuestC); rode: called when the guest launch was
    accepted. FusedStep._spmm_group(jobs, rider) decides: the guest launch, or - refused, or no guest - run() right ahead of the
    group's usual launches. Calling a rider runs it."""
    def __init__(self, run: Callable, guest: Optional[Callable] = None, rode: Optional[Callable] = None):
        self.run, self.guest, self.rode = run, guest, rode

    def __call__(self):
        self.run()


class _TrainStep:
    """What ONE training step hands from its forward to its backward, created by step_eager() and passed down as an argument: an
    evaluation's forward() has none, so it cannot advance AdamW, emit the regulariser's partial sums or consume reach marks.
    ride: the step's sampler, plan and loss values ride SpMM launches; ev_plan / ev_reach: four streams - the scatter plan / the weight
    gradient's row list are ready; reach_pending: the batch whose reach flags are marked and wait for the fusion launch's compaction."""
    def __init__(self, ride: bool = False):
        self.ride, self.ev_plan, self.ev_reach, self.reach_pending = ride, None, None, None


# one captured evaluation: the graph and everything it reads or writes (sums / auc_sum: pinned, None without a held-out set / auc=True)
_EvalGraph = namedtuple("_EvalGraph", "graph idx scores q train ws sums sums_ws held auc_sum auc_ws")


class FusedStep:
    # resident blocks the weight-gradient launch is laid out for (llmrec_wgrad_target_t.block_budget; 0 = 256, one per CU). A block of
    # that launch owns its CU's whole register file, so a 256-block round starves whatever runs beside it: the ID chain's last SpMM took
    # 81 us beside it and 12 us alone and, once the row list had shortened the GEMM, had become the step's tail. 224 blocks leave 32 CUs
    # free: 256 / 240 / 224 / 208 / 192 blocks -> 0.474 / 0.459 / 0.454 / 0.456 / 0.469 ms per step on one box (measured on four streams,
    # LLMREC_STREAMS=1, where the other streams' kernels use those CUs). On ONE stream - the default - nothing else is in flight, and
    # the 32 CUs run the ID chain's hosted backward product inside the same launch (host_wgrad, _host_wgrad_applies). The budget cannot
    # move without changing dW's bits: it sets the slab length (csrc/dense.hip: wgrad_multi_slab_rows), i.e. the summation partition.
    wgrad_blocks = 224
    WGRAD_ROWS = INLINE_ADAMW = FOLD = True      # schedule switches of the class: DataParallelStep (llmrec_amd/dp.py) turns all three off
    # A step whose batch capacity b_max is ABOVE this takes the WIDE loss segment (llmrec_bpr_*_wide*: the scatter plan by a multi-block
    # sort, the selection by the exact multi-block radix select, each problem in a workspace block of its own) instead of the launches
    # that stage the batch in LDS and refuse b_max > LLMREC_BPR_MAX_B. The route depends on b_max alone, not on any process-wide switch
    # (main.py builds such a step under LLMREC_FUSED=wide only: step_options.route); up to LLMREC_BPR_MAX_B both segments leave the same
    # bits everywhere (tests lower WIDE_FROM to run the wide one at a small batch). The wide selection is 8 launches (init, four
    # histogram passes, the ties' count, the write pass, the backward rows) against 2, its plan 4 (keys, two sorts, run lengths) against 1.
    WIDE_FROM = _lib.CONST["LLMREC_BPR_MAX_B"]

    def __init__(self, model, graph, hp: Hyper, rates, optimizer: ops.FusedAdamW, b_max: int, drop_rate: float = 0.0, drop_seed: int = 0,
                 mask_rate: float = 0.0, mask_items: bool = False, mask_seed: int = 0, decoder=None, user_targets=None, item_targets=None,
                 att_re_rate: float = 0.0, feat_loss_type: str = "sce", alpha_l: float = 2.0):
        """model: Models.MM_Model (parameters + constant feature tensors); graph: ops.BipartiteGraph
        or any object with .ui/.iu SparseOperands; rates: (model_cat, user_cat, item_cat); drop_rate / drop_seed: dropout on the eight
        projections inside the step (reference Models.py:145-150; step_options.resolve, "DROPOUT") - 0 = none: the step is what it is without the option.
        mask_rate / mask_items / mask_seed: feature masking inside the step (reference Models.py:130-142; _mask_round) - every forward
        overwrites int(mask_rate * n_users) rows of model.user_feats and, with mask_items (--mask), int(mask_rate * n_items) rows of every
        attribute feature matrix with the column mean, in place and cumulatively; the lists are llmrec_mask_nodes' stream of
        (mask_seed, round, side), not torch.randperm's. decoder (Models.Decoder), user_targets [U, F] / item_targets {key: [I, F]} (the
        unmasked embeddings), att_re_rate, feat_loss_type ("sce" / "mse") and alpha_l: the restoration term of main.py:258-273, added
        with mask_items and att_re_rate != 0 (_restore). The defaults leave the step exactly what it is."""
        self.m, self.hp, self.opt = model, hp, optimizer
        self.ui, self.iu = graph.ui, graph.iu
        self.U, self.I = model.n_users, model.n_items
        self.d = d = model.embedding_dim
        self.L = model.n_ui_layers
        self.keys = list(model.item_feats.keys())
        self.S = S = 2 + len(self.keys)                      # item-side streams: image, text, attributes
        self.c_m, self.c_u, self.c_a = rates
        self.b_max = b_max
        self.wide = b_max > self.WIDE_FROM                 # the loss segment's route: b_max alone
        if b_max > _lib.CONST["LLMREC_BPR_WIDE_MAX_B"]:
            raise RuntimeError("FusedStep: b_max %d exceeds LLMREC_BPR_WIDE_MAX_B = %d" % (b_max, _lib.CONST["LLMREC_BPR_WIDE_MAX_B"]))
        # every switch of the step - multi_stream, gemm, preprop, wgrad_rows, inline_adamw, fold, bwd_mask, bwd_zero_skip, host_chain,
        # host_wgrad, check_zero and the validated drop_rate - is decided once, with its rationale, in step_options.resolve(); below: allocation only
        self.mask_rate, self.mask_items, self.mask_seed = float(mask_rate), bool(mask_items), int(mask_seed)
        if not 0.0 <= self.mask_rate <= 1.0 or (self.mask_items and self.mask_rate == 0):      # (false for a NaN)
            raise ValueError("FusedStep: mask_rate %r outside [0, 1], or mask_items without a rate" % (mask_rate,))
        if self.mask_rate > 0 and drop_rate != 0:
            raise RuntimeError("FusedStep: feature masking and dropout inside one step are not supported")
        self.m_users = int(self.mask_rate * self.U)
        self.m_items = int(self.mask_rate * self.I) if self.mask_items else 0
        if self.mask_items and (self.m_users == 0 or self.m_items == 0 or not self.keys):
            # (the reference's restoration loss is then the mean over no rows, NaN: the per-op path's to produce - step_options.route)
            raise RuntimeError("FusedStep: mask_items with an empty user or item list")
        self.att_re_rate = float(att_re_rate)
        self.restore = self.mask_items and self.att_re_rate != 0
        opts = step_options.resolve(None, n_users=self.U, n_items=self.I, d=d, n_attr=len(self.keys), drop_rate=drop_rate,
                                    wgrad_rows_default=self.WGRAD_ROWS, inline_adamw_default=self.INLINE_ADAMW, fold_default=self.FOLD,
                                    bwd_nnz=self.iu.bwd.nnz, bwd_valued=self.iu.bwd.val is not None,
                                    bwd_col_scaled=self.iu.bwd.col_scale is not None, latency_nnz=ops.SPMM_LATENCY_NNZ,
                                    mask_items=self.mask_items, restore=self.restore)
        for name, value in opts._asdict().items():
            setattr(self, name, value)
        self.drop_seed = int(drop_seed)
        dev = model.item_id_embedding.weight.device
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        U, I = self.U, self.I
        # forward buffers
        self.U_cat, self.I_cat = f(U, S * d), f(I, S * d)
        self.P_usr, self.prof_i, self.prof_u = f(U, d), f(I, d), f(U, d)
        self.Ul = [f(U, d) for _ in range(self.L)]
        self.Il = [f(I, d) for _ in range(self.L)]
        self.E_u, self.E_i = f(U, d), f(I, d)
        # backward buffers
        # The loss backward scatters into buffers that are all-zero between steps - dE_u / dE_i and the sc_* sources of the fusion
        # backward - and clears exactly the rows it touched afterwards (llmrec_bpr_multi_zero_rows_f32); the fusion backward
        # writes d*_cat = source + its own term (llmrec_fuse_bwd_src_f32). No dense memset of the six gradient buffers (70 MB
        # per step at the Netflix shape; measured -2.2 % of the step in round 2). (check_zero asserts that invariant before every scatter.)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.dE_u, self.dE_i = z(U, d), z(I, d)
        self.sc_U, self.sc_I, self.sc_prof = z(U, 2 * d), z(I, S * d), z(U, d)
        # one byte per row, stamped by the loss launch for the rows of the batch with the step's stamp (a device counter: nothing is ever
        # cleared, no reader races a clean-up): the fusion backward writes the ~90 % of rows no sample touched (zero gradient, zero
        # sources) without reading them. (The same stamps offered to the transposed side product as a mask over ALL its slices, with the
        # mask bytes loaded at gather time, bought nothing in round 3; restricted to the attribute slices, read on the device and with
        # the in-place skip they do: bwd_mask, step_options.resolve.)
        self.flag_u = torch.zeros(U, dtype=torch.uint8, device=dev)
        self.flag_i = torch.zeros(I, dtype=torch.uint8, device=dev)
        self.row_stamp = torch.zeros(1, dtype=torch.int32, device=dev)     # advanced by the scores launch (LLMREC_ROW_STAMP)
        # the batch's deterministic scatter plan (llmrec_bpr_scatter_plan: sorted (id, slot) keys + run lengths), built right behind the
        # sampler: the loss backward adds the rows several samples share in one fixed order - no float atomics, same-seed runs agree bit for bit
        self.bpr_plan = torch.zeros(max(ops.bpr_plan_words(b_max), 1), dtype=torch.int64, device=dev)
        # running sums (double) of the logged scalars [loss, mf, emb] over the steps since the caller last cleared them: the epoch line of
        # reference main.py:280-283 without any host-side arithmetic between graph replays
        self.epoch_sums = torch.zeros(3, dtype=torch.float64, device=dev)
        self.dU_cat, self.dI_cat = f(U, S * d), f(I, S * d)
        self.dprof_u, self.dprof_i, self.dP_usr = f(U, d), f(I, d), f(U, d)
        self.bufU, self.bufI, self.tmpU, self.tmpI = f(U, d), f(I, d), f(U, d), f(I, d)
        self.out = f(8, 2)
        self.saved = f(8 * ops.bpr_saved_floats(b_max))
        self.scal = f(4)                                     # [feat_reg, loss, mf, emb]
        if self.wide:                                        # the wide loss segment's workspaces (its own launches initialise them)
            self.ws_plan_wide = ops.bpr_plan_wide_workspace(b_max, dev)
            self.ws_sel_wide = ops.bpr_multi_wide_workspace(1 + S, b_max, dev)
        self.ws_sumsq = torch.empty(_lib.query("llmrec_sumsq_workspace_bytes", 0, 0), dtype=torch.uint8, device=dev)
        feats = [model.image_feats, model.text_feats, model.user_feats] + [model.item_feats[k] for k in self.keys]
        ws = max(_lib.query("llmrec_linear_wgrad_workspace_bytes", x.shape[0] * (len(self.keys) if i >= 3 else 1), d, x.shape[1])
                 for i, x in enumerate(feats))
        self.ws_wgrad = torch.empty(ws, dtype=torch.uint8, device=dev)
        wsq = lambda x: torch.empty(_lib.query("llmrec_linear_wgrad_workspace_bytes", x.shape[0], d, x.shape[1]), dtype=torch.uint8, device=dev)
        # one workspace per weight gradient that may be in flight at the same time (user / text / image run beside item_trans')
        self.ws_wgrad_b, self.ws_wgrad_c, self.ws_wgrad_d = wsq(model.user_feats), wsq(model.text_feats), wsq(model.image_feats)
        self.ws_wgrad_multi = None                           # sized at the first backward (needs the gradient tensors)
        self._partials = {}
        self.s1, self.s2, self.s3 = (torch.cuda.Stream(device=dev) for _ in range(3))
        for p in model.parameters():
            if p.requires_grad and p.grad is None and p is not model.batch_norm.weight and p is not model.batch_norm.bias:
                p.grad = torch.zeros_like(p)
        # loss weights of the 8 BPR problems (main.py:273): main (mf + emb), image/text (mm_mf_rate), attributes (aug_mf_rate)
        self.w_mf = [1.0, hp.mm_mf_rate, hp.mm_mf_rate] + [hp.aug_mf_rate] * len(self.keys)
        self.w_emb = [1.0] + [0.0] * (S)
        self.n_prob = 1 + S
        if self.n_prob > _lib.CONST["LLMREC_BPR_MAX_PROBLEMS"]:
            raise RuntimeError("FusedStep: %d BPR problems exceed LLMREC_BPR_MAX_PROBLEMS" % self.n_prob)
        self.graph_exec = None
        self.graph_multi, self.graph_unroll = None, 0        # capture(batcher=, unroll=): a graph of `unroll` steps
        self.batcher = self._capture_args = None             # capture()'s in-graph sampler and its arguments (check_wgrad_geometry re-captures)
        self.static = self._last_eval = None
        self._eval_graphs = {}                               # key -> _EvalGraph (_last_eval: the one replayed last)
        # measurement only (bench.py `roofline`): a uint64 tensor of STAMP_SLOTS device timestamps written by llmrec_timestamp launches around
        # the step, the projection launch and the weight-gradient launches - the durations INSIDE a replayed graph, which cannot carry events
        self.stamps = None
        self.spmm_edge_units = 0.0                            # edge traversals (nnz x d / 64) of the SpMM launches of the last step built
        if self.drop_rate > 0:                               # the masks' step counter and its launch's count-off (step_options: DROPOUT)
            self.drop_step = torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64)
            self.drop_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.mask_rate > 0:
            # the masking round's counter with its launch's count-off, the round's node lists (read again by the restoration launches)
            # and one fp64 running column sum per masked tensor (_mask_round)
            self.mask_step = torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64)
            self.mask_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            self.mask_nodes_u = torch.zeros(max(self.m_users, 1), dtype=torch.int64, device=dev)[:self.m_users]
            self.mask_nodes_i = torch.zeros(max(self.m_items, 1), dtype=torch.int64, device=dev)[:self.m_items]
            self._masked_user, self._masked_items = [model.user_feats], [model.item_feats[k] for k in self.keys] if self.mask_items else []
            self.user_sums = [torch.zeros(model.user_feats.shape[1], dtype=torch.float64, device=dev)]
            self.item_sums = [torch.zeros(x.shape[1], dtype=torch.float64, device=dev) for x in self._masked_items]
            self.refresh_feature_sums()
        if self.restore:
            if decoder is None or user_targets is None or item_targets is None or feat_loss_type not in ops.RESTORE_LOSS_TYPES:
                raise RuntimeError("FusedStep: the restoration term needs the decoder, both target sets and feat_loss_type sce or mse")
            if d != 64 or S > 2 + _lib.CONST["LLMREC_MASK_MAX_TENSORS"]:
                raise RuntimeError("FusedStep: the restoration launches are compiled for d = 64 and at most %d attribute streams"
                                   % _lib.CONST["LLMREC_MASK_MAX_TENSORS"])
            as_target = lambda x: torch.as_tensor(x).detach().to(device=dev, dtype=torch.float32).contiguous()
            self.decoder, self.feat_loss_type, self.alpha_l = decoder, feat_loss_type, float(alpha_l)
            self.user_targets, self.item_targets = as_target(user_targets), [as_target(item_targets[k]) for k in self.keys]
            self.re_rows_u, self.re_rows_i = f(self.m_users), f(len(self.keys) * self.m_items)     # the per-row terms (scratch)
            self.re_vals = z(1 + len(self.keys))                                                   # [user, attribute k ...] stream losses
        if not self.preprop:
            self.P_cat, self.dP_cat = f(I, S * d), f(I, S * d)        # the projected features and their gradient (reference order)
        else:
            item_feats = [model.image_feats, model.text_feats] + [model.item_feats[k] for k in self.keys]
            self.AX = [self._propagate_constant(self.ui.fwd, x) for x in item_feats]
            self.a_rowsum = ops.spmm_raw(self.ui.fwd, torch.ones(I, 4, dtype=torch.float32, device=dev))[:, 0].contiguous()   # A_ui 1
            self.ws_colsum = torch.empty(_lib.query("llmrec_weighted_colsum_workspace_bytes", S * d), dtype=torch.uint8, device=dev)
        if self.wgrad_rows:
            self.act_flags = torch.zeros(U + 16, dtype=torch.uint8, device=dev)[:U]   # all-zero between calls (readable in 16-byte words)
            self.act_rows = torch.zeros(U + 32, dtype=torch.int32, device=dev)
            self.act_n = torch.zeros(1, dtype=torch.int32, device=dev)
            self.act_expected = None      # rows the launch geometry is laid out for: set from the first step's count (capture() / step_eager())
        if self.fold:
            self.ss_cap = 2 * 2048                                # >= the fusion launch's grid (two problems, <= 2048 blocks each)
            self.ss_partial = torch.zeros(self.ss_cap, dtype=torch.float32, device=dev)
            self.ss_n = 0
        self._refuse_guests = False                           # tests: treat every guest launch as refused (the separate calls run)
        self._block_slots = 2 * torch.cuda.get_device_properties(dev).multi_processor_count     # the projection keeps >= 2 blocks per CU
        self._emb_params = [model.user_id_embedding.weight, model.item_id_embedding.weight]
        self._lin_params = [p for p in optimizer.params if p.grad is not None and all(p is not e for e in self._emb_params)]
        # (Four streams: launch = capture order at the fork points decides which branch the graph runs behind its parent without a cross-queue
        # hand-off, ~10 us. Measured one at a time in round 2, profiles/README.md: the forward's side-feature SpMMs are captured before the
        # profile chain, the BPR backward before the regulariser / loss assembly, -3.6 % together; the other fork points are neutral or lose.)

    # -- raw kernel helpers -----------------------------------------------------------------------
    @staticmethod
    def _propagate_constant(a: ops.Csr, X: torch.Tensor) -> torch.Tensor:
        """A X for a constant feature matrix, 64 columns at a time (set-up only)."""
        X = X.detach()
        out = torch.empty(a.n_rows, X.shape[1], dtype=torch.float32, device=X.device)
        step = 64 if X.shape[1] % 64 == 0 else X.shape[1]
        for c0 in range(0, X.shape[1], step):
            ops.spmm_raw(a, X[:, c0:c0 + step], out=out[:, c0:c0 + step])
        return out

    def _fork(self, *streams):
        if self.multi_stream:
            cur = torch.cuda.current_stream()
            for st in streams:
                st.wait_stream(cur)

    def _mark(self):
        """An event at the current point of the current stream (a fork point that side streams may wait for later)."""
        if not self.multi_stream:
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def _fork_from(self, ev, *streams):
        if self.multi_stream:
            for st in streams:
                st.wait_event(ev)

    def _join(self, *streams):
        if self.multi_stream:
            cur = torch.cuda.current_stream()
            for st in streams:
                cur.wait_stream(st)

    def _on(self, st):
        """Context: launch on side stream `st` (or stay on the current stream when disabled)."""
        return torch.cuda.stream(st) if self.multi_stream else torch.cuda.stream(torch.cuda.current_stream())

    STAMP_SLOTS = 6       # step begin, projection begin / end, weight gradient begin / end (reduction included), step end

    def _stamp(self, slot: int):
        if self.stamps is not None:
            _call("llmrec_timestamp", self.stamps.data_ptr() + 8 * slot)

    def _spmm_args(self, a: ops.Csr, X, Y, accumulate=False, tag=0, epilogue=None, mask=None):
        """(slice width, plan, partials, epilogue) of one product. tag: one partial-sum scratch per concurrent chain - and so per problem
        of a grouped launch. mask (accumulate only): (row bytes, stamp counter, first masked slice) of ops.spmm_epilogue's slice-ranged mask."""
        d = X.shape[1]
        sw, pl = a.plan_for(d, whole_row=epilogue is not None and epilogue.op != ops.EPI_NONE)
        partials = None
        if pl.n_seg:
            key = (id(pl), d, tag)
            partials = self._partials.get(key)
            if partials is None:
                partials = self._partials[key] = torch.empty(pl.n_seg * d, dtype=torch.float32, device=X.device)
        if accumulate:
            m = dict(x_row_mask=mask[0], x_mask_stamp=mask[1], mask_from_slice=mask[2]) if mask is not None else {}
            epilogue = ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y, **m)
        return sw, pl, partials, epilogue

    def _spmm(self, a: ops.Csr, X, Y, accumulate=False, tag=0, epilogue=None, mask=None):
        """Y = epilogue(A X) (llmrec_spmm_f32); accumulate: Y += A X. tag: one partial-sum scratch per concurrent chain. (A refused mask
        raises: bwd_mask promised the shape, and the fusion backward has already left the masked rows unwritten.)"""
        d = X.shape[1]
        self.spmm_edge_units += a.nnz * (d / 64.0)
        sw, pl, partials, epilogue = self._spmm_args(a, X, Y, accumulate, tag, epilogue, mask)
        rp, ci = pl.csr_of(a)
        _call("llmrec_spmm_f32", a.n_rows, a.n_cols, _p(rp), _p(ci), _p(a.val), _p(a.row_scale), _p(a.col_scale),
              _p(X), _ld(X), _p(Y), _ld(Y), d, sw, _c.byref(pl.c_struct()), _p(partials),
              _c.byref(epilogue) if epilogue is not None else None)

    def _spmm_jobs(self, jobs):
        for a, X, Y, kw in jobs:
            self._spmm(a, X, Y, **kw)

    def _check_batch(self, B: int):
        if B > self.b_max:
            raise RuntimeError("FusedStep: batch of %d exceeds b_max %d" % (B, self.b_max))

    def _spmm_group(self, jobs, rider: Optional[_Rider] = None):
        """Independent products [(a, X, Y, kwargs of _spmm)] in ONE llmrec_spmm_multi_f32 launch, longest first (one stream: each of these
        latency-bound products alone leaves most CUs idle). Separate launches when the group has one product, when a graph is in the
        HBM-bound regime (nnz >= ops.SPMM_LATENCY_NNZ: one product fills the chip) or when the library refuses the group. Bit-identical
        either way: a row's summation tree does not depend on the launch it runs in.
        rider: a short launch that depends on nothing the chip is busy with. With a guest descriptor it rides as the first blocks of this
        group's launch (llmrec_spmm_multi_guest_f32; a group of one product too); refused, or without one, it runs by its own entry
        point right ahead of the group's usual launches."""
        jobs = [j for j in jobs if j is not None]
        groupable = not (self.multi_stream or any(a.nnz >= ops.SPMM_LATENCY_NNZ for a, _, _, _ in jobs))
        as_guest = rider is not None and rider.guest is not None and groupable and not self._refuse_guests
        probs, keep = self._spmm_problems(jobs) if as_guest or (groupable and len(jobs) > 1) else (None, None)
        guest = rider.guest() if as_guest else None                      # (None: no guest form after all - the replicas' sampler)
        launched = guest is not None and ops.spmm_multi_guest(probs, guest)
        if launched and rider.rode is not None:
            rider.rode()
        if rider is not None and not launched:
            rider()
        if not launched and groupable and len(jobs) > 1:
            launched = ops.spmm_multi(probs)
        if not launched:
            return self._spmm_jobs(jobs)
        for a, X, _, _ in jobs:
            self.spmm_edge_units += a.nnz * (X.shape[1] / 64.0)

    def _spmm_problems(self, jobs):
        """(the llmrec_spmm_problem_t of each job, longest first; what they point into)"""
        order = sorted(jobs, key=lambda j: -j[0].nnz * j[1].shape[1])             # (stable)
        probs, keep = [], []
        for a, X, Y, kw in order:
            sw, pl, partials, epi = self._spmm_args(a, X, Y, **kw)
            rp, ci = pl.csr_of(a)
            pc = pl.c_struct()
            keep.append(epi)
            probs.append(ops.SpmmProblemC(a.n_rows, a.n_cols, rp.data_ptr(), ci.data_ptr(), ops._ptr(a.val), ops._ptr(a.row_scale),
                                          ops._ptr(a.col_scale), X.data_ptr(), _ld(X), Y.data_ptr(), _ld(Y), X.shape[1], sw,
                                          _c.addressof(pc), ops._ptr(partials), _c.addressof(epi) if epi is not None else None))
        return probs, keep

    def _linear(self, X, lin, out):
        _call("llmrec_linear_fwd_f32", X.shape[0], self.d, X.shape[1], _p(X), _ld(X), _p(lin.weight), _ld(lin.weight), _p(lin.bias),
              _p(out), _ld(out))

    def projection_jobs(self):
        """(X, Linear, out, bias_scale) of the step's 8 projections (Models.py:145-150), longest K first: the launch's tail then
        consists of the short (512 / 768-wide) work units. Pre-propagated: the item-side operands are A_ui F_k and land in U_cat."""
        m = self.m
        if self.preprop:
            lins = [m.image_trans, m.text_trans] + [m.item_trans] * len(self.keys)
            jobs = [(self.AX[s_], lins[s_], self._side(self.U_cat, s_), self.a_rowsum) for s_ in range(self.S)]
        else:
            jobs = [(m.item_feats[key], m.item_trans, self._side(self.P_cat, 2 + k), None) for k, key in enumerate(self.keys)]
            jobs += [(m.text_feats, m.text_trans, self._side(self.P_cat, 1), None), (m.image_feats, m.image_trans, self._side(self.P_cat, 0), None)]
        jobs.append((m.user_feats, m.user_trans, self.P_usr, None))
        jobs.sort(key=lambda j: -j[0].shape[1])
        return jobs

    def wgrad_targets(self, dY_cat, dP_usr):
        """The step's weight gradients as llmrec_linear_wgrad_multi targets [(pairs, dW, db, accumulate)]: item_trans (5 attribute
        streams), user_trans, text_trans, image_trans. dY_cat = the [rows, 7 d] gradient of the projections' outputs (dU_cat when
        the operands are pre-propagated - its pairs carry the row weights of the bias gradient - else dP_cat)."""
        m = self.m
        if self.preprop:
            feats, roww = self.AX, self.a_rowsum
        else:
            feats, roww = [m.image_feats, m.text_feats] + [m.item_feats[key] for key in self.keys], None
        rows = (self.act_rows, self.act_n, self.act_expected) if self.wgrad_rows else None
        item_pairs = [(self._side(dY_cat, 2 + k), feats[2 + k], roww, rows) for k in range(len(self.keys))]
        return [(item_pairs, m.item_trans.weight.grad, m.item_trans.bias.grad, False),
                ([(dP_usr, m.user_feats)], m.user_trans.weight.grad, m.user_trans.bias.grad, False),
                ([(self._side(dY_cat, 1), feats[1], roww)], m.text_trans.weight.grad, m.text_trans.bias.grad, False),
                ([(self._side(dY_cat, 0), feats[0], roww)], m.image_trans.weight.grad, m.image_trans.bias.grad, False)]

    def _project_all(self):
        """All 8 projections in one grouped launch (d <= 64), else one by one."""
        jobs = self.projection_jobs()
        if self.d > 64 or len(jobs) > _lib.CONST["LLMREC_LINEAR_MAX_PROBLEMS"]:
            if self.preprop:
                raise RuntimeError("FusedStep: the pre-propagated projection needs the grouped launch (d <= 64); set LLMREC_PREPROPAGATE=0")
            for X, lin, out, _ in jobs:
                self._linear(X, lin, out)
            return
        arr = self._projection_problems(jobs)
        _call("llmrec_linear_fwd_grouped_bf16x3" if self.gemm == "bf16x3" else "llmrec_linear_fwd_grouped_f32", len(jobs), arr, self.d)

    @staticmethod
    def _projection_problems(jobs):
        return ops.linear_problems([(X, lin.weight, lin.bias, out, bscale) for X, lin, out, bscale in jobs])

    def _project_all_hosting(self, job) -> bool:
        """_project_all() with the independent product `job` (a, X, Y, kwargs of _spmm) as TRAILING blocks of the grouped launch
        (llmrec_linear_fwd_grouped_host_spmm_bf16x3). False: nothing was launched - hosting is off, the launch has no tail to fill
        (no more work units than block slots: the product would only queue behind the projection), or the library refuses the pair -
        and the caller issues _project_all() and the product as before. Bit-identical either way."""
        a, X, Y, kw = job
        jobs = self.projection_jobs()
        if not (self.host_chain and not self._refuse_guests and not self.multi_stream and self.gemm == "bf16x3" and self.d == 64
                and len(jobs) <= _lib.CONST["LLMREC_LINEAR_MAX_PROBLEMS"] and a.nnz < ops.SPMM_LATENCY_NNZ
                and kw.get("epilogue") is None and not kw.get("accumulate")
                and sum(-(-j[0].shape[0] // 128) for j in jobs) > self._block_slots):
            return False
        probs, keep = self._spmm_problems([job])
        arr = self._projection_problems(jobs)
        if not _lib.call_unless_unsupported("llmrec_linear_fwd_grouped_host_spmm_bf16x3", len(jobs), arr, self.d, _c.byref(probs[0]),
                                            ops._stream()):
            return False
        del keep
        self.spmm_edge_units += a.nnz * (X.shape[1] / 64.0)
        return True

    def _wgrad(self, dY, X, lin, accumulate, ws=None):
        ops.linear_wgrad_grouped([(dY, X)], lin.weight.grad, lin.bias.grad, accumulate, self.ws_wgrad if ws is None else ws,
                                 precision=self.gemm)

    def _dropout(self, backward: bool = False):
        """The step's two dropout launches (drop_rate > 0): the item-side streams, then the user profile - the projections in the
        forward, their gradients (the same masks: the counter has not moved) in the backward, whose second launch carries the ticket
        and so advances the counter: it is the step's last reader of it."""
        cat, usr = (self.dP_cat, self.dP_usr) if backward else (self.P_cat, self.P_usr)
        ops.dropout_rows_(cat, self.drop_rate, self.drop_seed, self.drop_step, ops.DROPOUT_TAG_ITEM_STREAMS)
        ops.dropout_rows_(usr, self.drop_rate, self.drop_seed, self.drop_step, ops.DROPOUT_TAG_USER_PROFILE,
                          ticket=self.drop_ticket if backward else None)

    def refresh_feature_sums(self):
        """The running column sums of the masked feature tensors from scratch (llmrec_col_sums_f64): at set-up, and after anything but
        the step itself has written model.user_feats / model.item_feats."""
        if self.mask_rate > 0:
            ops.col_sums(self._masked_user, self.user_sums)
            if self._masked_items:
                ops.col_sums(self._masked_items, self.item_sums)

    def _mask_round(self):
        """One masking round ahead of a forward, training and evaluation alike (reference Models.py:131-142): the round's node lists,
        then the listed rows of user_feats - and, with mask_items, of the attribute matrices (one launch for all of them: they share
        the list) - become the column mean of the tensor as it stood before this round (llmrec_mask_rows_f32: no re-read of the
        matrices). Read / write sets:
          node launches  read the round counter; write the lists. The LAST one carries the ticket and advances the counter, so a
                    replayed graph draws new lists with no host action. The lists' previous readers (the last step's restoration
                    and clean-up launches) precede them in stream order.
          row launches   read the lists and the running sums; write the listed rows and the sums. Their first reader is the
                    projection launch, behind them on the same stream; no pre-propagated operand holds a masked tensor
                    (step_options.resolve, MASKING)."""
        ops.mask_nodes(self.U, self.m_users, self.mask_seed, self.mask_step, ops.MASK_SIDE_USERS, out=self.mask_nodes_u,
                       ticket=None if self.mask_items else self.mask_ticket)
        if self.mask_items:
            ops.mask_nodes(self.I, self.m_items, self.mask_seed, self.mask_step, ops.MASK_SIDE_ITEMS, out=self.mask_nodes_i, ticket=self.mask_ticket)
        if self.m_users:
            ops.mask_rows_(self._masked_user, self.user_sums, self.mask_nodes_u)
        if self.mask_items:
            ops.mask_rows_(self._masked_items, self.item_sums, self.mask_nodes_i)

    def _att_slices(self, cat):
        return [self._side(cat, 2 + k) for k in range(len(self.keys))]

    def _restore(self):
        """The restoration term (reference main.py:258-271; restore = mask_items and att_re_rate != 0), behind the loss backward's
        scatter and ahead of the fusion backward: the user stream for its value only (the reference detaches its input), the
        attribute streams in one launch whose gradient rows go into the scatter source of dI_cat's attribute slices. Read / write sets:
          user launch   reads prof_u, the user targets, decoder.u_net and the user list; writes re_rows_u and re_vals[0].
          attribute launch   reads I_cat's attribute slices, the item targets, decoder.i_net and the item list; adds att_re_rate x the
                    gradient into rows `list` of sc_I's attribute slices - behind the selection launch's scatter into the same buffer
                    (stream order), ahead of their one reader, the fusion backward - and stamps those rows in flag_i with the step's
                    stamp (the scores launch advanced it), so that the fusion backward reads them; writes re_rows_i and re_vals[1:].
        What the step otherwise assumes about these rows is off: bwd_mask / bwd_zero_skip / wgrad_rows (step_options.resolve,
        RESTORATION); _restore_finish clears them."""
        u_net, i_net = self.decoder.u_net[0], self.decoder.i_net[0]
        ops.restore_loss([self.prof_u], [self.user_targets], self.mask_nodes_u, u_net.weight.detach(), u_net.bias.detach(), self.feat_loss_type,
                         self.alpha_l, self.re_rows_u, self.re_vals[:1])
        ops.restore_loss(self._att_slices(self.I_cat), self.item_targets, self.mask_nodes_i, i_net.weight.detach(), i_net.bias.detach(),
                         self.feat_loss_type, self.alpha_l, self.re_rows_i, self.re_vals[1:], dXs=self._att_slices(self.sc_I),
                         scale=self.att_re_rate, row_flags=self.flag_i, row_stamp=self.row_stamp)

    def _restore_finish(self):
        """The restoration term's tail, ONE launch behind everything else of the step: att_re_rate x the stream losses joins the logged
        loss (scal[1], epoch_sums[0] - written by the loss-value launch, earlier on this stream or joined), and the list's rows of
        sc_I's attribute slices, read by the fusion backward, go back to zero: the scatter targets stay all-zero between steps."""
        ops.restore_finish(self.re_vals, self.att_re_rate, self.scal, self.epoch_sums, views=[self.sc_I[:, 2 * self.d:]], nodes=self.mask_nodes_i)

    def _softmax_bwd(self, Y, dY, dZ, alpha: float = 1.0):
        _call("llmrec_softmax_rows_bwd_scaled_f32", Y.shape[0], self.d, float(alpha), _p(Y), _ld(Y), _p(dY), _ld(dY), _p(dZ), _ld(dZ))

    def _axpy(self, alpha, X, Y, accumulate, rows=None, cols=None):
        rows = X.shape[0] if rows is None else rows
        cols = X.shape[1] if cols is None else cols
        _call("llmrec_axpy_f32", rows, cols, float(alpha), None, _p(X), _ld(X), _p(Y), _ld(Y), 1 if accumulate else 0)

    def _side(self, cat, s):
        return cat[:, s * self.d:(s + 1) * self.d]

    def _norm_terms(self, cat, prof):
        """[image, text, profile, attributes...] in the reference's order of addition (Models.py:188-197)."""
        return [self._side(cat, 0), self._side(cat, 1), prof] + [self._side(cat, 2 + k) for k in range(len(self.keys))]

    def _rates(self):
        r = [self.c_m, self.c_m, self.c_u] + [self.c_a] * len(self.keys)
        return (_c.c_float * len(r))(*r)

    # -- forward ----------------------------------------------------------------------------------
    def forward(self, profile_on_main: bool = False, mask: bool = True):
        """The evaluation's forward (no training step: it advances and consumes nothing - but, with mask_rate > 0, it is one masking
        round, as the reference's). profile_on_main: the profile chain stays on the current stream (the evaluation's graph, see
        eval_topk); mask=False: without the masking launches (the warm-up run ahead of an evaluation's capture)."""
        self._forward(None, profile_on_main=profile_on_main, mask=mask)

    def _train_forward(self, sampler: Optional[_Rider] = None, after_chain: Optional[_Rider] = None, step: Optional[_TrainStep] = None):
        """The forward of a training step (step_eager's riders and record; DataParallelStep, which runs its own backward, passes none)."""
        self._forward(step if step is not None else _TrainStep(), sampler, after_chain)

    def _forward(self, step: Optional[_TrainStep], sampler=None, after_chain=None, profile_on_main: bool = False, mask: bool = True):
        """step: the training step this forward belongs to, None = evaluation. sampler / after_chain: launches for the ID chain's stream,
        ahead of / behind its SpMMs (the batch and what is derived from it). mask: with mask_rate > 0, begin with the masking round."""
        m, d = self.m, self.d
        if mask and self.mask_rate > 0:
            self._mask_round()
        if self.multi_stream:
            self._forward_streams(step, sampler, after_chain, profile_on_main)
        else:
            self._forward_one_stream(step, sampler, after_chain)

        # E_u and E_i (Models.py:185-197) in ONE launch: llmrec_fuse_fwd_multi_f32 (two independent row ranges)
        keep = []

        def problem(pr, out, base, layers, cat, prof):
            means, norms = [base] + layers, self._norm_terms(cat, prof)
            mp, ml = ops._ptr_table(means)
            npt, nl = ops._ptr_table(norms)
            rates = self._rates()
            keep.extend((mp, ml, npt, nl, rates))
            pr.rows, pr.mean_scale, pr.n_mean, pr.n_norm = out.shape[0], 1.0 / len(means), len(means), len(norms)
            pr.mean_terms, pr.mean_ld = _c.cast(mp, _c.c_void_p), _c.cast(ml, _c.c_void_p)
            pr.norm_terms, pr.norm_ld, pr.rates = _c.cast(npt, _c.c_void_p), _c.cast(nl, _c.c_void_p), _c.cast(rates, _c.c_void_p)
            pr.out, pr.ldo = out.data_ptr(), _ld(out)
        arr = (ops.FuseFwdProblem * 2)()
        problem(arr[0], self.E_i, m.item_id_embedding.weight, self.Il, self.I_cat, self.prof_i)
        problem(arr[1], self.E_u, m.user_id_embedding.weight, self.Ul, self.U_cat, self.prof_u)
        if self.fold and step is not None:                               # + the regulariser's sum of squares over the image / text streams (terms 0, 1)
            n_part = _c.c_int32(0)
            pending, step.reach_pending = step.reach_pending, None
            if pending is not None and _lib.call_unless_unsupported(         # + the reach flags' compaction as the launch's first block
                    "llmrec_fuse_fwd_multi_sumsq_compact_f32", 2, arr, d, 2, _p(self.ss_partial), self.ss_cap, _c.byref(n_part),
                    self.iu.fwd.n_cols, _p(self.act_flags), _p(self.act_rows), _p(self.act_n), ops._stream()):
                pending = None
            else:
                _call("llmrec_fuse_fwd_multi_sumsq_f32", 2, arr, d, 2, _p(self.ss_partial), self.ss_cap, _c.byref(n_part))
            if pending is not None:                                      # refused: the list by its own two launches (marking again changes nothing)
                ops.batch_reach_rows(*pending, self.iu.fwd, self.act_flags, self.act_rows, self.act_n)
            self.ss_n = int(n_part.value)
        else:
            _call("llmrec_fuse_fwd_multi_f32", 2, arr, d)

    def _chain_fwd_jobs(self):
        """The ID chain's 2 L products [(a, X, Y, kwargs)] in dependency order; the last layer's carry the row softmax as the epilogue."""
        jobs, i_prev = [], self.m.item_id_embedding.weight
        for l in range(self.L):
            kw = dict(tag=2, epilogue=ops.spmm_epilogue(ops.EPI_SOFTMAX)) if l == self.L - 1 else dict(tag=2)
            jobs.append((self.ui.fwd, i_prev, self.Ul[l], kw))
            jobs.append((self.iu.fwd, self.Ul[l], self.Il[l], dict(kw)))
            i_prev = self.Il[l]
        return jobs

    def _forward_one_stream(self, step, sampler, after_chain):
        """The forward's products on ONE stream, as dependency groups of grouped SpMM launches: the k-th product of the ID chain, of the
        side chain and of the profile chain share a launch (_spmm_group). The chain runs behind the projection so that its first two layers
        pair with the side and profile products.
        sampler / after_chain are step_eager's riders (given only where they ride: step.ride): the sampler rides the FIRST group's launch
        and after_chain - the scatter plan and the reach marks - the chain's third product, which runs alone. A rider without a guest
        descriptor runs ahead of the projection. Read / write sets:
          sampler   reads its tables (users with interactions, the train CSR, the augmented pairs) and the step counter; writes users / pos /
                    neg / n_valid, the counter and its ticket. The first group reads the ID tables, the projections P_cat / U_cat and P_usr
                    and writes U_1, I_cat, prof_i: disjoint. The batch's last reader of the previous step, the item table's clean-up launch,
                    precedes this launch in stream order; its first reader is the plan, two launches later.
          plan + marks   read the batch and the by-item CSR; write the plan buffer and the reach flags. Their host reads I_1 and writes U_2;
                    the flags are consumed by the fusion launch's compaction block, two launches later, the plan by the loss backward.
        HOSTED (self.host_chain, _project_all_hosting): the chain's first product runs as trailing blocks of the projection launch and the
        groups are those of chain[1:] - with L = 2 {I_1, I_cat, prof_i}, {U_2, prof_u}, {I_2}: three launches instead of four.
          hosted product   reads the item ID table, last written by the previous step's item-table AdamW / clean-up launch (earlier in stream
                    order), and writes U_1; the projection's units read the features and the Linears and write U_cat / P_cat and P_usr: disjoint.
          sampler   rides the first group as before: that group now reads U_1, U_cat and P_usr and writes I_1, I_cat, prof_i.
          plan + marks   ride the group that runs alone, now the last one (it reads U_2 and writes I_2); their readers - the fusion launch's
                    compaction block and the loss backward - still follow it in stream order.
        DROPOUT (drop_rate > 0, training forward only): two launches between the projection launch and the first group.
          dropout   reads the dropout counter (last written by the previous step's backward, earlier in stream order) and P_cat / P_usr,
                    written by the projection launch's units; writes P_cat / P_usr in place, read first by the first group. A hosted
                    product's U_1 is not touched. Neither launch carries the ticket: the counter stays where it is until the backward."""
        if sampler is not None and sampler.guest is None:
            sampler()
        if step is not None and not self.fold:
            self.opt.advance()
        if after_chain is not None and after_chain.guest is None:        # (reads the batch only)
            after_chain()
        chain = self._chain_fwd_jobs()
        self._stamp(1)
        if chain and self._project_all_hosting(chain[0]):
            chain = chain[1:]
        else:
            self._project_all()
        self._stamp(2)
        if step is not None and self.drop_rate > 0:
            self._dropout()
        side = [(self.ui.fwd, self.P_cat, self.U_cat, {})] if not self.preprop else []
        side.append((self.iu.fwd, self.U_cat, self.I_cat, {}))
        prof = [(self.iu.fwd, self.P_usr, self.prof_i, dict(tag=1)), (self.ui.fwd, self.prof_i, self.prof_u, dict(tag=1))]
        groups = list(zip_longest(chain, side, prof))                    # (two at least: the profile chain's)
        # the riders' hosts: the sampler's is the first group, the plan's comes behind it - the chain's third product where there is one
        hosts = {0: sampler, min(2, len(groups) - 1): after_chain}
        for k, jobs in enumerate(groups):
            rider = hosts.get(k)
            self._spmm_group(jobs, rider if rider is not None and rider.guest is not None else None)
        if step is not None and not self.fold:
            self._feat_reg()

    def _forward_streams(self, step, sampler, after_chain, profile_on_main):
        """The forward's products on four streams (LLMREC_STREAMS=1: the A/B reference of the one-stream schedule)."""
        self._fork(self.s2)
        with self._on(self.s2):                                          # ID chain: needs no projection
            if sampler is not None:                                      # the batch is first read by the losses, after the join below:
                sampler()                                                # sampling rides beside the projection instead of ahead of it
            if step is not None and not self.fold:
                self.opt.advance()                                       # AdamW's step counter / bias corrections, off the critical path
            self._spmm_jobs(self._chain_fwd_jobs())
            ev_chain = self._mark() if after_chain is not None else None     # the chain's SpMMs are done; what follows on this stream
            if after_chain is not None:                                      # is not needed by the fusion
                after_chain()
        self._stamp(1)
        self._project_all()
        self._stamp(2)
        if step is not None and self.drop_rate > 0:                      # (ahead of ev1: the profile stream reads the dropped P_usr)
            self._dropout()
        ev1 = self._mark()
        if not self.preprop:
            self._spmm(self.ui.fwd, self.P_cat, self.U_cat)              # 7 streams, one adjacency pass
        self._spmm(self.iu.fwd, self.U_cat, self.I_cat)
        if profile_on_main:
            self._spmm(self.iu.fwd, self.P_usr, self.prof_i, tag=1)
            self._spmm(self.ui.fwd, self.prof_i, self.prof_u, tag=1)
        else:
            self._fork_from(ev1, self.s1)
            with self._on(self.s1):                                      # profile stream: items first
                self._spmm(self.iu.fwd, self.P_usr, self.prof_i, tag=1)
                self._spmm(self.ui.fwd, self.prof_i, self.prof_u, tag=1)
        if step is not None and not self.fold:                           # training: the feature regulariser's value needs only U_cat / I_cat -
            self._fork(self.s3)                                          # captured HERE it runs beside the fusion and the BPR launches (captured
            with self._on(self.s3):                                      # after the BPR backward, round 2, the graph ran it last: the step's tail)
                self._feat_reg()
        if ev_chain is not None:
            self._join(self.s1)
            torch.cuda.current_stream().wait_event(ev_chain)                     # (not the stream's tail: after_chain's launches are joined later)
        else:
            self._join(self.s1, self.s2)

    def outputs(self):
        """The reference's 14-tuple as views of the forward buffers (Models.py:199)."""
        att_i = {k: self._side(self.I_cat, 2 + j) for j, k in enumerate(self.keys)}
        att_u = {k: self._side(self.U_cat, 2 + j) for j, k in enumerate(self.keys)}
        return (self.E_u, self.E_i, self._side(self.I_cat, 0), self._side(self.I_cat, 1), self._side(self.U_cat, 0),
                self._side(self.U_cat, 1), self.P_usr, att_i, self.prof_u, self.prof_i, att_u, att_i, None, None)

    # -- losses + backward ------------------------------------------------------------------------
    def _problems(self):
        arr = (ops.BprProblem * self.n_prob)()
        tabs = [(self.E_u, self.E_i, self.dE_u, self.dE_i)]
        tU, tI, tP = self.sc_U, self.sc_I, self.sc_prof
        for s in range(2):
            tabs.append((self._side(self.U_cat, s), self._side(self.I_cat, s), self._side(tU, s), self._side(tI, s)))
        for k in range(len(self.keys)):
            tabs.append((self.prof_u, self._side(self.I_cat, 2 + k), tP, self._side(tI, 2 + k)))
        for i, (eu, ei, deu, dei) in enumerate(tabs):
            arr[i].Eu, arr[i].ldu, arr[i].Ei, arr[i].ldi = eu.data_ptr(), _ld(eu), ei.data_ptr(), _ld(ei)
            arr[i].dEu, arr[i].lddu, arr[i].dEi, arr[i].lddi = deu.data_ptr(), _ld(deu), dei.data_ptr(), _ld(dei)
            arr[i].g_mf, arr[i].g_emb = self.w_mf[i], self.w_emb[i]
        return arr

    def loss_backward(self, users, pos, neg, n_valid=None, step: Optional[_TrainStep] = None):
        """The 8 losses and the whole backward behind _train_forward(). step: step_eager's record (None: nothing to wait for, nothing rides)."""
        step = step if step is not None else _TrainStep()
        B = users.numel()
        self._check_batch(B)
        probs = self._problems()
        hp = self.hp
        remember = float(1 - hp.prune_loss_drop_rate)
        # critical path: scores -> [selection + gradient rows] (two launches); the loss VALUES are beside it (below)
        self._check_scatter_targets()
        if step.ev_plan is not None:                                     # (four streams: the plan was built behind the ID chain)
            torch.cuda.current_stream().wait_event(step.ev_plan)
        # the scores launch begins the step (row stamp; folded: AdamW's counter too), the selection stamps the batch's rows
        scores = (self.n_prob, probs, self.d, _p(users), _p(pos), _p(neg), B, _p(n_valid), _p(self.saved), _p(self.row_stamp))
        select = (self.n_prob, probs, self.d, _p(users), _p(pos), _p(neg), B, _p(n_valid), remember, float(hp.decay), float(hp.batch_size),
                  _p(self.saved), _p(self.flag_u), _p(self.flag_i), _p(self.row_stamp), _p(self.bpr_plan))
        if self.fold:
            o = self.opt
            if o.dev_state is None:
                o.dev_state = torch.zeros(3, dtype=torch.float32, device=self.E_u.device)
            _call("llmrec_bpr_multi_scores_wide_f32" if self.wide else "llmrec_bpr_multi_scores_step_f32", *scores, _p(o.dev_state), o.lr,
                  o.betas[0], o.betas[1])
        elif self.wide:
            _call("llmrec_bpr_multi_scores_wide_f32", *scores, None, 0.0, 0.0, 0.0)         # (the row stamp only)
        else:
            _call("llmrec_bpr_multi_scores_f32", *scores)
        if self.wide:
            _call("llmrec_bpr_multi_select_bwd_wide_f32", *select, _p(self.ws_sel_wide), self.ws_sel_wide.numel())
        else:
            _call("llmrec_bpr_multi_select_bwd_f32", *select)
        if self.restore:
            self._restore()
        # The loss values and the logged scalars, on the ID chain's stream (_backward places them: a branch of their own right behind the BPR
        # launches - the graph ran it as the step's tail). Folded: ONE launch - loss values + regulariser (the fusion launch's partial sums) +
        # assembly - and, where the step's riders apply, the same launch as a guest of the backward's first SpMM group (_backward_one_stream).
        losses = (self.n_prob, B, n_valid, remember, float(hp.decay), float(hp.batch_size), self.out, self.saved)
        reg = (self.ss_partial, self.ss_n, float(hp.feat_reg_decay * 0.5 / self.I), self.scal, self.epoch_sums) if self.fold else None

        def folded():
            _call("llmrec_bpr_multi_losses_wide_f32" if self.wide else "llmrec_bpr_multi_losses_assemble_f32", *_raw(losses),
                  (_c.c_float * self.n_prob)(*self.w_mf), *_raw(reg))

        def unfolded():
            if self.wide:
                _call("llmrec_bpr_multi_losses_wide_f32", *_raw(losses), None, None, 0, 0.0, None, None)   # (the loss values only)
            else:
                _call("llmrec_bpr_multi_losses_f32", *_raw(losses))
            self._join(self.s3)                  # the regulariser's value (s3, during the forward)
            self._assemble_loss(0)               # loss = sum_p w_mf[p] * mf_p + emb_0 + feat_reg
        values = _Rider(folded, (lambda: ops.guest_losses(*losses, self.w_mf, *reg)) if step.ride else None) if self.fold else _Rider(unfolded)
        self._backward(probs, users, pos, neg, n_valid, bpr_bwd_done=True, side_work=values, ev_reach=step.ev_reach)
        if not self.fold:
            self._join(self.s3)
        if self.restore:
            self._restore_finish()

    def _assemble_loss(self, mode: int, tail=None, inv_world: float = 1.0):
        """Logged scalars (main.py:273,280-283) from the 8 BPR results + the regulariser: one single-wave launch."""
        w = (_c.c_float * self.n_prob)(*self.w_mf)
        _call("llmrec_loss_assemble_f32", mode, self.n_prob, _p(self.out), w, _p(self.scal), _p(tail), float(inv_world),
              _p(self.epoch_sums) if mode != 1 else None)

    def _feat_reg(self):
        """Feature regulariser (main.py:151-156) over the image/text columns of both cat buffers -> scal[0]."""
        coef = self.hp.feat_reg_decay * 0.5 / self.I
        for k, blk in enumerate((self.I_cat, self.U_cat)):
            _call("llmrec_sumsq_f32", blk.shape[0], 2 * self.d, _p(blk), _ld(blk), float(coef), k, _p(self.scal), _p(self.ws_sumsq),
                  self.ws_sumsq.numel())

    def _check_scatter_targets(self):
        if self.check_zero and not torch.cuda.is_current_stream_capturing():
            dirty = [n for n, t in (("dE_u", self.dE_u), ("dE_i", self.dE_i), ("sc_U", self.sc_U), ("sc_I", self.sc_I), ("sc_prof", self.sc_prof))
                     if float(t.abs().max()) != 0.0]
            if dirty:
                raise RuntimeError("FusedStep: scatter targets not all-zero before the loss backward: %s (an aborted step? call reset_scatter_targets())" % dirty)

    def _backward(self, probs, users, pos, neg, n_valid, replicated_scale: float = 1.0, bpr_bwd_done: bool = False, side_work=None,
                  ev_reach=None):
        """Hand-written backward from the saved BPR state to the parameter gradients (and, with inline_adamw, the update).
        replicated_scale weights the batch-independent loss terms (1 / world on batch-sharded replicas, whose
        gradients are summed over ranks afterwards). bpr_bwd_done: the loss launch already scattered the gradient rows.
        side_work: launches for the ID chain's stream, ahead of its last SpMM (loss_backward's rider); ev_reach: four streams - the event
        behind the weight gradient's row list."""
        hp = self.hp
        if not bpr_bwd_done:
            self._check_scatter_targets()
            _call("llmrec_bpr_multi_bwd_f32", self.n_prob, probs, self.d, _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid),
                  float(hp.decay), float(hp.batch_size), _p(self.saved), _p(self.bpr_plan))
        # dE_u / dE_i hold the scattered rows now. (Only the fused loss launch stamps the rows it touched; keep: alive until the launch.)
        fuse, keep = self._fuse_bwd_problems(hp.feat_reg_decay * 0.5 / self.I * replicated_scale, stamped=bpr_bwd_done)
        schedule = self._backward_streams if self.multi_stream else self._backward_one_stream
        deferred = schedule(probs, (users, pos, neg, n_valid), fuse, side_work, masked=bpr_bwd_done and self.bwd_mask)
        if self.drop_rate > 0:
            self._dropout_backward()
        self._weight_gradients(ev_reach, deferred)
        self._join(self.s2)
        if self.fold and side_work is not None:                          # (four streams: side_work ran on a stream of its own)
            self._join(self.s3)

    def _dropout_backward(self):
        """drop_rate > 0: the forward's two masks on dP_cat and dP_usr, between the schedule that forms them and the weight gradients -
        the only readers of either. Read / write sets:
          dP_cat launch   reads the counter and dP_cat, written by the side chain's last transposed product (the current stream); writes dP_cat.
          dP_usr launch   reads the counter and dP_usr, written by the profile chain's last transposed product (one stream: the same
                    group as dP_cat's; four streams: s1, joined here first); writes dP_usr, and - the ticket - the counter and the ticket
                    word. It is the step's last reader of the counter, and nothing runs beside it that reads it: the other three readers
                    precede it on this stream, and what the ID chain's stream still has queued (its products, the clean-up, the item
                    table's AdamW) reads neither the counter nor a projection's gradient.
        user_trans' exact-fp32 weight gradient, which the schedules otherwise issue right behind the profile chain, follows here: it reads
        the dropped dP_usr."""
        self._join(self.s1)
        self._dropout(backward=True)
        if self.gemm != "bf16x3":
            self._wgrad(self.dP_usr, self.m.user_feats, self.m.user_trans, False, ws=self.ws_wgrad_b)

    def _fuse_bwd_problems(self, coef: float, stamped: bool):
        """The backward of both fusions as the two problems of ONE launch (llmrec_fuse_bwd_src_multi_f32) -> (problems, the arrays they
        point into). stamped: the loss launch stamped the batch's rows; the others are written without being read."""
        keep = []

        def problem(pr, dout, cat, prof, dcat, dprof, srcs, flags):
            norms, dnorms = self._norm_terms(cat, prof), self._norm_terms(dcat, dprof)
            npt, nl = ops._ptr_table(norms)
            dp, dl = ops._ptr_table(dnorms)
            # sources = what the loss backward scattered for this side (terms in _norm_terms order: image, text, profile, attributes);
            # the feature regulariser's gradient on the image / text streams (terms 0, 1) rides along: 2 coef x
            sp = (_c.c_void_p * len(srcs))(*[t.data_ptr() if t is not None else None for t in srcs])
            sl = (_c.c_int64 * len(srcs))(*[_ld(t) if t is not None else 0 for t in srcs])
            rates = self._rates()
            keep.extend((npt, nl, dp, dl, sp, sl, rates))
            pr.rows, pr.dOut, pr.lddo, pr.n_norm = dout.shape[0], dout.data_ptr(), _ld(dout), len(norms)
            pr.norm_terms, pr.norm_ld, pr.rates = _c.cast(npt, _c.c_void_p), _c.cast(nl, _c.c_void_p), _c.cast(rates, _c.c_void_p)
            pr.d_terms, pr.d_ld = _c.cast(dp, _c.c_void_p), _c.cast(dl, _c.c_void_p)
            pr.src_terms, pr.src_ld = _c.cast(sp, _c.c_void_p), _c.cast(sl, _c.c_void_p)
            pr.n_reg_terms, pr.reg_two_coef = 2, float(2.0 * coef)
            if stamped:
                pr.row_flags, pr.row_stamp = flags.data_ptr(), self.row_stamp.data_ptr()
        arr = (ops.FuseBwdProblem * 2)()
        if stamped and self.bwd_zero_skip:                               # the attribute terms (behind image, text, profile) of idle item rows:
            arr[0].zero_skip_from_term = 3                               # their only reader, the masked side product, skips those rows
        problem(arr[0], self.dE_i, self.I_cat, self.prof_i, self.dI_cat, self.dprof_i,
                [self._side(self.sc_I, 0), self._side(self.sc_I, 1), None] + [self._side(self.sc_I, 2 + k) for k in range(len(self.keys))], self.flag_i)
        problem(arr[1], self.dE_u, self.U_cat, self.prof_u, self.dU_cat, self.dprof_u,
                [self._side(self.sc_U, 0), self._side(self.sc_U, 1), self.sc_prof] + [None] * len(self.keys), self.flag_u)
        return arr, keep

    def _chain_head(self, side_work, fuse=None):
        """Head of the ID chain's backward: the user table's gradient and AdamW (U^0 only enters the mean: its gradient needs nothing else),
        the logged scalars (side_work), the first softmax backward. The first two go first: whatever this stream still has queued when the
        weight-gradient GEMM takes every CU (about when the chain's last SpMM starts) waits for its blocks to retire and becomes the step's tail.
        fuse: the fusion backward's problems when it shares the head's launch (one stream, folded step): it, the AdamW and the softmax
        backward are independent and adjacent - ONE launch (llmrec_step_rows_group_f32) instead of three that each wait for the one before."""
        L, inv, user = self.L, 1.0 / (self.L + 1), self._emb_params[:1]
        sources = {user[0]: (self.dE_u, inv)}                                     # AdamW reads inv * dE_u and stores it as the table's .grad
        sm = (self.Il[L - 1], self.dE_i, self.tmpI, inv) if L >= 1 else None      # dI[L] = inv dE_i (mean part), g = softmax_bwd(I_L, dI[L])
        if fuse is not None:
            # members: AdamW reads dE_u, writes the user table, its moments and its .grad; the fusion backward reads dE_u / dE_i, the
            # cat / profile terms and the scatter sources, writes dU_cat / dI_cat / dprof_*; the softmax backward reads I_L and dE_i,
            # writes tmpI. (The rows of dE_* are cleared later, in the item table's launch.)
            if not self.opt.step_params_rows_group(user, sources, fuse, self.d, sm):
                _call("llmrec_fuse_bwd_src_multi_f32", 2, fuse, self.d)
                self.opt.step_params(user, sources=sources)
                if sm is not None:
                    self._softmax_bwd(*sm[:3], alpha=inv)
        elif self.fold:
            self.opt.step_params(user, sources=sources)
        else:
            self._axpy(inv, self.dE_u, user[0].grad, False)
            if self.inline_adamw:                                                 # U^0 only enters the mean: the user table's gradient is final here
                self.opt.step_params(user)
        if side_work is not None:
            side_work()
        if fuse is None and sm is not None:                                       # (with fuse it ran above, in the group or right behind it)
            self._softmax_bwd(*sm[:3], alpha=inv)

    def _chain_bwd_jobs(self):
        """The ID chain's 2 L transposed products [(a, X, Y, kwargs)] in dependency order (items of layer l+1 from the new users; softmax
        on the last layer). Every "+ mean term" and every softmax backward is an epilogue of the SpMM that produces the tensor:
          dI[L] = inv dE_i                      -> g = softmax_bwd(I_L, dI[L])            (one row kernel, no SpMM feeds it: _chain_head)
          dU[l+1] = inv dE_u + A_iu^T g         -> h = softmax_bwd(U_L, dU[l+1]) on the last layer
          dI[l]   = inv dE_i + A_ui^T h         -> (l > 0) feeds the next round as g; (l = 0) IS the item table's gradient"""
        L, inv = self.L, 1.0 / (self.L + 1)
        jobs, g = [], self.tmpI if L >= 1 else self.bufI
        for l in range(L - 1, -1, -1):
            if l == L - 1:
                jobs.append((self.iu.bwd, g, self.tmpU, dict(tag=2, epilogue=ops.spmm_epilogue(ops.EPI_SOFTMAX_BWD, inv, self.dE_u, self.Ul[l]))))
                h = self.tmpU
            else:
                jobs.append((self.iu.bwd, g, self.bufU, dict(tag=2, epilogue=ops.spmm_epilogue(ops.EPI_NONE, inv, self.dE_u))))
                h = self.bufU
            dst = self.m.item_id_embedding.weight.grad if l == 0 else self.bufI
            jobs.append((self.ui.bwd, h, dst, dict(tag=2, epilogue=ops.spmm_epilogue(ops.EPI_NONE, inv, self.dE_i))))
            g = self.bufI
        return jobs

    def _chain_tail(self, probs, batch, ev_fuse=None):
        """Tail of the ID chain's backward, after the last reader of dE_u / dE_i (the chain and the fusion backward - ev_fuse on four
        streams): clear the rows the batch touched, update the item table."""
        users, pos, neg, n_valid = batch
        B = users.numel()
        if self.L == 0:
            self._axpy(1.0 / (self.L + 1), self.dE_i, self.m.item_id_embedding.weight.grad, False)
        # (The wait below is for an EARLY event. A wait for a late one anywhere in this stream's chain - e.g. for the transposed side
        # product, had the row stamps needed a clean-up - makes the graph runtime start the WHOLE chain late:
        # profiles/experiments/r03_wgrad.md, last table.)
        if ev_fuse is not None:
            torch.cuda.current_stream().wait_event(ev_fuse)
        if self.fold and self.L > 0:                                              # clean-up + the item table's AdamW in ONE launch
            jobs = [(users, self.dE_u), (pos, self.dE_i), (neg, self.dE_i), (users, self.sc_U), (pos, self.sc_I), (neg, self.sc_I),
                    (users, self.sc_prof)]
            self.opt.step_params(self._emb_params[1:], zero_rows=(jobs, B, n_valid))
        else:
            _call("llmrec_bpr_multi_zero_rows_f32", self.n_prob, probs, self.d, _p(users), _p(pos), _p(neg), B, _p(n_valid))
            if self.inline_adamw:                                                 # the item table's gradient is final: update it here,
                self.opt.step_params(self._emb_params[1:])                        # beside the weight-gradient GEMM

    def _side_bwd_jobs(self, masked: bool = False):
        """(side chain, profile chain) of the backward as [(a, X, Y, kwargs)]. Side: I_cat = iu(U_cat), U_cat = ui(P_cat) (or the
        pre-propagated projection); profile: prof_u = ui(prof_i), prof_i = iu(P_usr) - user_trans' weight gradient joins the item-side ones.
        masked: the first side product reads the attribute slices of the stamped item rows only (bwd_mask)."""
        side = [(self.iu.bwd, self.dI_cat, self.dU_cat, dict(accumulate=True, mask=(self.flag_i, self.row_stamp, 2) if masked else None))]
        if not self.preprop:
            side.append((self.ui.bwd, self.dU_cat, self.dP_cat, {}))
        prof = [(self.ui.bwd, self.dprof_u, self.dprof_i, dict(accumulate=True, tag=1)), (self.iu.bwd, self.dprof_i, self.dP_usr, dict(tag=1))]
        return side, prof

    def _check_mask_promise(self, masked: bool, done: bool = False):
        """LLMREC_CHECK_ZERO: the masked side product's promise. Before it: the idle item rows (flag_i != the step's stamp) of dI_cat's
        attribute slices are all-zero - or, where the fusion backward no longer writes them, are poisoned with NaN so that a read would
        show; done: behind it, dU_cat is finite."""
        if not (masked and self.check_zero) or torch.cuda.is_current_stream_capturing():
            return
        if done:
            if self.bwd_zero_skip and not bool(torch.isfinite(self.dU_cat).all()):
                raise RuntimeError("FusedStep: the masked side product read an idle row of dI_cat's attribute slices")
            return
        idle = self.flag_i != (int(self.row_stamp.item()) % 255 + 1)
        att = self.dI_cat[:, 2 * self.d:]
        if self.bwd_zero_skip:
            # (debug only: this WRITES the step's buffer. It is safe exactly as long as the masked side product is the only reader of
            # these rows - the premise of zero_skip_from_term; whoever adds another reader must drop the skip, and this poison with it.)
            att[idle] = float("nan")
        elif idle.any() and float(att[idle].abs().max()) != 0.0:
            raise RuntimeError("FusedStep: dI_cat's attribute slices are not all-zero outside the stamped item rows")

    def _backward_one_stream(self, probs, batch, fuse, side_work, masked=False):
        """The backward up to the weight gradients on ONE stream: the k-th product of the ID chain, of the side chain and of the profile
        chain share a launch (_spmm_group); folded, the fusion backward shares the chain head's.
        Where side_work carries a guest descriptor (loss_backward's rider), its loss-value launch rides the FIRST group's launch instead of
        running in the chain head. It reads `saved` (the scores and selection launches), the fusion launch's partial sums and n_valid; it
        writes out, the four totals of each problem in `saved`, scal and the epoch sums - read by the host after the step. Its host reads
        tmpI, dE_u, U_L, dI_cat and dprof_u and writes tmpU, dU_cat and dprof_i: disjoint.
        HOSTED (host_wgrad, _host_wgrad_applies): the groups that have a side or profile partner run here; the chain's first product
        without one, the products behind it and the chain's tail are handed on - returned as (chain[k:], probs, batch) - and
        _weight_gradients runs them in and behind its launch. Read / write sets of that product beside the launch: _weight_gradients."""
        if not self.fold:
            _call("llmrec_fuse_bwd_src_multi_f32", 2, fuse, self.d)
        rides = side_work is not None and side_work.guest is not None
        self._chain_head(None if rides else side_work, fuse if self.fold else None)
        chain, (side, prof) = self._chain_bwd_jobs(), self._side_bwd_jobs(masked)
        self._check_mask_promise(masked)
        n_shared = max(len(side), len(prof))
        hosting = len(chain) > n_shared and self._host_wgrad_applies(chain[n_shared])
        for k, jobs in enumerate(zip_longest(chain[:n_shared] if hosting else chain, side, prof)):
            self._spmm_group(jobs, side_work if k == 0 and rides else None)
        self._check_mask_promise(masked, done=True)
        if self.gemm != "bf16x3" and not self.drop_rate > 0:             # (bf16x3: user_trans' gradient is in the multi-target launch; dropout: _dropout_backward)
            self._wgrad(self.dP_usr, self.m.user_feats, self.m.user_trans, False, ws=self.ws_wgrad_b)
        if hosting:
            return chain[n_shared:], probs, batch
        self._chain_tail(probs, batch)
        return None

    def _wgrad_multi_workspace(self, targets):
        """The multi-target weight gradient's workspace, sized at the first backward (needs the gradient tensors); False: the targets are
        outside that launch's fast path."""
        if self.ws_wgrad_multi is None:
            need = ops.linear_wgrad_multi_workspace(targets, self.wgrad_blocks)
            self.ws_wgrad_multi = torch.empty(max(need, 0), dtype=torch.uint8, device=self.dU_cat.device) if need >= 0 else False
        return self.ws_wgrad_multi

    def _host_wgrad_applies(self, job) -> bool:
        """Whether the chain product `job` (a, X, Y, kwargs of _spmm) is handed to the weight-gradient launch (host_wgrad). The mirror of
        _project_all_hosting's gate: one stream, the folded step with the Linears' AdamW in the reduction launch (the hosting entry
        point is that call's), bf16x3 at d = 64 without dropout (whose launches sit between the schedule and the weight gradients), a
        latency-bound product, the multi-target fast path, and the forward host's size rule - more 128-row projection units than block
        slots: below it the step is too small for the chip either way (and tests/step_schedule_expected.json's steps stay as recorded).
        The library still has the last word (_weight_gradients: a refused pair runs the product by its own launch)."""
        a = job[0]
        if not (self.host_chain and self.host_wgrad and not self._refuse_guests and not self.multi_stream and self.fold and self.inline_adamw
                and self.gemm == "bf16x3" and self.d == 64 and self.drop_rate == 0 and a.nnz < ops.SPMM_LATENCY_NNZ
                and sum(-(-j[0].shape[0] // 128) for j in self.projection_jobs()) > self._block_slots):
            return False
        dY_cat = self.dU_cat if self.preprop else self.dP_cat
        return self._wgrad_multi_workspace(self.wgrad_targets(dY_cat, self.dP_usr)) is not False

    def _backward_streams(self, probs, batch, fuse, side_work, masked=False):
        """The backward up to the weight gradients on four streams (LLMREC_STREAMS=1: the A/B reference of the one-stream schedule):
        fusion backward and side chain on the current stream, profile chain on s1, ID chain on s2."""
        ev_rows = self._mark()                                           # dE_u / dE_i hold the scattered rows: all the ID chain needs
        _call("llmrec_fuse_bwd_src_multi_f32", 2, fuse, self.d)
        ev_fuse = self._mark()                                           # the fusion backward has read dE_u / dE_i
        side, prof = self._side_bwd_jobs(masked)
        self._check_mask_promise(masked)
        # folded step: the critical transposed side product is captured BEFORE the two side branches (main_first) and the logged-scalar
        # launch gets a stream of its own (loss_s3) - each alone lost, both together won: profiles/experiments/r05_step_chain.md
        main_first, loss_s3 = self.fold, self.fold and side_work is not None
        if main_first:
            self._spmm_jobs(side)
            self._fork_from(ev_fuse, self.s1)
        else:
            self._fork(self.s1)
        if loss_s3:
            self._fork_from(ev_rows, self.s3)
            with self._on(self.s3):
                side_work()
            side_work = None
        with self._on(self.s1):
            self._spmm_jobs(prof)
            if self.gemm != "bf16x3" and not self.drop_rate > 0:         # (dropout: behind the mask on dP_usr, _dropout_backward)
                self._wgrad(self.dP_usr, self.m.user_feats, self.m.user_trans, False, ws=self.ws_wgrad_b)
        # the ID chain depends on the BPR rows only, not on the fusion backward: it starts beside it (captured after it, so that the
        # fusion backward stays the graph's same-queue successor of the BPR launch) and has most of its SpMMs behind it when the
        # weight-gradient GEMM takes every CU (one 512-register wave per SIMD leaves no room for a second kernel)
        self._fork_from(ev_rows, self.s2)
        with self._on(self.s2):
            self._chain_head(side_work)
            self._spmm_jobs(self._chain_bwd_jobs())
            self._chain_tail(probs, batch, ev_fuse)
        if not main_first:
            self._spmm_jobs(side)
        self._check_mask_promise(masked, done=True)

    def _weight_gradients(self, ev_reach=None, deferred=None):
        """The four Linears' gradients from dU_cat (pre-propagated; else dP_cat) and dP_usr, and - with inline_adamw - their update.
        ev_reach: four streams - the event behind the row list (step_eager's record).
        deferred: (chain[k:], probs, batch) handed on by _backward_one_stream (host_wgrad) - chain[k] runs INSIDE the weight-gradient
        launch, in the CUs its 224-block layout leaves free; chain[k + 1:] and the chain's tail follow the reduction launch. Read / write sets:
          hosted product  reads bufI (the chain's previous product, earlier in stream order), dE_u (the loss backward; cleared by the
                    tail, which now runs behind this launch), the adjacency and its column scale; writes bufU, read first by chain[k + 1].
          its host  reads dU_cat, dP_usr, the constant operands and the row list; writes its workspace - then the reduction launch the
                    Linears' gradients, parameters and moments. Disjoint (the library checks the extents and refuses an overlap).
        A refused pair: chain[k] by its own launch right ahead of the weight gradient, then the same order. Bit-identical either way."""
        m, S, d = self.m, self.S, self.d
        hosted = deferred[0][0] if deferred is not None else None
        dY_cat = self.dU_cat if self.preprop else self.dP_cat
        targets = self.wgrad_targets(dY_cat, self.dP_usr)
        item_pairs, text_pairs, image_pairs = targets[0][0], targets[2][0], targets[3][0]
        done, updated = False, []
        if self.gemm == "bf16x3":
            # ONE launch for all four Linears: equal slabs over all of them, so the launch is whole rounds of equal blocks and the
            # short gradients pay no ramp-up / ragged last round of their own (round 2, same box: three launches back to back 0.661 ms
            # per step, one launch 0.637 ms). user_trans' gradient is in the same launch since round 3: with the pre-propagated
            # operands nothing separates the two launches in time any more, and side by side each ran at half speed (the chip is
            # power-bound here: profiles/experiments/r03_wgrad.md). The bias gradients (row-weighted when pre-propagated) come out of it too.
            self._join(self.s1)                                          # dP_usr (the profile chain is long done by now)
            if self._wgrad_multi_workspace(targets) is not False:
                self._stamp(3)
                if ev_reach is not None:                                 # (four streams: the row list was built behind the ID chain)
                    torch.cuda.current_stream().wait_event(ev_reach)
                lins = (m.item_trans, m.user_trans, m.text_trans, m.image_trans)              # (wgrad_targets' order)
                if self.inline_adamw:                                  # the four Linears' AdamW rides in the slab-reduction launch
                    update = (self.opt, [(l.weight, l.bias) for l in lins])
                    accepted = False
                    if hosted is not None:                               # (_host_wgrad_applies: inline_adamw and this fast path)
                        probs, keep = self._spmm_problems([hosted])
                        accepted = ops.linear_wgrad_multi(targets, self.ws_wgrad_multi, update=update, block_budget=self.wgrad_blocks,
                                                          host_spmm=(probs[0], self._block_slots // 2))     # (2 block slots per CU)
                        del keep
                        if accepted:
                            self.spmm_edge_units += hosted[0].nnz * (hosted[1].shape[1] / 64.0)
                        else:                                            # refused, nothing launched: the product by its own launch
                            self._spmm_jobs([hosted])
                        hosted = None
                    if not accepted:
                        ops.linear_wgrad_multi(targets, self.ws_wgrad_multi, update=update, block_budget=self.wgrad_blocks)
                    updated = [p_ for l in lins for p_ in (l.weight, l.bias)]
                else:
                    ops.linear_wgrad_multi(targets, self.ws_wgrad_multi, block_budget=self.wgrad_blocks)
                self._stamp(4)
                done = True
            else:                                                        # outside the multi-target fast path: user_trans' on its own
                self._wgrad(self.dP_usr, m.user_feats, m.user_trans, False, ws=self.ws_wgrad_b)
        if not done:
            # exact-fp32 GEMMs, or shapes outside the multi-target fast path (N != 64, K % 128 != 0): one launch per Linear; their
            # kernels sum dY unweighted, so a pre-propagated step takes its bias gradients from llmrec_weighted_colsum_f32
            strip = lambda pairs: [p_[:2] for p_ in pairs]
            bias = (lambda lin: None) if self.preprop else (lambda lin: lin.bias.grad)
            if self.preprop:
                outs = [m.image_trans.bias.grad, m.text_trans.bias.grad] + [m.item_trans.bias.grad] * len(self.keys)
                gp = (_c.c_void_p * S)(*[t.data_ptr() for t in outs])
                _call("llmrec_weighted_colsum_f32", self.U, S, d, _p(dY_cat), _ld(dY_cat), _p(self.a_rowsum), gp, 0, _p(self.ws_colsum), self.ws_colsum.numel())
            ops.linear_wgrad_grouped(strip(item_pairs), m.item_trans.weight.grad, bias(m.item_trans), False, self.ws_wgrad, precision=self.gemm)
            ops.linear_wgrad_grouped(strip(text_pairs), m.text_trans.weight.grad, bias(m.text_trans), False, self.ws_wgrad_c, precision=self.gemm)
            ops.linear_wgrad_grouped(strip(image_pairs), m.image_trans.weight.grad, bias(m.image_trans), False, self.ws_wgrad_d, precision=self.gemm)
        if deferred is not None:                                         # the rest of the ID chain, then its tail (one stream)
            rest, probs_bpr, batch = deferred
            for job in rest if hosted is not None else rest[1:]:         # (hosted still set: no launch above took the first product)
                self._spmm_group([job])
            self._chain_tail(probs_bpr, batch)
        self._join(self.s1)                                              # user_trans' gradient
        if self.inline_adamw:                                            # whatever the reduction launch did not update (all four Linears on
            self.opt.step_params([p_ for p_ in self._lin_params if all(p_ is not q for q in updated)])   # the per-target fallback paths)

    def build_scatter_plan(self, users, pos, neg, n_valid=None):
        """llmrec_bpr_scatter_plan of this batch into the step's plan buffer (one launch; step_eager does it behind the sampler - callers
        that drive forward() / loss_backward() themselves call it once per batch, any time before the loss backward)."""
        self._check_batch(users.numel())
        if self.wide:
            _call("llmrec_bpr_scatter_plan_wide", _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid), _p(self.bpr_plan),
                  _p(self.ws_plan_wide), self.ws_plan_wide.numel())
        else:
            _call("llmrec_bpr_scatter_plan", _p(users), _p(pos), _p(neg), users.numel(), _p(n_valid), _p(self.bpr_plan))

    def reset_scatter_targets(self):
        """Dense clear of the scatter targets, which the step keeps all-zero between steps by clearing the rows it touched (set-up,
        (re)capture, and after a step that raised between the loss backward's scatter and its row-wise clean-up)."""
        for t in (self.dE_u, self.dE_i, self.sc_U, self.sc_I, self.sc_prof):
            t.zero_()

    def _plan_reach_rider(self, step: _TrainStep, batch) -> _Rider:
        """The scatter plan of the loss backward and the weight gradient's row list. Where the step's riders apply, a ladder - a refused
        rung launches nothing and the next one runs:
          1. plan + reach marks as the guest of an SpMM launch (_forward_one_stream names the host);
          2. the same as ONE launch of their own: the marking half of llmrec_batch_reach_rows behind the plan's blocks. After 1 or 2 the
             flags are marked and the compaction rides in front of the fusion launch's blocks (_forward): two launches fewer;
          3. the separate launches: the plan, then llmrec_batch_reach_rows' two. (All there is where the riders do not apply.)
        On four streams they run on the ID chain's stream BEHIND its SpMMs (the plan is needed ~200 us later, the list at the step's far
        end): the fusion waits for the chain's event, the loss launches for ev_plan, the weight gradient for ev_reach. Round 6, one box,
        300 steps twice: 0.4539 / 0.4539 ms per step ahead of the SpMMs, 0.4470 / 0.4481 behind them (profiles/experiments/r06_step_chain.md)."""
        users, pos, neg, n_valid = batch
        by_item = self.iu.fwd
        plan_reach = (users, pos, neg, users.numel(), n_valid, self.bpr_plan, by_item.n_cols, by_item.n_rows, by_item.rowptr, by_item.colidx,
                      self.act_flags) if step.ride else None   # the arguments of rungs 1 and 2

        def marked():
            step.reach_pending = batch

        def alone():
            if step.ride and _lib.call_unless_unsupported("llmrec_bpr_scatter_plan_reach_mark", *_raw(plan_reach), ops._stream()):   # rung 2
                return marked()
            self.build_scatter_plan(users, pos, neg, n_valid)                                                        # rung 3
            step.ev_plan = self._mark()
            if self.wgrad_rows:
                ops.batch_reach_rows(users, pos, neg, n_valid, by_item, self.act_flags, self.act_rows, self.act_n)
                step.ev_reach = self._mark()
        return _Rider(alone, (lambda: ops.guest_plan_reach(*plan_reach)) if step.ride else None, marked)             # rung 1

    def step_eager(self, users, pos, neg, n_valid=None, sampler=None):
        """sampler: optional callable - a plain one or sampler_of()'s rider - that fills (users, pos, neg, n_valid) on the current stream
        first (inside the same graph when captured; running it on a side stream beside the forward measured no faster)."""
        if sampler is not None and not isinstance(sampler, _Rider):
            sampler = _Rider(sampler)
        # riders (the sampler, the plan + reach marks and the loss values in SpMM launches: three launches fewer) apply on one stream with a
        # device sampler in the step, a reach list to build and the folded loss-value launch - and not on the wide route: the plan and
        # the loss values have no guest form above LLMREC_BPR_MAX_B (decided here, once, not by a refused call per step), so the
        # sampler, the plan and llmrec_batch_reach_rows' two launches (rung 3 of _plan_reach_rider's ladder) run on their own
        step = _TrainStep(ride=bool(self.wgrad_rows and sampler is not None and self.fold and not self.multi_stream and not self.wide))
        if step.ride:
            self._check_batch(users.numel())
        batch_lists = self._plan_reach_rider(step, (users, pos, neg, n_valid))
        self.spmm_edge_units = 0.0
        calls0 = _lib.n_calls
        try:
            self._stamp(0)
            if self.multi_stream or step.ride:                   # the sampler rides beside the projection (_forward_streams) / in an SpMM launch
                self._train_forward(sampler, batch_lists, step)
            else:
                if sampler is not None:
                    sampler()
                batch_lists()
                self._train_forward(step=step)
            self.loss_backward(users, pos, neg, n_valid, step)
            if not self.inline_adamw:
                self.opt.step(advanced=True)
            self._stamp(5)
            self.entry_point_calls_per_step = _lib.n_calls - calls0 - (2 if self.stamps is not None else 0) * 3
            if self.wgrad_rows and self.act_expected is None and not torch.cuda.is_current_stream_capturing():
                self._size_wgrad_for_rows()                      # first step: one read-back of the list length
        except Exception:
            if not torch.cuda.is_current_stream_capturing():   # the all-zero invariant of the scatter targets may be broken: restore it
                with contextlib.suppress(Exception):
                    if step.reach_pending is not None:         # marked, not yet compacted: the flags' all-zero invariant too
                        self.act_flags.zero_()
                    self.reset_scatter_targets()
            raise
        return self.scal[1], self.scal[2], self.scal[3]

    def _size_wgrad_for_rows(self, expected: Optional[int] = None):
        """Lay the weight-gradient launch out for the list length the last step saw (+ 10 %): the kernel cuts a listed problem's slabs
        into equal pieces of the ACTUAL length every step, this only decides how many blocks each target gets. One host read-back;
        the workspace is re-sized here (outside any capture). expected: the layout itself (finish_load: a saved run's), no read-back."""
        if expected is not None:
            self.act_expected = expected
        else:
            n = int(self.act_n.item())
            self.act_expected = max(64, min(self.U, int(n * 1.10) + 32))
        need = ops.linear_wgrad_multi_workspace(self.wgrad_targets(self.dU_cat if self.preprop else self.dP_cat, self.dP_usr), self.wgrad_blocks)
        self.ws_wgrad_multi = torch.empty(max(need, 0), dtype=torch.uint8, device=self.dP_usr.device) if need >= 0 else False

    def check_wgrad_geometry(self, factor: float = 1.5) -> bool:
        """the row-listed weight gradient's launch geometry is laid out for the list length of the FIRST step (+ 10 %) and frozen
        into the captured graph; the kernel re-cuts its slabs for the actual length, so results never depend on it, but a workload whose
        batches later reach many more (or far fewer) rows would run in a badly balanced launch with no signal. Call this where the host
        synchronises anyway (main.py: once per epoch, behind the epoch sums): ONE read-back of the last step's list length; when it left
        [expected / factor, expected * factor] the launch is laid out again and the step graph RE-captured (no warm-up step: nothing is
        trained here). Returns whether it re-captured."""
        if not self.wgrad_rows or self.act_expected is None or torch.cuda.is_current_stream_capturing():
            return False
        want = max(64, min(self.U, int(int(self.act_n.item()) * 1.10) + 32))
        if self.act_expected / factor <= want <= self.act_expected * factor:
            return False
        self._size_wgrad_for_rows()
        if self.graph_exec is not None and self._capture_args is not None:
            self.capture(warm=False, **self._capture_args)
        return True

    def flush(self):
        """Nothing is deferred in the single-graph step (DataParallelStep defers its AdamW)."""

    # -- state (checkpoints) ----------------------------------------------------------------------
    def state_tensors(self):
        """[(name, tensor)] of EVERYTHING this step carries in device memory from one step boundary to the next; a checkpoint is these
        bytes (llmrec_amd/checkpoint.py knows no more). A new piece of device state = one more line here.
          param/*, adamw/*   every parameter of the model in named_parameters() order, AdamW's counter and both moments of each
                    (engine.model_state_tensors);
          row_stamp, flag_u, flag_i   the stamp counter and the rows' stamps. All three, so that a loaded state EQUALS the saved one: stale
                    stamps that meet a rewound counter would make the fusion backward skip, or read, the wrong rows;
          epoch_sums   the running sums of the logged scalars;
          drop_step, drop_ticket   (drop_rate > 0) the dropout masks' counter and its count-off;
          mask_step, mask_ticket, user_sums/*, item_sums/*   (mask_rate > 0) the masking round's counter, its count-off and the running
                    fp64 column sums. The masked feature matrices themselves are NOT here: prepare_load() replays the rounds;
          decoder/*   (the restoration term) the decoder's parameters: never stepped, but a resumed run must not depend on the order of
                    initialisation.
        NOT state, by design:
          dE_u, dE_i, sc_U, sc_I, sc_prof, act_flags   the scatter targets and the reach flags are all-zero at every step boundary (the
                    invariant LLMREC_CHECK_ZERO asserts), in the saved run and in the loading one;
          .grad, saved, bpr_plan, out, scal, the forward / backward buffers, the node lists, the workspaces and partial sums   are
                    rewritten by every step before anything reads them;
          AX, a_rowsum, the targets, the adjacency   the pre-propagated operands are constants of the run, formed at set-up.
        The sampler's counter belongs to the batcher (engine.DeviceBatcher.state_tensors), which the caller lists beside this step."""
        from .engine import model_state_tensors
        out = model_state_tensors(self.m, self.opt)
        out += [("step/row_stamp", self.row_stamp), ("step/flag_u", self.flag_u), ("step/flag_i", self.flag_i), ("step/epoch_sums", self.epoch_sums)]
        if self.drop_rate > 0:
            out += [("step/drop_step", self.drop_step), ("step/drop_ticket", self.drop_ticket)]
        if self.mask_rate > 0:
            out += [("step/mask_step", self.mask_step), ("step/mask_ticket", self.mask_ticket)]
            out += [("step/user_sums/%d" % k, t) for k, t in enumerate(self.user_sums)]
            out += [("step/item_sums/%d" % k, t) for k, t in enumerate(self.item_sums)]
        if self.restore:
            out += [("decoder/" + name, p.data) for name, p in self.decoder.named_parameters()]
        return out

    def host_state(self):
        """What the step keeps on the HOST across steps and a resumed run must share: the list length the weight-gradient launch is
        laid out for (frozen at the first step, re-laid by check_wgrad_geometry) - it fixes that launch's summation partition."""
        return {"act_expected": self.act_expected if self.wgrad_rows else None}

    replayed_mask_rounds = None     # (rounds, seconds) of the last prepare_load()'s replay

    def prepare_load(self, saved):
        """Ahead of a load: saved(name) is the saved tensor of that name (a device tensor; None: not in the checkpoint). Only a masking
        step has work here. Its feature matrices are not in the checkpoint (0.5 GB at the Netflix shape): the lists are a function of
        (seed, round, side), the values of the running fp64 sums, and the kernels are deterministic, so a FRESH step (mask_step == 0,
        features as read, sums from refresh_feature_sums()) replays _mask_round() saved-mask_step times and must then hold the saved
        mask_step and sums bit for bit. A step that has already masked raises: there is no rollback in this mode."""
        if not self.mask_rate > 0:
            return
        import time
        want = saved("step/mask_step")
        if want is None:
            raise RuntimeError("FusedStep.prepare_load: the checkpoint holds no masking state")
        if int(self.mask_step.view(torch.int64).item()) != 0:
            raise RuntimeError("FusedStep.prepare_load: this step has already masked its features (mask_step != 0); a masking checkpoint "
                               "loads into a fresh step only")
        rounds = int(want.view(torch.int64).item())
        t0 = time.perf_counter()
        for _ in range(rounds):
            self._mask_round()
        torch.cuda.current_stream().synchronize()
        self.replayed_mask_rounds = (rounds, time.perf_counter() - t0)
        mine = dict(self.state_tensors())
        bad = [name for name in mine if name.startswith(("step/mask_step", "step/user_sums/", "step/item_sums/"))
               and not torch.equal(mine[name].view(torch.int64), saved(name).view(torch.int64))]
        if bad:
            raise RuntimeError("FusedStep.prepare_load: %d replayed masking rounds do not reproduce the saved %s (other features, "
                               "another seed or mask_rate?)" % (rounds, bad))

    def finish_load(self, host):
        """Behind a load: the host half (host_state()). A different launch layout is applied now - and a captured step re-captured
        without a warm-up step, as check_wgrad_geometry does."""
        expected = (host or {}).get("act_expected")
        if self.wgrad_rows and expected is not None and expected != self.act_expected:
            self._size_wgrad_for_rows(int(expected))
            if self.graph_exec is not None and self._capture_args is not None:
                self.capture(warm=False, **self._capture_args)

    @torch.no_grad()
    def load_state(self, saved, host=None):
        """Make this step's state the saved one: saved(name) -> tensor (any device). Writes INTO the existing tensors and never rebinds
        one - a captured graph holds their addresses - so loading into a live, captured step is legal: a rollback to the saved step.
        (llmrec_amd.checkpoint.Checkpointer moves the same bytes in one launch between prepare_load() and finish_load().)"""
        self.prepare_load(saved)
        for name, t in self.state_tensors():
            src = saved(name)
            if src is None or src.shape != t.shape or src.dtype != t.dtype:
                raise RuntimeError("FusedStep.load_state: %s is missing from the saved state or has another shape / dtype" % name)
            t.copy_(src)
        self.finish_load(host)

    # -- evaluation -------------------------------------------------------------------------------
    def eval_topk(self, query_users: torch.Tensor, train: Optional[ops.Csr], K: int, use_graph: bool = False, held=None, Ks=None,
                  auc: bool = False):
        """Reference Trainer.test up to the ranked lists (main.py:297-303, batch_test.py:83-109): no-grad forward +
        scoring + masked top-K for the listed users -> (idx int32 [n, K], scores). With use_graph the whole
        evaluation (~40 launches) is one HIP graph per (query set, K), replayed at every epoch end.
        held = (rowptr, colidx) of the held-out CSR + Ks (use_graph only): the evaluation also ends with llmrec_topk_eval_sums - hits, per-user
        precision / recall / ndcg / hit-ratio and their sums over the users, two launches at the graph's tail writing the 4 x len(Ks)
        doubles into PINNED host memory (self.eval_sums(...) after a stream synchronisation; batch_test.py:160-165 divided by the
        number of users) - nothing per user leaves the device and no copy follows the replay.
        auc=True (with held, use_graph only; --test_flag full): the graph also ends with llmrec_score_auc_f32 - the full-rank AUC of every
        listed user against the same held-out rows, summed by a fixed tree into one pinned double (self.eval_auc_sum())."""
        if auc and (not use_graph or held is None):
            raise RuntimeError("FusedStep.eval_topk: auc=True needs use_graph=True and the held-out rows")
        if not use_graph:
            self.forward()
            return ops.score_topk(self.E_u, self.E_i, query_users, train, K)
        Ks = tuple(int(k) for k in Ks) if held is not None else None
        key = (query_users.data_ptr(), query_users.numel(), K, id(train), None if held is None else (held[0].data_ptr(), Ks), bool(auc))
        ev = self._eval_graphs.get(key)
        if ev is None:
            q = query_users.to(torch.int64).contiguous()
            n = q.numel()
            idx = torch.empty(n, K, dtype=torch.int32, device=q.device)
            sc = torch.empty(n, K, dtype=torch.float32, device=q.device)
            wide = K > _lib.CONST["LLMREC_TOPK_MAX"]               # rounds of the sweep inside the graph (llmrec_score_topk_wide_f32)
            nnz = ops._wide_train_nnz(train, q) if wide else 0
            ws = ops.topk_workspace(n, self.I, q.device, self.d, K, nnz)
            sums = sums_ws = None
            if held is not None:
                sums = torch.zeros(4, len(Ks), dtype=torch.float64).pin_memory()
                sums_ws = torch.empty(_lib.query("llmrec_topk_eval_sums_workspace_bytes", n, len(Ks)), dtype=torch.uint8, device=q.device)
            auc_sum = auc_ws = None
            if auc:
                auc_sum = torch.zeros(1, dtype=torch.float64).pin_memory()
                auc_ws = ops.auc_workspace(n, self.I, q.device, self.d)

            # what the three scoring launches share: the queries, both tables, the train rows to mask
            scoring = (n, _p(q), _p(self.E_u), _ld(self.E_u), _p(self.E_i), _ld(self.E_i), self.I, self.d,
                       _p(train.rowptr) if train is not None else None, _p(train.colidx) if train is not None else None)

            def run(mask=True):
                # the evaluation's graph has TWO branches (the ID chain beside the projection; the profile chain stays on the main stream):
                # 0.572 ms per replay back to back / 0.599 one at a time, against 0.73 - 0.76 / 0.595 with the training forward's three
                # side branches - successive launches of a many-branch graph pay for their cross-queue joins (tools/eval_probe.py, round 6)
                self.forward(profile_on_main=True, mask=mask)
                if wide:
                    _call("llmrec_score_topk_wide_f32", *scoring, K, _p(idx), _p(sc), _p(ws), ws.numel(), ops.topk_wide_mode(None, self.I, self.d, K), nnz)
                else:
                    _call("llmrec_score_topk_mode_f32", *scoring, K, _p(idx), _p(sc), _p(ws), ws.numel() if ws is not None else 0,
                          ops.topk_mode(None, self.I, self.d, K))
                if held is not None:
                    ops.topk_eval_sums(idx, q, held[0], held[1], Ks, out=sums, ws=sums_ws)
                if auc:
                    _call("llmrec_score_auc_f32", *scoring, _p(held[0]), _p(held[1]), None, None, _c.c_void_p(auc_sum.data_ptr()), _p(auc_ws),
                          auc_ws.numel())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run(mask=False)                                # (one eval_topk call is ONE masking round: the replay below)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _capture_without_gc(g, self.multi_stream):
                run()
            ev = self._eval_graphs[key] = _EvalGraph(g, idx, sc, q, train, ws, sums, sums_ws, held, auc_sum, auc_ws)
        ev.graph.replay()
        self._last_eval = ev
        return ev.idx, ev.scores

    def eval_sums(self):
        """The pinned [4, len(Ks)] sums of the LAST eval_topk(..., held=...) replay; synchronises the current stream first."""
        ev = self._last_eval
        if ev is None or ev.sums is None:
            raise RuntimeError("FusedStep.eval_sums: the last evaluation was not captured with a held-out set")
        torch.cuda.current_stream().synchronize()
        return ev.sums

    def eval_auc_sum(self):
        """The pinned float64 [1] sum of the per-user AUCs of the LAST eval_topk(..., auc=True) replay; synchronises the current stream first."""
        ev = self._last_eval
        if ev is None or ev.auc_sum is None:
            raise RuntimeError("FusedStep.eval_auc_sum: the last evaluation was not captured with auc=True")
        torch.cuda.current_stream().synchronize()
        return ev.auc_sum

    def drop_eval_graph(self, query_users: torch.Tensor):
        """Release every captured evaluation (graph, result lists, top-K workspace) of this query tensor."""
        for key in [k for k in self._eval_graphs if k[0] == query_users.data_ptr() and k[1] == query_users.numel()]:
            del self._eval_graphs[key]

    # -- HIP graph --------------------------------------------------------------------------------
    def _make_static(self):
        dev = self.E_u.device
        # ONE int64 block [users | pos | neg | n_valid] so that a host-sampled batch can arrive in a single asynchronous H2D copy
        # (step_packed): b_max ids each, then one slot whose LOW 32 bits are the int32 n_valid the kernels read (little-endian)
        b = self.b_max
        blk = torch.zeros(3 * b + 1, dtype=torch.int64, device=dev)
        self.static_block = blk
        self.static = {"users": blk[0:b], "pos": blk[b:2 * b], "neg": blk[2 * b:3 * b], "n_valid": blk[3 * b:3 * b + 1].view(torch.int32)[:1]}
        return self.static

    @staticmethod
    def sampler_of(batcher, st):
        """step_eager's `sampler` for a DeviceBatcher filling the buffers st (users / pos / neg / n_valid): the rider whose run() is the
        batcher's own launch and whose guest (where the batcher offers one) is the same call as the guest descriptor of an SpMM launch."""
        if batcher is None:
            return None
        args = (st["users"], st["pos"], st["neg"], st["n_valid"])
        return _Rider(lambda: batcher.fill(*args), (lambda: batcher.guest(*args)) if hasattr(batcher, "guest") else None)

    def capture(self, warm_users=None, warm_pos=None, warm_neg=None, warm_n_valid=None, batcher=None, unroll: int = 1, warm: bool = True):
        """Capture one step (fixed batch capacity b_max, actual size on the device in n_valid).
        With `batcher` (engine.DeviceBatcher, capacity == b_max) the sampler is part of the graph: a
        training step is then ``step()`` with no arguments = one graph replay, nothing else on the stream.
        warm=False (a RE-capture, check_wgrad_geometry): no warm-up step is run - it would be an extra optimiser step - and the static
        batch buffers are kept."""
        st = self._make_static() if (warm or self.static is None) else self.static
        self.batcher = batcher
        self._capture_args = {"batcher": batcher, "unroll": unroll}
        if batcher is not None and batcher.capacity != self.b_max:
            raise RuntimeError("FusedStep.capture: batcher capacity %d != b_max %d" % (batcher.capacity, self.b_max))
        if batcher is None and warm:
            self._load(warm_users, warm_pos, warm_neg, warm_n_valid)

        def one_step():
            self.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=self.sampler_of(batcher, st))
        self.reset_scatter_targets()                           # (re)capture starts from the invariant, whatever ran before
        if warm:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):                         # warm-up on a side stream (allocations, plan caches)
                one_step()
            torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _capture_without_gc(g, self.multi_stream):
            one_step()
        self.graph_exec = g
        # with the sampler inside the graph nothing host-side separates two steps: run_steps() replays a graph of `unroll` steps (the
        # device front end takes ~10 us to start the next graph behind the previous one's last kernel - paid once per `unroll` steps)
        self.graph_multi, self.graph_unroll = None, 0
        if batcher is not None and unroll > 1:
            g2 = torch.cuda.CUDAGraph()
            with _capture_without_gc(g2, self.multi_stream):
                for _ in range(unroll):
                    one_step()
            self.graph_multi, self.graph_unroll = g2, unroll

    def run_steps(self, n: int):
        """n training steps of the captured graph(s) (in-graph sampler only): as many replays of the `unroll`-step graph as fit, single
        steps for the remainder. Returns the logged scalars of the last step."""
        if self.graph_exec is None or self.batcher is None:
            raise RuntimeError("FusedStep.run_steps: capture(batcher=...) first")
        k = self.graph_unroll if self.graph_multi is not None else 0
        while k and n >= k:
            self.graph_multi.replay()
            n -= k
        for _ in range(n):
            self.graph_exec.replay()
        return self.scal[1], self.scal[2], self.scal[3]

    def _load(self, users, pos, neg, n_valid):
        st, B = self.static, users.numel()
        if B > self.b_max:
            raise RuntimeError("FusedStep: batch of %d exceeds b_max %d" % (B, self.b_max))
        st["users"][:B].copy_(users); st["pos"][:B].copy_(pos); st["neg"][:B].copy_(neg)
        if n_valid is None:
            st["n_valid"].fill_(B)
        else:
            st["n_valid"].copy_(n_valid)

    def packed_layout(self):
        """(slots, b_max): a batch for step_packed is an int64 block of `slots` = 3 b_max + 1 entries - users at [0, B'), positives at
        [b_max, b_max + B'), negatives at [2 b_max, 2 b_max + B'), the number of triples B' in the last slot."""
        return 3 * self.b_max + 1, self.b_max

    def step_packed(self, host_block: torch.Tensor):
        """One training step from a host-sampled batch already laid out as packed_layout() says (pinned memory): ONE asynchronous H2D copy
        into the captured step's static buffers, then the graph replay - no per-tensor device copies (step(users, pos, neg) issues four)."""
        if self.graph_exec is None or self.batcher is not None:
            raise RuntimeError("FusedStep.step_packed: capture(users, pos, neg) first (a graph without an in-graph sampler)")
        self.static_block.copy_(host_block, non_blocking=True)
        self.graph_exec.replay()
        return self.scal[1], self.scal[2], self.scal[3]

    def step(self, users=None, pos=None, neg=None, n_valid=None):
        """One training step; replays the captured graph when there is one (no arguments when the
        sampler was captured with it)."""
        if self.graph_exec is None:
            return self.step_eager(users, pos, neg, n_valid)
        if users is not None:
            if self.batcher is not None:
                raise RuntimeError("FusedStep.step: this graph samples its own batch; call step() without arguments")
            self._load(users, pos, neg, n_valid)
        elif self.batcher is None:
            raise RuntimeError("FusedStep.step: a batch is needed (the graph was captured without a sampler)")
        self.graph_exec.replay()
        return self.scal[1], self.scal[2], self.scal[3]
