"""The schedule switches of the fused training step (llmrec_amd/fused.py), decided ONCE, here: resolve() is a pure function of the
environment (any mapping), the shapes, the class defaults of the step (FusedStep.WGRAD_ROWS / INLINE_ADAMW / FOLD: DataParallelStep turns
all three off) and three properties of the backward's side product. It touches no device and imports neither torch nor the library, so
the CPU suite holds it to hand-written records (tests/test_step_options_cpu.py). FusedStep.__init__ copies the record onto its
same-named attributes; the rationale of every switch stands beside the line that decides it.

A new switch of the step: a name in ENV_SWITCHES, a field of StepOptions, its line in resolve()."""
from __future__ import annotations

import os
from typing import Mapping, NamedTuple, Optional

# every environment variable resolve() reads
ENV_SWITCHES = ("LLMREC_STREAMS", "LLMREC_GEMM", "LLMREC_PREPROPAGATE", "LLMREC_WGRAD_ROWS", "LLMREC_FOLD", "LLMREC_BWD_MASK",
                "LLMREC_HOST_CHAIN", "LLMREC_CHECK_ZERO")
# the variables main.py reads itself to choose the path that builds a step (names only: tests clear both tuples before they build one)
TRAINER_SWITCHES = ("LLMREC_FUSED", "LLMREC_GRAPH", "LLMREC_DEVICE_SAMPLER", "LLMREC_FUSED_DROPOUT", "LLMREC_EVAL_GRAPH")


def route(fused: Optional[str], fused_dropout: Optional[str], *, mask, mask_rate: float, drop_rate: float, b_max: int, cap: int,
          wide_cap: int, n_users: int = 0, n_items: int = 0) -> str:
    """Which path trains a step: "fused" (FusedStep, the capped loss segment), "fused_wide" (FusedStep above its WIDE_FROM: the wide loss
    segment) or "modular" (the per-op autograd path). Pure: main.py reads the environment and the device itself.
    fused / fused_dropout: the values of LLMREC_FUSED / LLMREC_FUSED_DROPOUT (None: unset); mask / mask_rate / drop_rate: the trainer's
    flags; b_max: the step's batch capacity (batch_size + its augmented share); cap / wide_cap: LLMREC_BPR_MAX_B / LLMREC_BPR_WIDE_MAX_B.
    LLMREC_FUSED: unset or "1" - the fused step up to `cap`, the modular path above it; "wide" (opt-in) - the same step up to `cap` and
    the wide loss segment up to `wide_cap`; "mask" (opt-in) - as "1", and --mask / --mask_rate > 0 stay in the fused step (below);
    anything else - the modular path. The reference masks user features whenever mask_rate > 0, with or without --mask, and the
    default fused step reads the unmasked features; --drop_rate > 0 stays fused under LLMREC_FUSED_DROPOUT=1 only.
    LLMREC_FUSED=mask with --mask or --mask_rate != 0 (FusedStep(mask_rate=, mask_items=, ...): the library's node lists, not
    torch.randperm's) still goes to the modular path for: a batch above `cap` (no wide segment with masking); --drop_rate > 0
    (no fused dropout with masking, whatever LLMREC_FUSED_DROPOUT says); a mask_rate outside (0, 1]; --mask with an empty user or item
    list, int(mask_rate * n_users) == 0 or int(mask_rate * n_items) == 0 - the reference's loss is then NaN (the mean over no rows),
    which stays the per-op path's to produce. n_users / n_items (keywords; 0 = unknown, so --mask is refused): the graph's sizes."""
    fused = "1" if fused is None else fused
    if fused == "mask":
        if not mask and mask_rate == 0:
            fused = "1"                                    # nothing to mask: the default step
        else:
            if b_max > cap or drop_rate != 0 or not 0.0 < mask_rate <= 1.0:
                return "modular"
            if mask and (int(mask_rate * n_users) == 0 or int(mask_rate * n_items) == 0):
                return "modular"
            return "fused"
    if fused not in ("1", "wide") or mask or mask_rate != 0 or not (drop_rate == 0 or fused_dropout == "1"):
        return "modular"
    if b_max <= cap:
        return "fused"
    return "fused_wide" if fused == "wide" and b_max <= wide_cap else "modular"


class StepOptions(NamedTuple):
    """The resolved switches of one step: FusedStep's attributes of the same names."""
    drop_rate: float
    check_zero: bool
    multi_stream: bool
    gemm: str
    preprop: bool
    wgrad_rows: bool
    inline_adamw: bool
    fold: bool
    bwd_mask: bool
    bwd_zero_skip: bool
    host_chain: bool
    host_wgrad: bool = True


def resolve(env: Optional[Mapping[str, str]], *, n_users: int, n_items: int, d: int, n_attr: int, drop_rate: float, wgrad_rows_default: bool,
            inline_adamw_default: bool, fold_default: bool, bwd_nnz: int, bwd_valued: bool, bwd_col_scaled: bool,
            latency_nnz: int, mask_items: bool = False, restore: bool = False) -> StepOptions:
    """env: the environment (None: the process's own); n_users / n_items / d: the shapes; n_attr: the number of attribute streams; the
    three class defaults; bwd_*: the backward's side product (iu.bwd) - its nnz, whether it keeps values, whether it has a column
    scale; latency_nnz: ops.SPMM_LATENCY_NNZ, the nnz below which a product is latency-bound; mask_items: the step masks the attribute
    features every forward (--mask); restore: it also adds the restoration term's gradient (--mask with att_re_rate != 0) - both move
    existing fields only (MASKING below)."""
    if not 0.0 <= float(drop_rate) < 1.0:                  # (false for a NaN)
        raise ValueError("FusedStep: drop_rate %r outside [0, 1)" % (drop_rate,))
    drop_rate = float(drop_rate)
    env = os.environ if env is None else env
    U, I = n_users, n_items
    # LLMREC_CHECK_ZERO=1 (debug; synchronises, so not under capture): assert before every scatter that the scatter targets of the loss
    # backward are all-zero between steps (FusedStep.__init__, "backward buffers")
    check_zero = env.get("LLMREC_CHECK_ZERO", "0") == "1"
    # Independent chains (7-stream side features / LLM profile / ID embeddings / the logged scalars) can run on four HIP streams in forward
    # and in backward (LLMREC_STREAMS=1), so that the latency-bound Netflix-scale SpMMs overlap the GEMMs in eager launches. The default
    # is ONE stream: a captured step must be a single-branch graph (llmrec_amd/__init__.py).
    multi_stream = env.get("LLMREC_STREAMS", "0") == "1"
    # projection / weight-gradient arithmetic: "bf16x3" (default) = exact 3-term bf16 split of both operands, six bf16
    # MFMAs, fp32-roundoff-class error (2e-6 measured); "f32" = the exact fp32 MFMA fma chain
    gemm = env.get("LLMREC_GEMM", "bf16x3")
    # PRE-PROPAGATED item-side operands (LLMREC_PREPROPAGATE=0 restores the reference's order of operations). The features F_k
    # and the adjacency are constants of a run, and projection followed by propagation is one product:
    #     A_ui (F_k W^T + 1 b^T) = (A_ui F_k) W^T + (A_ui 1) b^T            (Models.py:145-157: image / text / the 5 attributes)
    # so A_ui F_k [U, K] is formed ONCE at set-up, the step projects IT (llmrec_linear_problem_t.bias_scale = the row sums of A_ui) straight
    # into U_cat, and the backward takes dW = dU_cat^T (A_ui F_k), db = sum_u (A_ui 1)[u] dU_cat[u]. Per step this removes the two
    # [.., 7 d] SpMMs through A_ui (forward and transposed) from the critical path and shrinks both GEMMs from I = 17 366 to
    # U = 13 187 rows; every parameter-dependent product is still computed every step, only the order of the (associative)
    # products changes: results agree with the other order to fp32 rounding (tests/test_gpu_step.py, the bench's parity gate).
    # SHAPE-AWARE (VERDICT r03 next #4c): pre-propagation moves both GEMMs from I rows to U rows and takes the two [., 7 d] SpMMs off the
    # critical path. It wins when the user side is the smaller one (Netflix shape, U / I = 0.76: 0.46 vs 0.62 ms per step) and loses
    # when it is the larger one (MovieLens shape, U / I = 1.21: 0.49 vs 0.48 ms, measured with the row-listed weight gradient on):
    # default = pre-propagate iff U <= I. LLMREC_PREPROPAGATE=1 / 0 forces either order.
    want = env.get("LLMREC_PREPROPAGATE", "auto")
    preprop = d <= 64 and (want == "1" or (want not in ("0", "1") and U <= I))
    # DROPOUT (drop_rate > 0; opt-in: main.py builds such a step under LLMREC_FUSED_DROPOUT=1 only). nn.Dropout acts on the projections
    # F_k W^T + b BEFORE they are propagated, and A (drop(F W^T)) is not (A F) W^T: the step runs in the reference's order of operations
    # (P_cat / dP_cat; the row-listed weight gradient, which needs the pre-propagated operands, is off with it). The masks are
    # llmrec_dropout_rows_f32's - a function of (drop_seed, drop_step, tensor tag, row, column), not torch's stream: two launches on
    # P_cat / P_usr behind the projection launch of a TRAINING forward, the same two masks on dP_cat / dP_usr ahead of the weight
    # gradients. drop_step is device memory: the backward's second launch advances it (drop_ticket: its blocks' count-off), so a
    # replayed graph draws a new mask every step with no host action. An evaluation's forward launches none and never touches the counter.
    if drop_rate > 0:
        if want == "1":
            raise RuntimeError("FusedStep: drop_rate > 0 needs the reference's order of operations; LLMREC_PREPROPAGATE=1 cannot be honoured")
        preprop = False
    # MASKING (mask_items; opt-in: main.py builds such a step under LLMREC_FUSED=mask only). The reference overwrites mask_rate of the rows
    # of the five attribute feature matrices with the column mean at EVERY forward (Models.py:131-138), so A_ui F_k is no constant of the
    # run: the step runs in the reference's order of operations, as with dropout. User-feature masking alone (mask_rate > 0 without
    # --mask) changes user_feats only, which no pre-propagated operand holds: that step keeps the default schedule.
    if mask_items:
        if want == "1":
            raise RuntimeError("FusedStep: mask_items needs the reference's order of operations; LLMREC_PREPROPAGATE=1 cannot be honoured")
        preprop = False
    # ROW-LISTED weight gradient (VERDICT r03 next #4a; LLMREC_WGRAD_ROWS=0: the dense launch). The gradient of the five attribute
    # streams' projected features is EXACTLY ZERO outside the rows the batch reaches: an attribute stream meets the loss in the fused
    # embeddings and BPR terms of the batch's rows only (Models.py:160-163,188-197; main.py:249-254), so dU_cat[:, attribute columns] is
    # non-zero in the batch's users (fusion backward) and in the users adjacent to the batch's items (A_iu^T of the items' rows) - 43 %
    # of the users at the Netflix shape. llmrec_batch_reach_rows lists those rows (beside the forward: _plan_reach_rider) and the
    # weight-gradient launch streams the listed rows of dU_cat and A_ui F_k only (llmrec_wgrad_problem_t.row_list): the same sums
    # without the terms that are zero. The image / text streams stay dense (the feature regulariser reads every row, main.py:151-156),
    # and so does user_trans (its gradient is two hops wide: 66 % of the rows).
    wgrad_rows = bool(wgrad_rows_default and env.get("LLMREC_WGRAD_ROWS", "1") == "1" and preprop
                      and n_attr > 0 and gemm == "bf16x3")     # (the exact-fp32 launches ignore the list: do not build it)
    # AdamW inside the step, in two launches: the embedding tables as soon as the ID chain's backward has produced their
    # gradients (beside the weight-gradient GEMM), the four Linears right after the slab reduction of that GEMM - the
    # step's tail is then one small launch instead of reduction -> cross-stream join -> a 1.96 M-parameter update.
    # (Batch-sharded replicas all-reduce the gradients first and update afterwards: llmrec_amd/dp.py sets this to False.)
    inline_adamw = bool(inline_adamw_default)
    # FOLDED launches (round 5; LLMREC_FOLD=0 restores the separate launches): AdamW's counter advances inside the scores
    # launch ("a new step begins": llmrec_bpr_multi_scores_step_f32), the feature regulariser's sum of squares comes out of the fusion launch
    # as per-block partials (llmrec_fuse_fwd_multi_sumsq_f32: it holds those rows anyway) and is reduced by the ONE launch that also forms
    # the loss values and assembles the logged scalars (llmrec_bpr_multi_losses_assemble_f32), the user table's AdamW reads inv * dE_u
    # directly and stores it as the table's .grad on the way (no axpy), and the row-wise clean-up of the scatter targets rides in the item
    # table's AdamW launch (llmrec_adamw_multi_zero_rows_f32): eight launches fewer, same arithmetic except the regulariser's summation tree.
    fold = bool(fold_default and env.get("LLMREC_FOLD", "1") == "1" and inline_adamw)
    # MASKED side product of the backward (LLMREC_BWD_MASK=0: the dense calls; =spmm: the product's mask without the fusion backward's
    # skip). dI_cat's attribute slices (2 ..) are exactly zero outside the rows of the batch's items - the argument of the row-listed
    # weight gradient above, one product earlier - and the loss launch stamps those rows in flag_i. dU_cat += A_iu^T dI_cat then
    # gathers, in the slices from 2 on, the stamped rows only and leaves user rows without a stamped neighbour untouched
    # (llmrec_spmm_epilogue_t.x_mask_stamp: the stamp is read on the device, so a replayed graph follows it); the fusion backward in
    # turn no longer writes the zeros nobody reads (llmrec_fuse_bwd_problem_t.zero_skip_from_term). Same bits as the dense calls.
    # Needs the stamps (the folded loss launch), one 64-column slice per stream and exactly the product the mask is compiled for -
    # latency-bound, pattern-only, weighted by col_scale (an adjacency that keeps its values runs the dense calls); dU_cat keeps
    # its dense zeros (the dense weight-gradient fallbacks read every row).
    want = env.get("LLMREC_BWD_MASK", "1")
    bwd_mask = bool(want != "0" and fold and d == 64 and n_attr > 0 and bwd_nnz < latency_nnz and not bwd_valued and bwd_col_scaled)
    # RESTORATION (restore): the term's gradient lands in the mask nodes' rows of dI_cat's attribute slices - rows the batch need not
    # reach. The masked side product and the fusion backward's skip both rest on "zero outside the batch's rows": off. (So does the
    # row-listed weight gradient, which is off already: mask_items has taken the pre-propagated operands away.)
    if restore:
        bwd_mask = False
    bwd_zero_skip = bwd_mask and want != "spmm"
    # HOSTED ID chain (round 15; LLMREC_HOST_CHAIN=0: the chain's first product in the first SpMM group, as before). The chain's first
    # product A_ui E_i needs nothing from the projection, and the grouped projection's last round of work units leaves block slots
    # empty once the launch has more units than the device has slots: the product runs as trailing blocks of that launch
    # (llmrec_linear_fwd_grouped_host_spmm_bf16x3) and the forward needs one SpMM group fewer. Same bits: every row keeps its tree.
    # HOSTED backward product (round 16; the same variable's third value, LLMREC_HOST_CHAIN=fwd: the forward hosting only - round 15's
    # step, the A/B reference). The weight-gradient launch is laid out for FusedStep.wgrad_blocks = 224 blocks, each of which owns a CU,
    # and the one-stream step has nothing else to run on the other CUs for the launch's ~100 us. The first product of the ID chain's
    # backward that has no side or profile partner left to share a group with (iu.bwd: bufI -> bufU) is independent of that launch:
    # it runs there, as persistent blocks behind the weight gradient's (llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3), and the
    # chain's remaining product and tail follow the launch instead of preceding it. Same bits: the slab length, and with it dW's
    # summation, depends on the block budget alone, and every row of the product keeps its tree. FusedStep applies it where its gate
    # holds (_host_wgrad_applies). Any value but "0" / "fwd" is the default: both hostings.
    want = env.get("LLMREC_HOST_CHAIN", "1")
    host_chain = want != "0"
    host_wgrad = want != "fwd"
    return StepOptions(drop_rate, check_zero, multi_stream, gemm, preprop, wgrad_rows, inline_adamw, fold, bwd_mask, bwd_zero_skip,
                       host_chain, host_wgrad)
