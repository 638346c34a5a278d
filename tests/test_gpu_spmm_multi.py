"""GPU: grouped SpMM launches (llmrec_spmm_multi_f32) give the same bits as separate llmrec_spmm_f32 calls - at the bench's headline shape,
with sliced [rows, 7 x 64] operands beside d = 64 ones, every epilogue, weighted (transposed) operands, permuted-CSR plans, split rows
(the grouped finalize launch) and one to four problems - and refuse mixed kernel instances and aliased outputs."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def _problem(ops, a, X, Y, epi=None, partials=None):
    """(llmrec_spmm_problem_t, the objects it points to) of Y = epi(A X)."""
    d = X.shape[1]
    sw, pl = a.plan_for(d, whole_row=epi is not None and epi.op != ops.EPI_NONE)
    if pl.n_seg and partials is None:
        partials = torch.empty(pl.n_seg * d, dtype=torch.float32, device=DEV)
    rp, ci = pl.csr_of(a)
    pc = pl.c_struct()
    pr = ops.SpmmProblemC(a.n_rows, a.n_cols, rp.data_ptr(), ci.data_ptr(), ops._ptr(a.val), ops._ptr(a.row_scale), ops._ptr(a.col_scale),
                          X.data_ptr(), ops._ld(X), Y.data_ptr(), ops._ld(Y), d, sw, ctypes.addressof(pc), ops._ptr(partials),
                          ctypes.addressof(epi) if epi is not None else None)
    return pr, (pc, epi, partials, rp, ci)


def _single(ops, pr):
    from llmrec_amd import _lib
    _lib.call("llmrec_spmm_f32", pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X, pr.ldx, pr.Y, pr.ldy,
              pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, ops._stream())


def _run(ops, specs, grouped):
    """specs: [(a, X, Y0, epi_of(Y) or None)]. Returns the outputs (fresh copies of Y0) after one grouped or len(specs) single launches."""
    outs, probs, keep = [], [], []
    for a, X, Y0, epi_of in specs:
        Y = Y0.clone()
        pr, k = _problem(ops, a, X, Y, epi_of(Y) if epi_of is not None else None)
        outs.append(Y); probs.append(pr); keep.append(k)
    if grouped:
        assert ops.spmm_multi(probs)
    else:
        for pr in probs:
            _single(ops, pr)
    torch.cuda.synchronize()
    return outs


def _check(ops, specs):
    want = _run(ops, specs, grouped=False)
    got = _run(ops, specs, grouped=True)
    for i, (w, g) in enumerate(zip(want, got)):
        assert torch.equal(w.view(torch.int32), g.view(torch.int32)), i


def _rand(rng, *shape):
    return torch.tensor(rng.standard_normal(shape).astype(np.float32), device=DEV)


@pytest.fixture(scope="module")
def headline(ops):
    """The bench's Netflix shape: 13 187 users x 17 366 items, 55 146 train edges."""
    from llmrec_amd import synth
    U, I = 13187, 17366
    rows, cols = synth.bipartite_edges(U, I, 55146, seed=3)
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), U, I)
    return g, U, I


def test_grouped_forward_and_backward_groups_of_the_step(ops, headline):
    g, U, I = headline
    rng = np.random.default_rng(5)
    d, S = 64, 7
    E_i, U_cat, P_usr = _rand(rng, I, d), _rand(rng, U, S * d), _rand(rng, U, d)
    assert g.ui.fwd.plan_for(d)[1].slot_row is not None                      # pattern-only: the permuted CSR
    sm = lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX)
    # forward: chain layer (softmax or not) + the sliced side product + the profile product; pattern-only, unweighted
    for chain_epi in (None, sm):
        _check(ops, [(g.ui.fwd, E_i, torch.zeros(U, d, device=DEV), chain_epi),
                     (g.iu.fwd, U_cat, torch.zeros(I, S * d, device=DEV), None),
                     (g.iu.fwd, P_usr, torch.zeros(I, d, device=DEV), None)])
    # backward: transposed (col_scale-weighted) operands; softmax backward with Z / S, accumulation into the sliced output, "+ Z"
    gI, Zu, Su = _rand(rng, I, d), _rand(rng, U, d), torch.softmax(_rand(rng, U, d), dim=-1)
    dI_cat, dU_cat0, dprof_u, dprof_i0 = _rand(rng, I, S * d), _rand(rng, U, S * d), _rand(rng, U, d), _rand(rng, I, d)
    _check(ops, [(g.iu.bwd, gI, torch.zeros(U, d, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX_BWD, 1 / 3, Zu, Su)),
                 (g.iu.bwd, dI_cat, dU_cat0, lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y)),
                 (g.ui.bwd, dprof_u, dprof_i0, lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y))])
    Zi = _rand(rng, I, d)
    _check(ops, [(g.ui.bwd, _rand(rng, U, d), torch.zeros(I, d, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1 / 3, Zi)),
                 (g.iu.bwd, _rand(rng, I, d), torch.zeros(U, d, device=DEV), None)])


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_one_to_four_problems(ops, headline, n):
    g, U, I = headline
    rng = np.random.default_rng(10 + n)
    pool = [(g.ui.fwd, _rand(rng, I, 64), torch.zeros(U, 64, device=DEV), None),
            (g.iu.fwd, _rand(rng, U, 448), torch.zeros(I, 448, device=DEV), None),
            (g.iu.fwd, _rand(rng, U, 64), torch.zeros(I, 64, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX)),
            (g.ui.fwd, _rand(rng, I, 64), _rand(rng, U, 64), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y))]
    _check(ops, pool[:n])


def test_split_rows_use_the_grouped_finalize(ops):
    """Hub rows longer than the plan's block threshold are cut into segments; two such problems in one launch share one finalize launch."""
    rng = np.random.default_rng(77)
    n_rows, n_cols = 600, 45000
    degs = rng.integers(0, 40, size=n_rows)
    for k, dg in enumerate([0, 1, 32, 33, 511, 512, 513, 4095, 4096, 4097, 16384, 16385, 20000, 44000]):
        degs[(k * 13 + 1) % n_rows] = dg
    rows = np.repeat(np.arange(n_rows), degs)
    cols = np.concatenate([rng.choice(n_cols, size=dg, replace=False) for dg in degs])
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), n_rows, n_cols)
    assert g.ui.fwd.plan_for(64)[1].n_split > 0 and g.ui.fwd.plan_for(448)[1].n_split > 0
    Z, S = _rand(rng, n_rows, 64), torch.softmax(_rand(rng, n_rows, 64), dim=-1)
    _check(ops, [(g.ui.fwd, _rand(rng, n_cols, 448), torch.zeros(n_rows, 448, device=DEV), None),
                 (g.ui.fwd, _rand(rng, n_cols, 64), torch.zeros(n_rows, 64, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX_BWD, 0.5, Z, S)),
                 (g.iu.fwd, _rand(rng, n_rows, 64), torch.zeros(n_cols, 64, device=DEV), None)])
    _check(ops, [(g.ui.bwd, _rand(rng, n_rows, 64), torch.zeros(n_cols, 64, device=DEV), None),
                 (g.iu.bwd, _rand(rng, n_cols, 64), _rand(rng, n_rows, 64), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y))])


def test_mixed_instances_fall_back_and_aliases_are_refused(ops, headline):
    g, U, I = headline
    rng = np.random.default_rng(9)
    X_i, X_u = _rand(rng, I, 64), _rand(rng, U, 64)
    # unweighted forward + weighted transposed product: two kernel instances -> refused, nothing launched
    Y0, Y1 = torch.full((U, 64), 7.0, device=DEV), torch.full((U, 64), 7.0, device=DEV)
    p0, k0 = _problem(ops, g.ui.fwd, X_i, Y0)
    p1, k1 = _problem(ops, g.iu.bwd, X_i, Y1)
    assert not ops.spmm_multi([p0, p1])
    torch.cuda.synchronize()
    assert bool((Y0 == 7.0).all()) and bool((Y1 == 7.0).all())
    # one problem's output is another's operand (or output): refused as invalid
    Yi = torch.zeros(I, 64, device=DEV)
    p0, k0 = _problem(ops, g.ui.fwd, X_i, X_u)                                # writes X_u ...
    p1, k1 = _problem(ops, g.iu.fwd, X_u, Yi)                                 # ... which this one reads
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.spmm_multi([p0, p1])
    p1, k1 = _problem(ops, g.ui.fwd, X_i, X_u)                                # the same output twice
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.spmm_multi([p0, p1])
