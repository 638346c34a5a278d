"""GPU: the multi-target weight gradient + AdamW hosting one SpMM in the CUs its launch leaves free
(llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3) against the two separate calls, llmrec_linear_wgrad_multi_adamw_bf16x3 followed by
llmrec_spmm_f32 (each held to float64 elsewhere: tests/test_gpu_dense_families.py, tests/test_gpu_spmm_families.py): dW, db, W, b, both
moments of each and the product's Y `torch.equal`.

Shapes, the smallest that reach every path:
  weight gradient  two targets, K = 128 and K = 256, N = 64, each with problems of 300 and 77 rows; the 300-row problem of the first
                   target is row-listed, with 41 of its rows and once with none. One slab length for all (64 rows: the launch is far
                   below one round), so 5 + 2 slabs = 2 groups of four per target and 2 x 1 + 2 x 2 = 6 blocks - which the refusal at
                   n_cu = 6 beside the acceptance at n_cu = 10 pins down.
  product          the step's iu.bwd shape: a 600 x 500 pattern weighted by col_scale, Y = alpha Z + A X, d = 64, Y pre-filled with
                   NaN; rows of 0, 1, 31, 32, 33 non-zeros, the wavefront threshold and one above it (the first block-bucket length)
                   and one longer block-bucket row (thresholds from ops.spmm_shape). n_cu = 10: 4 guests for more than 12 virtual
                   blocks, so every guest's loop turns at least three times; n_cu = 256: more guests than virtual blocks.
Refused - "not accepted", every output at its sentinel: N = 128, a target with K % 128 != 0, n_cu = 6 (no CU left), a softmax epilogue,
a masked product, a sliced product, a plan with split rows, and Y inside the workspace."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
WG_BLOCKS = 6


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def _rand(rng, *shape, scale=1.0):
    return torch.tensor((scale * rng.standard_normal(shape)).astype(np.float32), device=DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def thresholds(ops):
    from llmrec_amd import _lib
    _, (t_wave, t_block, _) = ops.spmm_shape(64, 6000)
    return _lib.CONST["LLMREC_SPMM_LONG_ROW"], t_wave, t_block


# ------------------------------------------------------------------------------------------------------------------------------------
# the weight gradient's operands (read-only, shared) and one run's parameters
# ------------------------------------------------------------------------------------------------------------------------------------
def _operands(n_listed, N=64, Ks=(128, 256), seed=31):
    """[(K, [(dY, X, None, row list or None)])]: per target a 300-row and a 77-row problem; target 0's first is row-listed"""
    rng = np.random.default_rng(seed)
    out = []
    for ti, K in enumerate(Ks):
        pairs = []
        for pi, M in enumerate((300, 77)):
            dY, X, rows = _rand(rng, M, N), _rand(rng, M, K), None
            if ti == 0 and pi == 0 and n_listed is not None:
                ids = np.sort(rng.choice(M, size=n_listed, replace=False)).astype(np.int32)
                keep = torch.zeros(M, dtype=torch.bool, device=DEV)
                keep[torch.from_numpy(ids.astype(np.int64)).to(DEV)] = True
                dY[~keep] = 0.0                                           # the contract: a row that is not listed is all-zero
                row_list = torch.zeros(M + 32, dtype=torch.int32, device=DEV)
                row_list[:n_listed] = torch.from_numpy(ids).to(DEV)
                rows = (row_list, torch.tensor([n_listed], dtype=torch.int32, device=DEV), 0)
            pairs.append((dY, X, None, rows))
        out.append((K, pairs))
    return out


def _params(operands, N=64, seed=32):
    """fresh (W, b) per target with NaN gradients, the same values every call"""
    rng = np.random.default_rng(seed)
    lin = []
    for K, _ in operands:
        W, b = _rand(rng, N, K, scale=0.05), _rand(rng, N, scale=0.05)
        W.grad, b.grad = _nan(N, K), _nan(N)
        lin.append((W, b))
    return lin


def _outputs(opt, lin):
    out = []
    for W, b in lin:
        for p in (W, b):
            out += [p.detach().clone(), p.grad.clone(), opt.state[p][0].clone(), opt.state[p][1].clone()]
    return out


def _wgrad(ops, operands, host_spmm=None, ws=None, N=64):
    """one optimizer step through ops.linear_wgrad_multi -> (accepted or None, outputs, initial outputs)"""
    lin = _params(operands, N)
    params = [p for Wb in lin for p in Wb]
    opt = ops.FusedAdamW(params, lr=1e-3)
    opt.advance()
    for p in params:
        opt.moments(p)
    before = _outputs(opt, lin)
    targets = [(pairs, W.grad, b.grad, False) for (_, pairs), (W, b) in zip(operands, lin)]
    ok = ops.linear_wgrad_multi(targets, ws, update=(opt, lin), host_spmm=host_spmm)
    torch.cuda.synchronize()
    return ok, _outputs(opt, lin), before


# ------------------------------------------------------------------------------------------------------------------------------------
# the product
# ------------------------------------------------------------------------------------------------------------------------------------
def _operand(ops, planted, seed, n_rows=600, n_cols=500, n_edges=5000):
    """iu.bwd of a random bipartite graph - pattern-only, weighted by col_scale - with the planted row lengths (distinct columns per row)"""
    rng = np.random.default_rng(seed)
    deg = np.minimum(np.bincount(rng.integers(0, n_rows, size=n_edges), minlength=n_rows), 30)     # the random part: lane-group rows
    for k, dg in enumerate(planted):
        deg[(k * 37 + 5) % n_rows] = dg
    rows = np.repeat(np.arange(n_rows), deg)
    cols = np.concatenate([rng.choice(n_cols, size=dg, replace=False) for dg in deg])
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), n_rows, n_cols)
    a = g.iu.bwd
    assert a.val is None and a.col_scale is not None and (a.n_rows, a.n_cols) == (n_rows, n_cols)
    return a


def _spmm_problem(ops, a, X, Y, epi=None):
    d = X.shape[1]
    sw, pl = a.plan_for(d, whole_row=epi is not None and epi.op != ops.EPI_NONE)
    partials = torch.empty(pl.n_seg * d, dtype=torch.float32, device=DEV) if pl.n_seg else None
    rp, ci = pl.csr_of(a)
    pc = pl.c_struct()
    pr = ops.SpmmProblemC(a.n_rows, a.n_cols, rp.data_ptr(), ci.data_ptr(), ops._ptr(a.val), ops._ptr(a.row_scale), ops._ptr(a.col_scale),
                          X.data_ptr(), ops._ld(X), Y.data_ptr(), ops._ld(Y), d, sw, ctypes.addressof(pc), ops._ptr(partials),
                          ctypes.addressof(epi) if epi is not None else None)
    return pr, (pc, epi, partials, rp, ci)


def _spmm(ops, pr):
    from llmrec_amd import _lib
    _lib.call("llmrec_spmm_f32", pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X, pr.ldx, pr.Y, pr.ldy,
              pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, ops._stream())
    torch.cuda.synchronize()


def _same(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not torch.equal(g.view(torch.int32), w.view(torch.int32))]
    assert not bad, (what, bad)


@pytest.fixture(scope="module")
def product(ops, thresholds):
    """(operand, X, Z, alpha, the reference Y of llmrec_spmm_f32, virtual blocks of the 256-thread layout)"""
    short, t_wave, t_block = thresholds
    a = _operand(ops, [0, 1, short - 1, short, short + 1, t_wave, t_wave + 1, 400], seed=33)
    pl = a.plan_for(64)[1]
    assert (pl.t_wave, pl.t_block) == (t_wave, t_block) and pl.n_wave >= 2 and pl.n_block == 2 and pl.n_split == 0, (pl.n_wave, pl.n_block, pl.n_split)
    n_lane_rows = pl.n_short if pl.slot_row is not None else a.n_rows - pl.n_long
    virtual_blocks = pl.n_block + -(-pl.n_wave // 4) + -(-n_lane_rows // 16)          # 16 lane groups, 4 wavefronts per 256-thread block
    rng = np.random.default_rng(34)
    X, Z, alpha = _rand(rng, a.n_cols, 64), _rand(rng, a.n_rows, 64), 1.0 / 3.0
    want = _nan(a.n_rows, 64)
    pr, keep = _spmm_problem(ops, a, X, want, ops.spmm_epilogue(ops.EPI_NONE, alpha, Z))
    _spmm(ops, pr)
    assert bool(torch.isfinite(want).all()) and int((want != 0).any(dim=1).sum()) > a.n_rows // 2
    return a, X, Z, alpha, want, virtual_blocks


@pytest.mark.parametrize("n_cu", [WG_BLOCKS + 4, 256], ids=["4_guests_loop", "more_guests_than_blocks"])
@pytest.mark.parametrize("n_listed", [41, 0], ids=["41_of_300_listed", "empty_list"])
def test_hosted_launch_equals_the_two_separate_calls(ops, product, n_listed, n_cu):
    a, X, Z, alpha, want_Y, virtual_blocks = product
    n_guest = n_cu - WG_BLOCKS
    print("[wgrad host] %d virtual blocks on %d guests" % (virtual_blocks, n_guest))
    assert virtual_blocks > 3 * n_guest if n_cu < 256 else virtual_blocks < n_guest
    operands = _operands(n_listed)
    ok, want, before = _wgrad(ops, operands)
    assert ok is None and all(bool(torch.isfinite(t).all()) for t in want)
    assert all(not torch.equal(w, b) for w, b in zip(want, before))                  # every tensor moved: gradients, parameters, moments
    got_Y = _nan(a.n_rows, 64)
    pr, keep = _spmm_problem(ops, a, X, got_Y, ops.spmm_epilogue(ops.EPI_NONE, alpha, Z))
    ok, got, _ = _wgrad(ops, operands, host_spmm=(pr, n_cu))
    assert ok is True
    _same(got, want, "weight gradient, parameters, moments")
    bad = torch.nonzero((want_Y.view(torch.int32) != got_Y.view(torch.int32)).any(dim=1)).flatten()
    assert bad.numel() == 0, ("product rows", bad[:8].tolist())


def _refused(ops, operands, pr, Y, n_cu=256, ws=None, N=64):
    ok, got, before = _wgrad(ops, operands, host_spmm=(pr, n_cu), ws=ws, N=N)
    assert ok is False
    _same(got, before, "refused: gradients (NaN), parameters and moments untouched")
    assert bool(torch.isnan(Y).all())


@pytest.mark.parametrize("what", ["N_128", "K_192", "no_free_cu"])
def test_launches_outside_the_hosting_form_are_refused(ops, product, what):
    a, X, Z, alpha, _, _ = product
    Y = _nan(a.n_rows, 64)
    pr, keep = _spmm_problem(ops, a, X, Y, ops.spmm_epilogue(ops.EPI_NONE, alpha, Z))
    if what == "N_128":
        _refused(ops, _operands(None, N=128), pr, Y, N=128)
    elif what == "K_192":                                                  # organisation 1: 64-wide k slabs
        _refused(ops, _operands(None, Ks=(128, 192)), pr, Y)
    else:                                                                  # wg_blocks >= n_cu
        _refused(ops, _operands(41), pr, Y, n_cu=WG_BLOCKS)


@pytest.mark.parametrize("what", ["softmax", "masked", "sliced", "split_row", "unweighted"])
def test_products_outside_the_hosted_form_are_refused(ops, product, thresholds, what):
    a, X, Z, alpha, _, _ = product
    rng = np.random.default_rng(35)
    d, epi = 64, ops.spmm_epilogue(ops.EPI_NONE, alpha, Z)
    if what == "softmax":
        epi = ops.spmm_epilogue(ops.EPI_SOFTMAX)
    elif what == "masked":
        epi = ops.spmm_epilogue(ops.EPI_NONE, alpha, Z, x_row_mask=torch.ones(a.n_cols, dtype=torch.uint8, device=DEV), x_mask_active=1)
    elif what == "sliced":                                                 # 128 columns: two 64-column slices in the latency-bound regime
        d, epi = 128, None
        assert a.plan_for(128)[0] == 64
    elif what == "split_row":
        a = _operand(ops, [thresholds[2] + 1], seed=36, n_cols=thresholds[2] + 256)
        assert a.plan_for(64)[1].n_split == 1
        Z = _rand(rng, a.n_rows, 64)
        epi = ops.spmm_epilogue(ops.EPI_NONE, alpha, Z)
    elif what == "unweighted":                                             # the projection host's shape, not this host's
        a = ops.Csr(a.n_rows, a.n_cols, a.rowptr, a.colidx, None, None, None, a.plans)
        epi = None
    Y = _nan(a.n_rows, d)
    pr, keep = _spmm_problem(ops, a, _rand(rng, a.n_cols, d), Y, epi)
    _refused(ops, _operands(41), pr, Y)


def test_a_product_inside_the_workspace_is_refused(ops, product):
    a, X, Z, alpha, _, _ = product
    operands = _operands(41)
    lin = _params(operands)
    need = ops.linear_wgrad_multi_workspace([(pairs, W.grad, b.grad, False) for (_, pairs), (W, b) in zip(operands, lin)])
    assert need > 0
    ws = torch.full((max(need, a.n_rows * 64 * 4) // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    Y = ws[:a.n_rows * 64].view(a.n_rows, 64)
    pr, keep = _spmm_problem(ops, a, X, Y, ops.spmm_epilogue(ops.EPI_NONE, alpha, Z))
    _refused(ops, operands, pr, Y, ws=ws.view(torch.uint8))
    assert bool(torch.isnan(ws).all())
