"""GPU: the grouped projection hosting one SpMM as trailing blocks (llmrec_linear_fwd_grouped_host_spmm_bf16x3) against the two separate
calls, llmrec_linear_fwd_grouped_bf16x3 followed by llmrec_spmm_f32 (each held to float64 elsewhere: tests/test_gpu_dense_families.py,
tests/test_gpu_spmm_families.py): the projections' Y and the product's Y `torch.equal`.

Shapes, the smallest that reach every path:
  projections  three problems of 11 000 / 11 000 / 11 003 rows, K = 32 / 64 / 96, N = 64: 86 + 86 + 86 = 258 >= 256 units of 128 rows, the
               <4, 2, 3> instance the hosting kernel is compiled for, a ragged last unit (11 003 = 85 x 128 + 123), one problem with
               bias_scale. With 300 rows each the launch has 64-row units - an instance the host is not compiled for: refused.
  product      700 rows, ~6 000 random edges and, planted, an empty row and rows at every bucket boundary of the operand's plan (32 / 33,
               t_wave / t_wave + 1, t_block: thresholds read from the plan), a row of ~600 and one of t_block - 36 non-zeros (the bench
               graph's longest row has 2 012 of t_block = 2 048). The rows' columns are distinct, so the operand is t_block + 256 columns wide
               rather than ~900. The lane-group, wavefront and block buckets are all non-empty (asserted); the block bucket's rows run the
               eight partial sums of the 512-thread block on four wavefronts.
Refused with LLMREC_EUNSUPPORTED and nothing written: a split-row operand (a row of t_block + 1), the softmax epilogue, an accumulating
product (Z) - the hosted body is compiled without an epilogue."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENTRY = "llmrec_linear_fwd_grouped_host_spmm_bf16x3"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def _rand(rng, *shape):
    return torch.tensor(rng.standard_normal(shape).astype(np.float32), device=DEV)


def _projections(rng, rows):
    """[(X, W, bias, bias_scale or None)] of the three problems"""
    out = []
    for k, (M, K) in enumerate(zip(rows, (32, 64, 96))):
        out.append((_rand(rng, M, K), _rand(rng, 64, K), _rand(rng, 64), _rand(rng, M) if k == 1 else None))
    return out


def _linear_problems(ops, projs, Ys):
    arr = (ops.LinearProblem * len(projs))()
    for i, ((X, W, b, bs), Y) in enumerate(zip(projs, Ys)):
        arr[i].X, arr[i].ldx, arr[i].M, arr[i].K = X.data_ptr(), ops._ld(X), X.shape[0], X.shape[1]
        arr[i].W, arr[i].ldw, arr[i].bias = W.data_ptr(), ops._ld(W), b.data_ptr()
        arr[i].Y, arr[i].ldy = Y.data_ptr(), ops._ld(Y)
        arr[i].bias_scale = bs.data_ptr() if bs is not None else None
    return arr


def _operand(ops, planted, seed, n_rows=700, n_edges=6000):
    """ui.fwd of a random bipartite graph with the planted row lengths (distinct columns per row)"""
    rng = np.random.default_rng(seed)
    n_cols = max(planted) + 256
    deg = np.bincount(rng.integers(0, n_rows, size=n_edges), minlength=n_rows)
    deg = np.minimum(deg, 32)                                   # the random part: lane-group rows
    for k, dg in enumerate(planted):
        deg[(k * 37 + 5) % n_rows] = dg
    rows = np.repeat(np.arange(n_rows), deg)
    cols = np.concatenate([rng.choice(n_cols, size=dg, replace=False) for dg in deg])
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), n_rows, n_cols)
    return g.ui.fwd, n_rows, n_cols


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


def _separate(ops, projs, Ys, pr):
    from llmrec_amd import _lib
    _lib.call("llmrec_linear_fwd_grouped_bf16x3", len(projs), _linear_problems(ops, projs, Ys), 64, ops._stream())
    _lib.call("llmrec_spmm_f32", pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X, pr.ldx, pr.Y, pr.ldy,
              pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, ops._stream())
    torch.cuda.synchronize()


def _hosted(ops, projs, Ys, pr) -> bool:
    from llmrec_amd import _lib
    ok = _lib.call_unless_unsupported(ENTRY, len(projs), _linear_problems(ops, projs, Ys), 64, ctypes.byref(pr), ops._stream())
    torch.cuda.synchronize()
    return ok


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _untouched(ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


@pytest.fixture(scope="module")
def thresholds(ops):
    from llmrec_amd import _lib
    _, (t_wave, t_block, _) = ops.spmm_shape(64, 6000)
    return _lib.CONST["LLMREC_SPMM_LONG_ROW"], t_wave, t_block


@pytest.mark.parametrize("n_rows,n_edges", [(700, 6000), (17000, 60000)], ids=["one_task_per_lane_group", "pipelined_short_rows"])
def test_hosted_launch_equals_the_two_separate_calls(ops, thresholds, n_rows, n_edges):
    """17 000 rows: more lane-group tasks than 1 024 blocks of 16 hold, so the 256-thread layout runs the short rows as software pipelines
    (rows_body_pipe, two tasks per lane group) - the other path of the lane-group bucket."""
    short, t_wave, t_block = thresholds
    planted = [0, short, short + 1, t_wave, t_wave + 1, 600, t_block - 36, t_block]
    a, n_rows, n_cols = _operand(ops, planted, seed=21, n_rows=n_rows, n_edges=n_edges)
    pl = a.plan_for(64)[1]
    assert (pl.t_wave, pl.t_block) == (t_wave, t_block)
    n_lane_rows = pl.n_short if pl.slot_row is not None else n_rows - pl.n_long
    assert n_lane_rows > 0 and pl.n_wave >= 2 and pl.n_block >= 4 and pl.n_split == 0, (n_lane_rows, pl.n_wave, pl.n_block, pl.n_split)
    rng = np.random.default_rng(22)
    projs = _projections(rng, (11000, 11000, 11003))
    Xs = _rand(rng, n_cols, 64)
    want_Y, got_Y = [_nan(p[0].shape[0], 64) for p in projs], [_nan(p[0].shape[0], 64) for p in projs]
    want_S, got_S = _nan(n_rows, 64), _nan(n_rows, 64)
    pr_w, keep_w = _spmm_problem(ops, a, Xs, want_S)
    _separate(ops, projs, want_Y, pr_w)
    pr_g, keep_g = _spmm_problem(ops, a, Xs, got_S)
    assert _hosted(ops, projs, got_Y, pr_g)
    assert bool(torch.isfinite(want_S).all()) and all(bool(torch.isfinite(y).all()) for y in want_Y)
    assert int((want_S != 0).any(dim=1).sum()) > n_rows // 2            # (an empty row is a row of zeros)
    for i, (w, g) in enumerate(zip(want_Y, got_Y)):
        assert torch.equal(w.view(torch.int32), g.view(torch.int32)), ("projection", i)
    bad = torch.nonzero((want_S.view(torch.int32) != got_S.view(torch.int32)).any(dim=1)).flatten()
    assert bad.numel() == 0, ("product rows", bad[:8].tolist())


def test_64_row_units_are_refused(ops, thresholds):
    """300 rows per problem: 9 units of 128 rows, so the launch has 64-row units - <4, 1, 3>, which the hosting kernel is not compiled for."""
    a, n_rows, n_cols = _operand(ops, [thresholds[1] + 1, 600], seed=23)
    rng = np.random.default_rng(24)
    projs = _projections(rng, (300, 300, 300))
    Ys, S = [_nan(300, 64) for _ in projs], _nan(n_rows, 64)
    pr, keep = _spmm_problem(ops, a, _rand(rng, n_cols, 64), S)
    assert not _hosted(ops, projs, Ys, pr)
    assert _untouched(Ys + [S])


@pytest.mark.parametrize("what", ["split_row", "softmax", "accumulate"])
def test_products_outside_the_hosted_form_are_refused(ops, thresholds, what):
    short, t_wave, t_block = thresholds
    a, n_rows, n_cols = _operand(ops, [t_wave + 1, 600] + ([t_block + 1] if what == "split_row" else []), seed=25)
    rng = np.random.default_rng(26)
    projs = _projections(rng, (11000, 11000, 11003))
    Ys, S = [_nan(p[0].shape[0], 64) for p in projs], _nan(n_rows, 64)
    Z = _rand(rng, n_rows, 64)
    epi = {"split_row": None, "softmax": ops.spmm_epilogue(ops.EPI_SOFTMAX), "accumulate": ops.spmm_epilogue(ops.EPI_NONE, 1.0, Z)}[what]
    if what == "split_row":
        assert a.plan_for(64)[1].n_split == 1
    pr, keep = _spmm_problem(ops, a, _rand(rng, n_cols, 64), S, epi)
    assert not _hosted(ops, projs, Ys, pr)
    assert _untouched(Ys + [S])
