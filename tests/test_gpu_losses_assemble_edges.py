"""GPU: llmrec_bpr_multi_losses_assemble_f32 (one wavefront per 1024-slot sum tree, no LDS tree) against the launches it replaces -
llmrec_bpr_multi_losses_f32 + llmrec_sumsq_f32 x 2 + llmrec_loss_assemble_f32 mode 0 - at the edges of the tree: batch sizes around
one wavefront and around the 1024 slots, partial counts around the slots, k = 0. `out`, `saved`, `scal` and the double running sums
are compared bit for bit. With partial sums the regulariser's value has no launch to be compared with (llmrec_sumsq_f32 sums other
operands); its reference is the float32 restatement of the 1024-slot tree on the CPU (tests/_tree_ref.py), also bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests._tree_ref import tree_lds

pytestmark = pytest.mark.gpu

DEV = "cuda"
p_ = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
N_PARTIAL = (0, 1, 1023, 1024, 1025, 4096)
RATES = (0.29, 1e-4)                                                    # 1e-4 * B < 1 for every B <= 4096: k = 0, mf = nan


def _mixed(rng, n, positive=False):
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 4, size=n)      # 1e-6 .. 1e4: a changed addition order shows
    return (np.abs(x) if positive else x).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int64)


@pytest.fixture(scope="module")
def inputs():
    """per (n_prob, B_max): the `saved` block (every slot mixed in magnitude, norms positive), shared and never written"""
    assert torch.cuda.is_available()
    from llmrec_amd import _lib, ops
    rng = np.random.default_rng(2024)
    cache = {}
    for P in (1, 3, 8):
        for cap in (1126, _lib.CONST["LLMREC_BPR_MAX_B"]):
            per = ops.bpr_saved_floats(cap)
            s = _mixed(rng, P * per).reshape(P, per)
            s[:, cap + 4 + 2 * cap:cap + 4 + 5 * cap] = np.abs(s[:, cap + 4 + 2 * cap:cap + 4 + 5 * cap])
            cache[(P, cap)] = torch.tensor(s.reshape(-1)).to(DEV)
    partial = _mixed(rng, max(N_PARTIAL), positive=True)
    X = [torch.tensor(_mixed(rng, 77 * 64).reshape(77, 64)).to(DEV) for _ in range(2)]
    return cache, partial, X


@pytest.mark.parametrize("cap", [1126, 4096])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_losses_assemble_equals_the_separate_launches_at_the_trees_edges(inputs, P, cap):
    from llmrec_amd import _lib
    cache, partial_h, X = inputs
    assert cap in (1126, _lib.CONST["LLMREC_BPR_MAX_B"])
    saved0 = cache[(P, cap)]
    partial_d = torch.tensor(partial_h).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    w_mf = [1.0, 0.02, 0.02, 0.012, 0.012, 0.012, 0.012, 0.012][:P]
    wc = (ctypes.c_float * P)(*w_mf)
    coef = np.float32(1e-5 * 0.5 / 1733)
    ws_bytes = _lib.query("llmrec_sumsq_workspace_bytes", 77, 64)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    feat_ref = {n: np.float32(coef * np.float32(tree_lds(partial_h[:n]))) for n in N_PARTIAL if n}
    checked = 0
    for nvalid in (1, 63, 64, 65, 1023, 1024, 1025, cap):
        nv = torch.tensor([nvalid], dtype=torch.int32, device=DEV)
        for n_part in N_PARTIAL:
            for rate in RATES:
                res = []
                k = int(rate * float(nvalid))
                for folded in (True, False):
                    saved, out = saved0.clone(), torch.full((P, 2), 3.0, device=DEV)
                    if k == 0:                                           # nothing is kept: the selection leaves zeros, the mean is 0 / 0
                        saved.view(P, -1)[:, 2 * cap + 4:3 * cap + 4] = 0.0
                    scal = torch.full((4,), 9.0, device=DEV)
                    running = torch.tensor([1.5, 2.5, 3.5], dtype=torch.float64, device=DEV)
                    if n_part == 0 or not folded:                        # the regulariser as the unfolded step forms it: two sumsq launches
                        _lib.call("llmrec_sumsq_f32", 77, 64, p_(X[0]), 64, float(coef), 0, p_(scal), p_(ws), ws.numel(), st)
                        _lib.call("llmrec_sumsq_f32", 77, 64, p_(X[1]), 64, float(coef), 1, p_(scal), p_(ws), ws.numel(), st)
                    if folded:
                        _lib.call("llmrec_bpr_multi_losses_assemble_f32", P, cap, p_(nv), rate, 1e-5, 64.0, p_(out), p_(saved), wc,
                                  p_(partial_d) if n_part else None, n_part, float(coef), p_(scal), p_(running), st)
                    else:
                        _lib.call("llmrec_bpr_multi_losses_f32", P, cap, p_(nv), rate, 1e-5, 64.0, p_(out), p_(saved), st)
                        if n_part:                                       # the tree over the partials: the CPU restatement's value
                            scal[0] = float(feat_ref[n_part])
                        _lib.call("llmrec_loss_assemble_f32", 0, P, p_(out), wc, p_(scal), None, 1.0, p_(running), st)
                    res.append((saved, out, scal, running))
                torch.cuda.synchronize()
                tag = (P, cap, nvalid, n_part, rate)
                for name, a, b in zip(("saved", "out", "scal", "running"), *res):
                    assert torch.equal(_bits(a), _bits(b)), (tag, name, a.flatten()[:8].tolist(), b.flatten()[:8].tolist())
                got_out = res[0][1].cpu()
                if k == 0:
                    assert bool(torch.isnan(got_out[:, 0]).all()) and bool(torch.isnan(res[0][2][1])), tag   # the empty mean
                else:
                    assert bool(torch.isfinite(got_out).all()), tag
                checked += 1
    assert checked == 8 * len(N_PARTIAL) * len(RATES)
