"""GPU: the training step with the backward's masked side product and the fusion backward's zero skip (FusedStep.bwd_mask) against the
same step with LLMREC_BWD_MASK=0, on the d = 64 golden fixture (nf_mid_lr): six eager steps, a replayed four-step graph (six steps in
all) and 260 eager steps - the row stamp wraps at 255, where the rows stamped 255 steps earlier read as stamped again. Every parameter,
Adam moment, gradient and logged scalar `torch.equal`; the one-stream and the four-stream schedule alike. An adjacency that keeps its
values (the mask is compiled for pattern-only operands weighted by col_scale) switches bwd_mask off by itself: the dense calls run."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_reproducible import datasets          # noqa: F401  (the nf_mid_lr dataset fixture)


def _valued(t, seed):
    """the sparse adjacency with every value scaled by its own factor: rows are no longer constant, the operand keeps val"""
    t = t.coalesce()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    f = 1.0 + 0.25 * torch.rand(t.values().shape, generator=gen)
    return torch.sparse_coo_tensor(t.indices(), t.values() * f.to(t.values().device), t.shape).coalesce()


def _steps(root, monkeypatch, mask, n, graph=False, streams=False, check_zero=False, valued=False):
    from tests._step_env import fused_trainer, snapshot
    from tests.conftest import GOLDEN
    from llmrec_amd.fused import FusedStep
    meta = json.load(open(os.path.join(GOLDEN, "nf_mid_lr", "meta.json")))
    env = {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1", "LLMREC_DEVICE_SAMPLER": "1", "LLMREC_BWD_MASK": mask,
           "LLMREC_STREAMS": "1" if streams else "0", "LLMREC_CHECK_ZERO": "1" if check_zero else "0"}
    argv = ["--dataset", meta["config"]["dataset"], "--data_path", root + "/"] + meta["config"]["argv"] + ["--epoch", "1"]

    def keep_values(tr):
        tr.ui_graph, tr.iu_graph = _valued(tr.ui_graph, 1), _valued(tr.iu_graph, 2)
    _, tr, step, batcher = fused_trainer(monkeypatch, argv, env, train=True, prepare=keep_values if valued else None, step=True, batcher=True)
    assert step and step.fold and step.multi_stream == streams
    if valued:
        assert step.iu.bwd.val is not None and not step.bwd_mask and not step.bwd_zero_skip
    else:
        assert step.bwd_mask == (mask != "0") and step.bwd_zero_skip == (mask == "1")
    if graph:
        step.capture(batcher=batcher, unroll=4)                         # (the capture's warm-up is the first step)
        step.run_steps(n - 1)
    else:
        st = step._make_static()
        for _ in range(n):
            step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
    torch.cuda.synchronize()
    assert int(batcher.step_dev) == n and int(step.row_stamp) >= n       # (the stamp advances once per step)
    return snapshot(tr, step, ("scal", "out", "epoch_sums", "static_block", "dU_cat"))


def _assert_equal(a, b):
    assert sorted(a) == sorted(b) and any(k.startswith("m/") for k in a) and any(k.startswith("g/") for k in a)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad[:6]
    assert bool(torch.isfinite(a["scal"]).all())


@pytest.mark.parametrize("how", ["eager", "graph_unroll4", "four_streams", "spmm_only"])
def test_six_masked_steps_equal_six_dense_steps(datasets, monkeypatch, how):
    kw = dict(graph=how == "graph_unroll4", streams=how == "four_streams")
    dense = _steps(datasets["nf_mid_lr"], monkeypatch, "0", 6, **kw)
    masked = _steps(datasets["nf_mid_lr"], monkeypatch, "spmm" if how == "spmm_only" else "1", 6, **kw)
    _assert_equal(masked, dense)


def test_masked_steps_across_the_stamps_wrap(datasets, monkeypatch):
    dense = _steps(datasets["nf_mid_lr"], monkeypatch, "0", 260)
    masked = _steps(datasets["nf_mid_lr"], monkeypatch, "1", 260)
    _assert_equal(masked, dense)


@pytest.mark.parametrize("mask", ["1", "spmm"])
def test_check_zero_verifies_the_promise(datasets, monkeypatch, mask):
    """LLMREC_CHECK_ZERO: the idle rows of dI_cat's attribute slices are zero (mask without the skip) or, poisoned with NaN, unread."""
    dense = _steps(datasets["nf_mid_lr"], monkeypatch, "0", 3)
    checked = _steps(datasets["nf_mid_lr"], monkeypatch, mask, 3, check_zero=True)
    _assert_equal(checked, dense)


def test_valued_adjacency_runs_the_dense_calls(datasets, monkeypatch):
    """The default (LLMREC_BWD_MASK=1) with operands that keep val: bwd_mask is off and the step equals the one with the mask disabled."""
    dense = _steps(datasets["nf_mid_lr"], monkeypatch, "0", 3, valued=True)
    default = _steps(datasets["nf_mid_lr"], monkeypatch, "1", 3, valued=True)
    _assert_equal(default, dense)
