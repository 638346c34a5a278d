"""GPU: the fused training step on its WIDE loss segment (FusedStep above FusedStep.WIDE_FROM; main.py builds such a step under
LLMREC_FUSED=wide, step_options.route).
  1  forced wide (WIDE_FROM = 0) against the default route on the nf_tiny golden case, three steps, eager and graph, bit for bit -
     also at LLMREC_FOLD=0 and LLMREC_STREAMS=1;
  2  tests/_step_ref.CASE_C (a batch of 4608 > LLMREC_BPR_MAX_B) IN THE FUSED STEP, row by row against the float64 oracle with the
     margins, helpers and conditions of tests/test_gpu_step_rows.py, which runs the same case on the per-op path. Measured on the MI355X,
     worst err / bound over the three steps (per tensor: profiles/experiments/step_rows.md, column C-fused; M = 16 / 8 / 16 / 16):
     forward 2.35, table 1.18, linear 1.34 (graph: 1.43), scalar 2.37, AdamW 0.49, smallest cut gap / (64 err) 5.03;
  3  the in-graph device sampler at --batch_size 4096 under LLMREC_FUSED=wide: the batches are tests/_sampler_ref.py's, a second fresh
     trainer reproduces every parameter and moment, eager equals the replays;
  4  the default is unchanged: without LLMREC_FUSED the trainer steps aside at --batch_size 4096."""
import numpy as np
import pytest
import torch

from tests import _rowops_ref as RR
from tests import _step_ref as S
from tests.test_gpu_step_rows import CASES, M, _drive, datasets  # noqa: F401  (datasets: the module fixture that writes the cases once)

pytestmark = pytest.mark.gpu

def _batch(golden, s):
    s = s % golden.n_steps
    return tuple(torch.tensor(golden.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))


def _three_steps(monkeypatch, env, wide_from, graph):
    from llmrec_amd import _lib
    from llmrec_amd.fused import FusedStep
    from tests._dropin import golden_argv
    from tests._step_env import fused_trainer, snapshot
    from tests.conftest import GoldenCase
    g = GoldenCase("nf_tiny")
    with monkeypatch.context() as mp:
        if wide_from is not None:
            mp.setattr(FusedStep, "WIDE_FROM", wide_from)
        b = fused_trainer(mp, golden_argv(g), dict(env, LLMREC_FUSED="1", LLMREC_GRAPH="1" if graph else "0"), seed=g.args["seed"], step=True)
        step = b.step
        assert step and step.wide == (wide_from is not None) and step.b_max <= _lib.CONST["LLMREC_BPR_MAX_B"]
        calls = set()
        invoke = _lib._invoke
        mp.setattr(_lib, "_invoke", lambda fn, args: (calls.add(fn), invoke(fn, args))[1])
        snaps = []
        for s in range(3):
            b.trainer.train_step(*_batch(g, s))
            torch.cuda.synchronize()
            assert (step.graph_exec is not None) == graph
            snap = snapshot(b.trainer, step, extra=("out", "scal", "flag_u", "flag_i", "epoch_sums", "row_stamp"))
            snap["out"] = snap["out"][:step.n_prob]                       # (the rows of the problems there are)
            snaps.append(snap)
    wide_calls = {c for c in calls if "_wide" in c and "bpr" in c}
    if wide_from is None:
        assert not wide_calls
    else:
        assert wide_calls == {"llmrec_bpr_scatter_plan_wide", "llmrec_bpr_multi_scores_wide_f32", "llmrec_bpr_multi_select_bwd_wide_f32",
                              "llmrec_bpr_multi_losses_wide_f32"}, wide_calls
        assert not calls & {"llmrec_bpr_scatter_plan", "llmrec_bpr_multi_scores_f32", "llmrec_bpr_multi_scores_step_f32",
                            "llmrec_bpr_multi_select_bwd_f32", "llmrec_bpr_multi_losses_f32", "llmrec_bpr_multi_losses_assemble_f32",
                            "llmrec_bpr_scatter_plan_reach_mark"}
    return snaps


# (four streams run eagerly only: the package refuses to capture a multi-branch graph, llmrec_amd/__init__.py)
ROUTES = {"default-eager": ({}, False), "default-graph": ({}, True), "unfolded-eager": ({"LLMREC_FOLD": "0"}, False),
          "unfolded-graph": ({"LLMREC_FOLD": "0"}, True), "streams-eager": ({"LLMREC_STREAMS": "1"}, False)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_forced_wide_equals_the_default_route(monkeypatch, route):
    env, graph = ROUTES[route]
    want = _three_steps(monkeypatch, env, None, graph)
    got = _three_steps(monkeypatch, env, 0, graph)
    for s, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for k in a:
            x, y = a[k], b[k]
            if x.is_floating_point():                                      # bit for bit (a NaN would have to be the same NaN)
                x, y = x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.contiguous().view(
                    torch.int32 if y.dtype == torch.float32 else torch.int64)
            assert torch.equal(x, y), (s, k)


PATHS_C = {"eager": {"LLMREC_FUSED": "wide", "LLMREC_GRAPH": "0"}, "graph": {"LLMREC_FUSED": "wide", "LLMREC_GRAPH": "1"}}


@pytest.mark.parametrize("path", list(PATHS_C))
def test_case_c_in_the_fused_step_row_by_row(datasets, monkeypatch, path):
    """Case C - 4608 triples, b_max = 5068 > LLMREC_BPR_MAX_B - trains in the fused step under LLMREC_FUSED=wide (on the parent commit the
    value means the per-op path: `b.step` is False there). The loop is tests/test_gpu_step_rows.py's for case B - the wide route runs
    case B's kernels plus an exact selection - with that file's margins M; the cut-gap and zero-row conditions are asserted unchanged."""
    from llmrec_amd import _lib
    from llmrec_amd.fused import FusedStep
    from tests._step_env import fused_trainer, snapshot
    name, case = "C", CASES["C"]
    root = datasets(name, None)
    b = fused_trainer(monkeypatch, S.case_argv(case, root), PATHS_C[path], train=True, step=True)
    assert isinstance(b.step, FusedStep) and b.step.b_max == 5068 > _lib.CONST["LLMREC_BPR_MAX_B"] and b.step.wide
    data, cfg, graphs = datasets.inputs(name, b.m.args)
    lr = float(b.m.args.lr)
    assert lr == 1e-3 and cfg.n_layers == 3 and tuple(cfg.keys) == tuple(data.keys)
    run = _drive("B", path, b, case, data, graphs, cfg)                 # case B's driver: tr.train_step on the injected island batches
    folded = bool(b.step.fold)
    fails, worst, worst_adamw, gaps_min = [], {}, {}, np.inf
    for s in range(S.STEPS):
        pre = snapshot(b.trainer, None, grads=False, cpu=True)
        batch, got = run(s)
        assert len(batch[0]) == 4608 > _lib.CONST["LLMREC_BPR_MAX_B"]
        post = snapshot(b.trainer, None, grads=True, cpu=True)
        got["grad"] = {k: post["g/" + k].numpy().astype(np.float64) for k in S.PARAMS}
        state = b.trainer.optimizer.dev_state.cpu().numpy()
        assert state.view(np.int32).tolist() == RR.adamw_state(s + 1, lr, S.ADAM["b1"], S.ADAM["b2"]).view(np.int32).tolist(), ("AdamW state", s, state)
        params = {k: pre["p/" + k] for k in S.PARAMS}
        r64 = S.oracle_step(params, data.feats, graphs, batch, cfg, torch.float64)
        r32 = S.oracle_step(params, data.feats, graphs, batch, cfg, torch.float32)
        gaps = S.cut_gaps(r64, r32)
        gaps_min = min(gaps_min, min(g[2] for g in gaps))
        assert all(g[2] >= 1.0 for g in gaps), ("cut gap below 64 fp32 errors", name, path, s, gaps)
        for tab in S.TABLES:                                             # the islands: exact zeros in both tables' gradients
            share = float((np.abs(r64["grad"][tab]).max(axis=1) > 0).mean())
            assert 0.0 < share <= 0.50, (tab, share)
        prov = S.Provenance(data.train_mat, batch, S.kept_sets(r64["maxi"], r64["keep"]))
        f, ratios = S.compare_step(got, r64, r32, M, prov)
        fails += ["step %d: %s" % (s, x) for x in f]
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k in S.PARAMS:
            bad, w = S.adamw_check(k, (pre["p/" + k].numpy(), pre["m/" + k].numpy() if "m/" + k in pre else None,
                                       pre["v/" + k].numpy() if "v/" + k in pre else None), post["g/" + k].numpy(),
                                   (post["p/" + k].numpy(), post["m/" + k].numpy(), post["v/" + k].numpy()), s + 1, lr,
                                   scaled_source=(folded and k == S.USER_TABLE))
            d = post["p/" + k].shape[-1]
            fails += ["step %d: AdamW %s element %d (row %d): |err| %.3e > bound %.3e" % (s, what, i, i // d, e, bd) for what, i, e, bd in bad]
            for what, v in w.items():
                worst_adamw[what] = max(worst_adamw.get(what, 0.0), v)
    by_family = {}
    for k, v in worst.items():
        by_family[S.family_of_key(k)] = max(by_family.get(S.family_of_key(k), 0.0), v)
    tag = "[step rows] C-fused-%s" % path
    for k in sorted(worst):
        print("%s ratio %-28s %.3g" % (tag, k, worst[k]))
    print("%s families %s; AdamW worst |err| / bound %s; smallest cut gap / (64 err) %.3g"
          % (tag, {k: "%.3g" % v for k, v in sorted(by_family.items())}, {k: "%.3g" % v for k, v in sorted(worst_adamw.items())}, gaps_min))
    assert not fails, "\n".join(fails[:12])


ENV_SAMPLER = {"LLMREC_FUSED": "wide", "LLMREC_DEVICE_SAMPLER": "1"}


def _sampled_run(monkeypatch, root, graph):
    """three steps of case A's dataset at --batch_size 4096 with the device sampler -> (per step the batch, the final parameters and moments)"""
    from llmrec_amd import _lib
    from llmrec_amd.fused import FusedStep
    from tests._step_env import fused_trainer, snapshot
    argv = S.case_argv(CASES["A"], root) + ["--batch_size", "4096"]
    with monkeypatch.context() as mp:
        b = fused_trainer(mp, argv, dict(ENV_SAMPLER, LLMREC_GRAPH="1" if graph else "0"), train=True, step=True, batcher=True)
        step, batcher = b.step, b.batcher
        assert isinstance(step, FusedStep) and step.wide and step.b_max == batcher.capacity > _lib.CONST["LLMREC_BPR_MAX_B"]
        batches = []
        st = None
        for s in range(3):
            if graph:
                if s == 0:
                    step.capture(batcher=batcher, unroll=1)              # the capture's warm-up is the first step
                else:
                    step.step()
                st = step.static
            else:
                st = st or step._make_static()
                step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
            torch.cuda.synchronize()
            assert int(batcher.step_dev) == s + 1
            nv = int(st["n_valid"])
            batches.append(tuple(st[k][:nv].cpu().numpy() for k in ("users", "pos", "neg")))
        snap = snapshot(b.trainer, step, extra=("out", "scal"), grads=True, cpu=True)
        info = (b.m.args.seed, list(b.m.data_generator.exist_users), float(b.m.args.aug_sample_rate))
    return batches, snap, info


def test_in_graph_sampler_on_the_wide_route(datasets, monkeypatch):
    root = datasets("A", None)
    batches, snap, (seed, exist, aug_rate) = _sampled_run(monkeypatch, root, graph=True)
    data = S.O.load_dataset(root + "/" + CASES["A"]["dataset"], __import__("llmrec_amd.synth", fromlist=["x"]).DATASET_KEYS[CASES["A"]["dataset"]])
    for s, got in enumerate(batches):
        want = S.sampled_batch(data, exist, seed, 4096, aug_rate, s)
        assert len(got[0]) == len(want[0]) >= 4096
        for a, w in zip(got, want):
            assert np.array_equal(a, w), s
    for again in (_sampled_run(monkeypatch, root, graph=True), _sampled_run(monkeypatch, root, graph=False)):
        batches2, snap2, _ = again
        assert all(np.array_equal(a, b) for x, y in zip(batches, batches2) for a, b in zip(x, y))
        assert set(snap) == set(snap2)
        for k in snap:
            assert torch.equal(snap[k], snap2[k]), k


def test_the_default_still_steps_aside_at_4096(monkeypatch):
    from llmrec_amd.fused import FusedStep
    from tests._dropin import golden_argv
    from tests._step_env import fused_trainer
    from tests.conftest import GoldenCase
    g = GoldenCase("nf_tiny")
    argv = golden_argv(g) + ["--batch_size", "4096"]
    assert fused_trainer(monkeypatch, argv, {}, step=True).step is False
    assert fused_trainer(monkeypatch, argv, {"LLMREC_FUSED": "1"}, step=True).step is False
    b = fused_trainer(monkeypatch, argv, {"LLMREC_FUSED": "wide"}, step=True)
    assert isinstance(b.step, FusedStep) and b.step.wide and b.step.b_max > 4096
    small = fused_trainer(monkeypatch, golden_argv(g), {"LLMREC_FUSED": "wide"}, step=True).step     # up to the cap: the same step as "1"
    assert isinstance(small, FusedStep) and not small.wide
