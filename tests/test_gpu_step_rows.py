"""GPU: whole training steps against the float64 oracle, ROW BY ROW (the yardstick: tests/_step_ref.py, shown to be neither blind nor too
tight by tests/test_step_ref_cpu.py). Three consecutive steps per case and path. Per step the device's parameters and moments are
snapshot, the step runs, its forward outputs (FusedStep.outputs()), the 8 (mf, emb) pairs, the loss, every .grad and the parameters
and moments are snapshot again, and the oracle step is evaluated twice - fp64 and fp32 - from the DEVICE's own pre-step parameters and
the step's actual batch: nothing is amplified along a trajectory. Every row of every forward tensor and gradient goes through
row_check, the 17 scalars through scalar_check, every element of the ten parameters and twenty moments through the AdamW bound of
tests/_rowops_ref.adamw fed with the device's own gradient. No row, element or step is excluded.

  A  hosted, everything on: tests/test_gpu_step_host_wgrad.py's shape (9000 x 1000 x 40 000, widths 128 / 256 / 128, d 64, two layers,
     batch 256, the pre-propagated order forced) - eager with the device sampler, graph with the in-graph sampler (capture(unroll=1),
     single replays), LLMREC_STREAMS=1.
  B  islands, the generic kernels, exact zeros: 3000 x 800 x ~12 000 in four disjoint blocks, the MovieLens keys, three layers, widths
     48 / 200 / 72 (nothing hosted, ragged K), an injected batch of 408 triples from ONE block with n_valid < b_max, a user 9 times, an
     item that is positive and negative - eager, a graph captured without a sampler, LLMREC_GEMM=f32.
  C  B's graph, a batch of 4608 > LLMREC_BPR_MAX_B: the modular path with the multi-block prune selection (576 distinct triples 8 times
     each: ties everywhere but across the cut).
Inputs (tests/_step_ref.py says why): the image / text features of the generated datasets are scaled by 1/8 - at the generator's scale
more than 71 % of those problems' samples saturate and no cut has a gap -, A's --seed is one of the few whose sampled batches satisfy the
cut-gap condition in all eight problems and three steps, and the triples of B and C are chosen from the fp64 forward of the initial
parameters so that every problem's maxi values fall into two groups with the cut between them.

CONDITIONS asserted at run time (a violation fails, nothing skips): in every step and problem the fp64 maxi values on either side of the
prune cut are at least 64 fp32-oracle errors apart (else fp32 and fp64 may legitimately keep different samples; the CPU test holds the
oracle's own trajectory to twice that); case B's table gradients have >= 50 % exactly-zero and >= 10 % non-zero rows.

MARGINS. M is a measurement: the worst err_r(got) / y_r per family on the MI355X (the step is bitwise reproducible, so these are
constants), times four for another compiler's contraction choices, rounded up to a power of two; none may exceed 256. Measured, worst
over the three steps (per tensor: profiles/experiments/step_rows.md; eager, graph and four streams agree to every digit):
                                   A (eager = graph = streams)   B (eager = graph)   B f32    C      x 4 -> M
  forward outputs                  2.61  (txt_u)                 2.22                2.82     1.71   11.3 -> 16
  table gradients                  1.99  (item table)            1.36                1.54     1.18   7.96 -> 8
  Linear gradients                 1.19                          2.04                2.07     1.74   8.28 -> 16
  scalars (16 BPR values, loss)    1.48                          2.79                1.70     1.59   11.2 -> 16
  AdamW, worst |err| / bound       0.50                          0.49                0.49     0.48   (the derivation's bound, no margin)
  smallest cut gap / (64 err)      2.13                          5.16                5.11     4.28
"""
import numpy as np
import pytest
import torch

from tests import _rowops_ref as RR
from tests import _step_ref as S

pytestmark = pytest.mark.gpu

M = dict(forward=16, table=8, linear=16, scalar=16)
assert max(M.values()) <= S.M_MAX

SAMPLER = {"LLMREC_FUSED": "1", "LLMREC_DEVICE_SAMPLER": "1", "LLMREC_PREPROPAGATE": "1"}
PATHS = {
    ("A", "eager"): dict(SAMPLER, LLMREC_GRAPH="0"),
    ("A", "graph"): dict(SAMPLER, LLMREC_GRAPH="1"),
    ("A", "streams"): dict(SAMPLER, LLMREC_GRAPH="0", LLMREC_STREAMS="1"),
    ("B", "eager"): {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "0"},
    ("B", "graph"): {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1"},
    ("B", "f32"): {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "0", "LLMREC_GEMM": "f32"},
    ("C", "default"): {},
}
CASES = {"A": S.CASE_A, "B": S.CASE_B, "C": S.CASE_C}


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """case -> data root; B and C share one dataset. The oracle's inputs are loaded once per root."""
    roots, loaded = {}, {}

    def get(name, args):
        key = "B" if name == "C" else name
        if key not in roots:
            roots[key] = str(tmp_path_factory.mktemp("step_rows_" + key))
            S.write_case(CASES[key], roots[key])
        return roots[key]

    def inputs(name, args):
        root = get(name, None)
        if root not in loaded:
            loaded[root] = S.oracle_inputs(CASES[name], root, args)
        data, _, graphs = loaded[root]
        return data, S.O.Config.from_args(vars(args), data.keys), graphs
    get.inputs = inputs
    return get


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _forward_of(out, keys):
    fwd = {k: _np(v) for k, v in dict(E_u=out[0], E_i=out[1], img_i=out[2], txt_i=out[3], img_u=out[4], txt_u=out[5], P_usr=out[6],
                                      prof_u=out[8], prof_i=out[9]).items()}
    for k in keys:
        fwd["att_u/" + k], fwd["att_i/" + k] = _np(out[10][k]), _np(out[11][k])
    return fwd


def _drive(name, path, b, case, data, graphs, cfg):
    """-> run(s): runs step s on the device and returns (batch as numpy arrays, {"fwd", "bpr", "loss"}) of it"""
    from llmrec_amd.fused import FusedStep
    tr, step, batcher = b.trainer, b.step, b.batcher
    keys = data.keys
    dev = torch.device("cuda")
    if name != "A":
        sd = tr.model_mm.state_dict()
        islands = S.island_batches(case, data, graphs, cfg, {k: sd[k].detach().cpu() for k in S.PARAMS})

    def fused_result():
        torch.cuda.synchronize()
        return {"fwd": _forward_of(step.outputs(), keys), "bpr": _np(step.out[:step.n_prob]).reshape(S.N_PROB, 2), "loss": float(step.scal[1])}

    if name == "A":
        assert step and step.host_chain and step.host_wgrad and step.fold and step.inline_adamw and step.bwd_mask and step.preprop
        assert step.multi_stream == (path == "streams")
        static = {}

        def run(s):
            if path == "graph":
                if s == 0:
                    step.capture(batcher=batcher, unroll=1)                      # the capture's warm-up is the first step
                else:
                    step.step()
                st = step.static
            else:
                st = static.setdefault("st", step._make_static())
                step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
            res = fused_result()
            assert int(batcher.step_dev) == s + 1
            nv = int(st["n_valid"])
            return tuple(st[k][:nv].cpu().numpy() for k in ("users", "pos", "neg")), res
        return run
    if name == "B":
        assert step and not step.preprop and not step.wgrad_rows and step.L == 3 and step.gemm == ("f32" if path == "f32" else "bf16x3")

        def run(s):
            batch = islands[s]
            assert len(batch[0]) < step.b_max
            tr.train_step(*(torch.from_numpy(t).to(dev) for t in batch))
            assert (step.graph_exec is not None) == (path == "graph")
            if path == "graph":
                assert int(step.static["n_valid"]) == len(batch[0]) < step.b_max
            return batch, fused_result()
        return run
    from llmrec_amd import _lib
    assert step is False and tr.batch_size + int(tr.batch_size * tr.hyper.aug_sample_rate) > _lib.CONST["LLMREC_BPR_MAX_B"]
    log = []
    tr._on_bpr = lambda mf, emb: log.append((float(mf), float(emb)))

    def run(s):
        batch = islands[s]
        assert len(batch[0]) == 4608 > _lib.CONST["LLMREC_BPR_MAX_B"]
        tr.model_mm.train()
        with torch.no_grad():
            out = tr.model_mm(tr.ui_graph, tr.iu_graph, tr.image_ui_graph, tr.image_iu_graph, tr.text_ui_graph, tr.text_iu_graph)
        fwd = _forward_of(out, keys)
        del log[:]
        loss, _, _ = tr.train_step(*(torch.from_numpy(t).to(dev) for t in batch))
        torch.cuda.synchronize()
        assert len(log) == S.N_PROB
        return batch, {"fwd": fwd, "bpr": np.array(log, dtype=np.float64), "loss": float(loss)}
    return run


@pytest.mark.parametrize("name,path", list(PATHS), ids=["%s-%s" % k for k in PATHS])
def test_three_steps_row_by_row(datasets, monkeypatch, name, path):
    from tests._step_env import fused_trainer, snapshot
    case = CASES[name]
    root = datasets(name, None)
    b = fused_trainer(monkeypatch, S.case_argv(case, root), PATHS[(name, path)], train=True, step=True, batcher=(name == "A"))
    data, cfg, graphs = datasets.inputs(name, b.m.args)
    lr = float(b.m.args.lr)
    assert lr == 1e-3 and cfg.n_layers == (2 if name == "A" else 3) and tuple(cfg.keys) == tuple(data.keys)
    run = _drive(name, path, b, case, data, graphs, cfg)
    folded = bool(b.step and b.step.fold)
    fails, worst, worst_adamw, gaps_min = [], {}, {}, np.inf
    for s in range(S.STEPS):
        pre = snapshot(b.trainer, None, grads=False, cpu=True)
        batch, got = run(s)
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
        if name != "A":                                                           # the islands: exact zeros in both tables' gradients
            for tab in S.TABLES:
                share = float((np.abs(r64["grad"][tab]).max(axis=1) > 0).mean())
                assert (0.10 if name == "B" else 0.0) < share <= 0.50, (tab, share)
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
    tag = "[step rows] %s-%s" % (name, path)
    for k in sorted(worst):
        print("%s ratio %-28s %.3g" % (tag, k, worst[k]))
    print("%s families %s; AdamW worst |err| / bound %s; smallest cut gap / (64 err) %.3g"
          % (tag, {k: "%.3g" % v for k, v in sorted(by_family.items())}, {k: "%.3g" % v for k, v in sorted(worst_adamw.items())}, gaps_min))
    assert not fails, "\n".join(fails[:12])
