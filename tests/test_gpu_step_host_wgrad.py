"""GPU: the training step with the ID chain's third backward product hosted by the weight-gradient launch (FusedStep.host_wgrad,
llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3; LLMREC_HOST_CHAIN=1, the default) against the same step with LLMREC_HOST_CHAIN=fwd -
the forward's hosted product only, the parent's step: four eager steps and one replayed four-step graph. Every parameter, Adam moment,
gradient buffer and logged scalar `torch.equal`; the hosted step really issued the hosting entry point in place of the plain one, one
SpMM launch fewer and one entry-point call fewer per step.

The model is tests/test_gpu_step_host_chain.py's in its rows - it passes the size rule both hostings share, more 128-row work units in
the projection launch than the device has block slots - and small in bytes: 9 000 users, 1 000 items, 40 000 interactions, d = 64.
Its feature widths are 128 / 256 / 128 instead of 32 / 64 / 128: the hosting kernel is the weight gradient's 128-wide organisation
(every K % 128 == 0), and with a narrower stream the step has no multi-target launch to host in. Two layers (so the chain's backward
has four products: two share groups with the side and profile chains, the third is the hosted one, the fourth follows the weight
gradient), the pre-propagated order forced."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ENTRY = "llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3"
PLAIN = "llmrec_linear_wgrad_multi_adamw_bf16x3"
DATASET = "netflix_valid_item"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from llmrec_amd import synth
    root = str(tmp_path_factory.mktemp("host_wgrad"))
    synth.write_dataset(os.path.join(root, DATASET), 9000, 1000, 40000, seed=11, image_dim=128, text_dim=256, llm_dim=128,
                        keys=synth.DATASET_KEYS[DATASET], max_deg=300)
    return root


def _steps(root, monkeypatch, host, graph):
    from tests._step_env import fused_trainer, snapshot
    from llmrec_amd import _lib
    from llmrec_amd.fused import FusedStep
    env = {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1", "LLMREC_DEVICE_SAMPLER": "1", "LLMREC_PREPROPAGATE": "1", "LLMREC_HOST_CHAIN": host}
    argv = ["--dataset", DATASET, "--data_path", root + "/", "--batch_size", "256", "--seed", "2022", "--debug", "--lr", "0.001",
            "--layers", "2", "--embed_size", "64", "--epoch", "1"]
    _, tr, step, batcher = fused_trainer(monkeypatch, argv, env, train=True, step=True, batcher=True)
    assert step and step.fold and step.inline_adamw and step.preprop and not step.multi_stream and step.L == 2 and step.d == 64
    assert step.host_chain and step.host_wgrad == (host == "1")
    assert sum(-(-j[0].shape[0] // 128) for j in step.projection_jobs()) > step._block_slots          # the size rule holds
    names = []
    if graph:
        step.capture(batcher=batcher, unroll=4)                         # (the capture's warm-up is the first step)
        step.run_steps(4)
        n = 5
    else:
        st = step._make_static()
        invoke = _lib._invoke
        monkeypatch.setattr(_lib, "_invoke", lambda fn, args: (names.append(fn), invoke(fn, args))[1])
        for _ in range(4):
            del names[:]
            step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
        monkeypatch.setattr(_lib, "_invoke", invoke)
        n = 4
    torch.cuda.synchronize()
    assert int(batcher.step_dev) == n
    out = snapshot(tr, step, ("scal", "out", "epoch_sums", "static_block", "dU_cat", "bufU", "bufI"))
    return out, list(names), step.entry_point_calls_per_step


@pytest.mark.parametrize("how", ["eager", "graph_unroll4"])
def test_hosted_steps_equal_the_forward_hosted_steps(dataset, monkeypatch, how):
    graph = how == "graph_unroll4"
    fwd, calls_fwd, per_step_fwd = _steps(dataset, monkeypatch, "fwd", graph)
    hosted, calls_hosted, per_step_hosted = _steps(dataset, monkeypatch, "1", graph)
    assert sorted(hosted) == sorted(fwd) and any(k.startswith("m/") for k in hosted) and any(k.startswith("g/") for k in hosted)
    bad = [k for k in hosted if not torch.equal(hosted[k], fwd[k])]
    assert not bad, bad[:6]
    assert bool(torch.isfinite(hosted["scal"]).all()) and bool((hosted["bufU"] != 0).any())
    assert per_step_hosted == per_step_fwd - 1, (per_step_hosted, per_step_fwd)
    if not graph:
        spmms = lambda calls: sum(c.startswith("llmrec_spmm_") for c in calls)
        print("[host wgrad] calls per step: %d hosted, %d forward-hosted; SpMM launches %d / %d" % (len(calls_hosted), len(calls_fwd),
                                                                                                  spmms(calls_hosted), spmms(calls_fwd)))
        assert calls_hosted.count(ENTRY) == 1 and PLAIN not in calls_hosted
        assert ENTRY not in calls_fwd and calls_fwd.count(PLAIN) == 1
        assert spmms(calls_hosted) == spmms(calls_fwd) - 1 and len(calls_hosted) == len(calls_fwd) - 1
        # the hosted product's successors follow the launch: the chain's last product, then the tail
        k = calls_hosted.index(ENTRY)
        assert calls_hosted[k + 1] == "llmrec_spmm_f32" and calls_fwd[calls_fwd.index(PLAIN) - 1] != "llmrec_spmm_f32", (calls_hosted[k:], calls_fwd)
