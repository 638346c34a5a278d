"""GPU: the training step with the ID chain's first product hosted by the projection launch (FusedStep.host_chain,
llmrec_linear_fwd_grouped_host_spmm_bf16x3) against the same step with LLMREC_HOST_CHAIN=0: four eager steps and one replayed four-step
graph. Every parameter, Adam moment, gradient buffer and logged scalar `torch.equal`, and the hosted step really issued the hosting entry
point and one SpMM group fewer.

The model passes the size rule of hosting - more 128-row work units in the projection launch than the device has block slots - and is small
in bytes: 9 000 users, 1 000 items, 40 000 interactions, feature widths 32 / 64 / 128, d = 64, two layers, the pre-propagated order forced
(the projections then run over the users: 8 x 71 = 568 units against 2 x 256 slots)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ENTRY = "llmrec_linear_fwd_grouped_host_spmm_bf16x3"
DATASET = "netflix_valid_item"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from llmrec_amd import synth
    root = str(tmp_path_factory.mktemp("host_chain"))
    synth.write_dataset(os.path.join(root, DATASET), 9000, 1000, 40000, seed=11, image_dim=32, text_dim=64, llm_dim=128,
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
    assert step and step.fold and step.preprop and not step.multi_stream and step.L == 2 and step.d == 64
    assert step.host_chain == (host == "1")
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
    out = snapshot(tr, step, ("scal", "out", "epoch_sums", "static_block", "dU_cat"))
    out["U_1"] = step.Ul[0].clone()
    return out, list(names)


@pytest.mark.parametrize("how", ["eager", "graph_unroll4"])
def test_hosted_steps_equal_unhosted_steps(dataset, monkeypatch, how):
    graph = how == "graph_unroll4"
    plain, calls_plain = _steps(dataset, monkeypatch, "0", graph)
    hosted, calls_hosted = _steps(dataset, monkeypatch, "1", graph)
    assert sorted(hosted) == sorted(plain) and any(k.startswith("m/") for k in hosted) and any(k.startswith("g/") for k in hosted)
    bad = [k for k in hosted if not torch.equal(hosted[k], plain[k])]
    assert not bad, bad[:6]
    assert bool(torch.isfinite(hosted["scal"]).all()) and bool((hosted["U_1"] != 0).any())
    if not graph:
        groups = lambda calls: sum(c.startswith("llmrec_spmm_") for c in calls)
        print("[host chain] calls per step: %d hosted, %d plain; SpMM launches %d / %d" % (len(calls_hosted), len(calls_plain), groups(calls_hosted),
                                                                                          groups(calls_plain)))
        assert calls_hosted.count(ENTRY) == 1 and "llmrec_linear_fwd_grouped_bf16x3" not in calls_hosted
        assert ENTRY not in calls_plain and calls_plain.count("llmrec_linear_fwd_grouped_bf16x3") == 1
        assert groups(calls_hosted) == groups(calls_plain) - 1 and len(calls_hosted) == len(calls_plain) - 1
