"""GPU: checkpoint and resume (llmrec_amd/checkpoint.py, main.py's LLMREC_CHECKPOINT / LLMREC_RESUME) on tests/golden/nf_tiny. Everything
is bit-exact - a run stopped and resumed EQUALS the uninterrupted run - so there are no tolerances anywhere in this file.
  * interrupted = uninterrupted on every path that trains: 4 epochs against 2 epochs + a FRESH import and Trainer resumed for 2 more;
  * a rollback into a live captured step (default schedule, LLMREC_CHECK_ZERO=1);
  * best.ckpt holds the best epoch's model: a fresh trainer that loads it re-evaluates to that epoch's logged metrics;
  * request() does not synchronise the host with the device; a second immediate request waits and both files are whole;
  * none of the three variables set: no file, no line, no checkpointer - and checkpointing does not change what is trained."""
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import checkpoint as C
from tests._dropin import golden_argv
from tests._step_env import fused_trainer
from tests.conftest import GoldenCase

BATCH = ["--batch_size", "64"]                                   # nf_tiny has 350 train pairs: 6 steps per epoch
PATHS = {
    # name: (environment, further flags)
    "graph": ({"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1"}, BATCH),                                   # host sampler, packed copy
    "device_sampler": ({"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1", "LLMREC_DEVICE_SAMPLER": "1"}, BATCH),   # the unroll=4 graph
    "modular": ({"LLMREC_FUSED": "0", "LLMREC_GRAPH": "0"}, BATCH),
    "wide": ({"LLMREC_FUSED": "wide"}, ["--batch_size", "4096"]),                                   # tests/test_gpu_step_wide.py's batch
    "dropout": ({"LLMREC_FUSED_DROPOUT": "1"}, BATCH + ["--drop_rate", "0.3"]),
    "mask_users": ({"LLMREC_FUSED": "mask"}, BATCH + ["--mask_rate", "0.1"]),
    "mask_items": ({"LLMREC_FUSED": "mask"}, BATCH + ["--mask", "True", "--mask_rate", "0.1", "--att_re_rate", "0.1"]),
}


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().clone() if t.numel() else torch.zeros(0, dtype=torch.uint8)


def _trainer(monkeypatch, path, epochs, ckpt=None, resume=None, every=None, extra=()):
    env, flags = PATHS[path]
    g = GoldenCase("nf_tiny")
    for k in C.CHECKPOINT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("LLMREC_CHECKPOINT", ckpt), ("LLMREC_RESUME", resume), ("LLMREC_CHECKPOINT_EVERY", every)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    b = fused_trainer(monkeypatch, golden_argv(g) + list(flags) + list(extra) + ["--epoch", str(epochs)], env, seed=g.args["seed"])
    b.m._progress = lambda it: it
    lines, epochs_log = [], []
    b.trainer.logger.logging = lines.append
    b.trainer._on_epoch = lambda ep, loss, mf, emb, ret, times: epochs_log.append(
        (ep, loss, mf, emb, {k: np.asarray(v, dtype=np.float64).tolist() for k, v in ret.items()}))
    return b, lines, epochs_log


def _state(b):
    """Every tensor of state_tensors() of every state owner (parameters, both moments, dev_state, the step's counters, stamps and sums,
    the sampler's counter, the decoder), as bytes on the host; with masking also the masked feature matrices."""
    tr = b.trainer
    torch.cuda.synchronize()
    out = {name: _bits(t) for name, t in tr._checkpointer()._tensors()}
    assert any(k.startswith("adamw/m/") for k in out) and "adamw/dev_state" in out and any(k.startswith("param/") for k in out)
    if tr._fused:
        assert {"step/row_stamp", "step/flag_u", "step/flag_i", "step/epoch_sums"} <= set(out)
        out["E_u"], out["E_i"] = _bits(tr._fused.E_u), _bits(tr._fused.E_i)           # the last evaluation's embeddings
    if tr._fused and tr._fused.mask_rate > 0:
        out["feat/user"] = _bits(tr.model_mm.user_feats)
        for k, x in tr.model_mm.item_feats.items():
            out["feat/item/" + k] = _bits(x)
    return out


def _differences(a, b):
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("path", list(PATHS))
def test_interrupted_equals_uninterrupted(path, monkeypatch, tmp_path):
    a, _, log_a = _trainer(monkeypatch, path, 4)
    a.trainer.train()
    want = _state(a)
    assert [e[0] for e in log_a] == [0, 1, 2, 3]
    if path != "modular":
        from llmrec_amd.fused import FusedStep
        assert isinstance(a.trainer._fused, FusedStep) and a.trainer._fused.wide == (path == "wide")
        assert (a.trainer._fused.drop_rate > 0) == (path == "dropout") and (a.trainer._fused.mask_rate > 0) == path.startswith("mask")
        assert a.trainer._fused.restore == (path == "mask_items")
    del a

    b1, _, log_b1 = _trainer(monkeypatch, path, 2, ckpt=tmp_path)
    b1.trainer.train()
    last = str(tmp_path / "last.ckpt")
    header, _ = C.read_file(last)                                 # in place when train() returns, and whole
    assert header["host"]["epoch"] == 1 and not os.path.exists(last + ".tmp")
    assert log_b1 == log_a[:2]
    del b1

    b2, lines, log_b2 = _trainer(monkeypatch, path, 4, resume=last)        # a FRESH import and Trainer
    b2.trainer.train()
    got = _state(b2)
    assert [e[0] for e in log_b2] == [2, 3]
    assert log_b2 == log_a[2:], "loss / mf / emb and every metric of epochs 2 and 3, exactly"
    bad = _differences(got, want)
    print("[checkpoint %s] %d tensors, %d bytes: %s" % (path, len(want), sum(t.numel() for t in want.values()), "bit-identical" if not bad else bad))
    assert not bad
    if path.startswith("mask"):
        rounds, seconds = b2.trainer._fused.replayed_mask_rounds       # the replay ran, and its bit-for-bit check with it
        assert rounds == header_mask_step(header, last) > 0
        assert any("replayed %d masking rounds" % rounds in s for s in lines)


def header_mask_step(header, path):
    """mask_step as the file holds it."""
    _, arena = C.read_file(path)
    e = next(e for e in header["manifest"] if e["name"] == "step/mask_step")
    return int(np.frombuffer(bytes(arena[e["offset"]:e["offset"] + 8]), dtype=np.int64)[0])


def test_a_masking_checkpoint_loads_into_a_fresh_step_only_and_the_per_op_path_refuses(monkeypatch, tmp_path):
    b, _, _ = _trainer(monkeypatch, "mask_users", 1, ckpt=tmp_path)
    b.trainer.train()
    last = str(tmp_path / "last.ckpt")
    with pytest.raises(RuntimeError, match="mask_step != 0"):      # this step has masked: no rollback in this mode
        b.trainer.load_checkpoint(last)
    del b
    monkeypatch.setitem(PATHS, "per_op_mask", ({"LLMREC_FUSED": "0", "LLMREC_GRAPH": "0"}, BATCH + ["--mask_rate", "0.1"]))
    p, _, _ = _trainer(monkeypatch, "per_op_mask", 1)
    with pytest.raises(RuntimeError, match="need the fused step"):
        p.trainer.save_checkpoint(str(tmp_path / "x.ckpt"))
    assert not os.path.exists(str(tmp_path / "x.ckpt"))


def test_rollback_into_a_live_captured_step(monkeypatch, tmp_path):
    """Capture, 3 steps, save, 3 more steps -> S6; load into the SAME step, the same 3 batches -> S6 again, bit for bit. The default
    schedule (bwd_mask and the row stamps active) under LLMREC_CHECK_ZERO=1."""
    g = GoldenCase("nf_tiny")
    monkeypatch.setitem(PATHS, "live", ({"LLMREC_FUSED": "1", "LLMREC_GRAPH": "1", "LLMREC_CHECK_ZERO": "1"}, []))
    b, _, _ = _trainer(monkeypatch, "live", 1)
    tr = b.trainer
    batch = lambda s: tuple(torch.tensor(g.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))
    for s in range(3):
        tr.train_step(*batch(s))
    step = tr._fused
    assert step.graph_exec is not None and step.check_zero
    graph, ptrs = step.graph_exec, [t.data_ptr() for _, t in step.state_tensors()]
    path = str(tmp_path / "s3.ckpt")
    tr.save_checkpoint(path, note="step 3")
    s3 = _state(b)
    for s in range(3, 6):
        tr.train_step(*batch(s))
    s6 = _state(b)
    assert _differences(s3, s6)
    host = tr.load_checkpoint(path)
    assert host["note"] == "step 3" and host["_global_step"] == 3 == tr._global_step
    assert not [k for k in _differences(_state(b), s3) if not k.startswith("E_")]     # the loaded state equals the saved state exactly (stamps included)
    assert step.graph_exec is graph and [t.data_ptr() for _, t in step.state_tensors()] == ptrs       # nothing was rebound
    for s in range(3, 6):
        tr.train_step(*batch(s))
    bad = _differences(_state(b), s6)
    assert not bad, bad


def test_best_file_holds_the_best_epoch(monkeypatch, tmp_path):
    b, _, log = _trainer(monkeypatch, "graph", 4, ckpt=tmp_path, extra=["--lr", "0.01"])
    b.trainer.train()
    best, best_epoch = 0, None
    for ep, _, _, _, ret in log:                                   # train()'s own rule
        if ret["recall"][1] > best:
            best, best_epoch = ret["recall"][1], ep
    path = str(tmp_path / "best.ckpt")
    if best_epoch is None:
        assert not os.path.exists(path)
        pytest.fail("the recall never rose above 0 in 4 epochs: this case shows nothing")
    header, _ = C.read_file(path)
    assert header["host"]["epoch"] == best_epoch and header["host"]["best_recall"] == best and header["host"]["stopping_step"] == 0
    assert header["host"]["test_ret"]["recall"] == log[best_epoch][4]["recall"]
    del b
    f, _, _ = _trainer(monkeypatch, "graph", 4, extra=["--lr", "0.01"])
    host = f.trainer.load_checkpoint(path)
    assert host["epoch"] == best_epoch
    users = list(f.m.data_generator.test_set.keys())
    ret = f.trainer.test(users, is_val=False)
    again = {k: np.asarray(v, dtype=np.float64).tolist() for k, v in ret.items()}
    assert again == log[best_epoch][4]                             # that epoch's logged metrics, exactly


def test_request_does_not_stall_the_host_and_a_second_request_waits(monkeypatch, tmp_path):
    g = GoldenCase("nf_tiny")
    b, lines, _ = _trainer(monkeypatch, "graph", 1)
    tr = b.trainer
    batch = lambda s: tuple(torch.tensor(g.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))
    tr.train_step(*batch(0))
    ck = tr._checkpointer()
    ck.directory = str(tmp_path)
    ck.save("warm.ckpt", {"k": 0})                                 # allocations (arena, pinned buffer, side stream) happen once, here
    tr.train_step(*batch(1))
    assert ck._idle.is_set()                                       # no write in flight
    torch.cuda.set_sync_debug_mode("error")
    try:
        ck.request("a.ckpt", {"k": 1})                             # raises if anything in it synchronises the host with the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ck.wait()
    state_a = _state(b)
    # the first write of the next pair is held until the second request has found it in flight
    gate, real = threading.Event(), C.write_file
    monkeypatch.setattr(C, "write_file", lambda *a: (gate.wait(), real(*a))[1])
    monkeypatch.setattr(ck, "_on_wait", gate.set)
    waits = ck.stats["waits"]
    ck.request("b.ckpt", {"k": 2})
    tr.train_step(*batch(2))                                       # the state moves on between the two requests
    ck.request("c.ckpt", {"k": 3})
    ck.wait()
    assert ck.stats["waits"] == waits + 1 and any("waited" in s and "c.ckpt" in s for s in lines)
    state_c = _state(b)
    assert _differences(state_a, state_c)

    def file_state(name):
        header, arena = C.read_file(str(tmp_path / name))         # whole: magic, lengths and crc hold
        return header["host"]["k"], {e["name"]: torch.frombuffer(bytearray(arena[e["offset"]:e["offset"] + e["bytes"]]), dtype=torch.uint8)
                                     if e["bytes"] else torch.zeros(0, dtype=torch.uint8) for e in header["manifest"]}
    for name, k, want in (("a.ckpt", 1, state_a), ("b.ckpt", 2, state_a), ("c.ckpt", 3, state_c)):
        got_k, got = file_state(name)
        assert got_k == k
        assert not [n for n in got if not torch.equal(got[n], want[n])], name
    assert open(str(tmp_path / "a.ckpt"), "rb").read() != open(str(tmp_path / "c.ckpt"), "rb").read()
    ck.close()


def test_defaults_write_nothing_and_checkpointing_changes_nothing(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    a, lines, log_a = _trainer(monkeypatch, "graph", 1)
    a.trainer.train()
    assert getattr(a.trainer, "_ckpt", None) is None               # nothing of the feature was even built
    assert os.listdir(str(tmp_path)) == []
    assert not [s for s in lines if "checkpoint" in s.lower()]
    kinds = ("PID: ", "Namespace(", "Epoch 0 [", "Test_Recall@", "#####Early stopping steps", "{'precision'", "None")
    assert all(s.startswith(kinds) for s in lines), lines           # the reference's lines and no other
    want, n_lines = _state(a), len(lines)
    del a
    b, lines_b, log_b = _trainer(monkeypatch, "graph", 1, ckpt=tmp_path / "ck", every=1)
    b.trainer.train()
    assert log_b == log_a and not _differences(_state(b), want)
    assert sorted(os.listdir(str(tmp_path / "ck"))) in (["best.ckpt", "last.ckpt"], ["last.ckpt"])
    assert len([s for s in lines_b if "checkpoint" not in s]) == n_lines
