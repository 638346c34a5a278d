"""GPU: the training step's launch schedule, entry for entry.

One eager training step is recorded as the ordered list of what the host issued:
  ["call", stream, entry point, n]   every call into the library (n = the leading problem count of a grouped entry point, else null),
  ["record", stream, k]              torch.cuda.Event.record (k = the ordinal of this record within the step),
  ["wait_event", stream, k]          torch.cuda.Stream.wait_event (k = the record it waits for; null = not recorded in this step),
  ["wait_stream", waiting, waited]   torch.cuda.Stream.wait_stream,
with stream in main / s1 / s2 / s3 / other. Launches + synchronisation are the whole dependency structure of the eager step and with it
the capture order of the step's graph. tests/step_schedule_expected.json holds the lists of the commit that introduced this test (the two
device_sampler variants: of the parent of the commit that added them, which then restructured FusedStep without moving a launch); a
change of FusedStep's schedule shows up as an exact difference (LLMREC_STEP_SCHEDULE_WRITE=<file> writes the recorded lists there
instead of comparing - for a change that MEANS to move the schedule)."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._dropin import golden_argv
from tests._step_env import fused_trainer, set_switches
from tests.conftest import GoldenCase

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_schedule_expected.json")
WRITE_TO = os.environ.get("LLMREC_STEP_SCHEDULE_WRITE")
GROUPED = re.compile(r"llmrec_(spmm_multi(_guest)?_f32|fuse_\w+_multi\w*|bpr_multi_\w+|linear_\w+_(grouped|multi)\w*)$")
VARIANTS = {
    "default": {},
    "streams": {"LLMREC_STREAMS": "1"},
    "unfolded": {"LLMREC_FOLD": "0"},
    "unfolded_streams": {"LLMREC_FOLD": "0", "LLMREC_STREAMS": "1"},
    "reference_order": {"LLMREC_PREPROPAGATE": "0"},
    "f32": {"LLMREC_GEMM": "f32"},
    "dense_wgrad": {"LLMREC_WGRAD_ROWS": "0"},
    "data_parallel": {},
    "device_sampler": {"LLMREC_DEVICE_SAMPLER": "1"},                 # the sampler, the plan + reach marks and the loss values ride SpMM launches
    "device_sampler_refused": {"LLMREC_DEVICE_SAMPLER": "1"},         # ... with every guest launch refused: the next rungs of the ladder
}


class Recorder:
    """Installed with monkeypatch around ONE step; `step` gives the streams' names."""

    def __init__(self, monkeypatch, step):
        from llmrec_amd import _lib
        self.log, self.events, self.quiet = [], [], False
        names = [(torch.cuda.current_stream(), "main"), (step.s1, "s1"), (step.s2, "s2"), (step.s3, "s3")]
        name = lambda st: next((n for s, n in names if s == st), "other")
        invoke, record = _lib._invoke, torch.cuda.Event.record
        wait_event, wait_stream = torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def ordinal(ev):
            return next((k for k in range(len(self.events) - 1, -1, -1) if self.events[k] is ev), None)

        def _invoke(fn, args):
            self.log.append(["call", name(torch.cuda.current_stream()), fn, int(args[0]) if GROUPED.match(fn) else None])
            return invoke(fn, args)

        def _record(ev, stream=None):
            if not self.quiet:
                self.events.append(ev)                       # (kept alive: an ordinal names one event)
                self.log.append(["record", name(stream if stream is not None else torch.cuda.current_stream()), len(self.events) - 1])
            return record(ev, stream)

        def _wait_event(st, ev):
            if not self.quiet:
                self.log.append(["wait_event", name(st), ordinal(ev)])
            return wait_event(st, ev)

        def _wait_stream(st, other):                         # (torch implements it as record + wait_event: one entry, not three)
            self.log.append(["wait_stream", name(st), name(other)])
            self.quiet = True
            try:
                return wait_stream(st, other)
            finally:
                self.quiet = False
        monkeypatch.setattr(_lib, "_invoke", _invoke)
        monkeypatch.setattr(torch.cuda.Event, "record", _record)
        monkeypatch.setattr(torch.cuda.Stream, "wait_event", _wait_event)
        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", _wait_stream)


def _batch(golden, s):
    return tuple(torch.tensor(golden.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))


def _record_second_step(golden, variant, monkeypatch):
    """(recorded list, the step object) of the SECOND training step: the first one sizes the row-listed weight gradient (one read-back)."""
    env = dict(VARIANTS[variant], LLMREC_FUSED="1", LLMREC_GRAPH="0")
    if variant == "data_parallel":
        set_switches(monkeypatch, env)
        # DataParallelStep on the same model, one replica, no communicator: _backward with bpr_bwd_done=False and inline_adamw=False
        from llmrec_amd.dp import DataParallelStep
        from tests.test_gpu_step import _dp_replica
        b_max = max(golden.z["step%d/users" % s].size for s in range(2)) + 3
        _, step = _dp_replica(golden, DataParallelStep, b_max, comm=None, rank=0, world=1)

        def run(s):
            u, p, n = _batch(golden, s)
            pad = torch.zeros(b_max - u.numel(), dtype=torch.int64, device="cuda")
            n_valid = torch.tensor([u.numel()], dtype=torch.int32, device="cuda")
            step.step_eager(torch.cat([u, pad]), torch.cat([p, pad]), torch.cat([n, pad]), n_valid)
    else:
        _, tr, step, _ = fused_trainer(monkeypatch, golden_argv(golden), env, seed=golden.args["seed"], step=True)
        assert step, "the golden configuration runs the fused step"
        run = lambda s: tr.train_step(*_batch(golden, s))
        if variant.startswith("device_sampler"):
            # the step the benchmark times: the batch is sampled on the device, inside the step (tests/test_gpu_spmm_guests.py drives it so)
            from llmrec_amd.fused import FusedStep
            tr.model_mm.train()
            batcher, st = tr._device_batcher(), step._make_static()
            step._refuse_guests = variant == "device_sampler_refused"
            run = lambda s: step.step_eager(st["users"], st["pos"], st["neg"], st["n_valid"], sampler=FusedStep.sampler_of(batcher, st))
    run(0)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        rec = Recorder(mp, step)
        run(1)
    torch.cuda.synchronize()
    return rec.log, step


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["nf_tiny", "ml_tiny"])        # d = 64, one layer: grouped SpMMs accepted; d = 16, two layers: refused, separate launches
def test_step_schedule_is_the_recorded_one(case, variant, monkeypatch):
    assert torch.cuda.is_available()
    got, step = _record_second_step(GoldenCase(case), variant, monkeypatch)
    key = "%s/%s" % (case, variant)
    print("[schedule %s] %d entries, %d calls" % (key, len(got), sum(e[0] == "call" for e in got)))
    if key == "nf_tiny/default":
        assert sum(e[0] == "call" for e in got) == step.entry_point_calls_per_step
    if WRITE_TO:
        table = json.load(open(WRITE_TO)) if os.path.exists(WRITE_TO) else {}
        table[key] = got
        with open(WRITE_TO, "w") as f:
            f.write("{\n" + ",\n".join('%s: [\n  %s\n]' % (json.dumps(k), ",\n  ".join(json.dumps(e) for e in table[k])) for k in sorted(table)) + "\n}\n")
        return
    want = json.load(open(EXPECTED))[key]
    diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert got == want, (key, len(got), len(want), diff[:4])
