"""Step time of the fused step on its WIDE loss segment (profiles/experiments/fused_wide.md), on bench.py's Netflix-shaped workload, one
GPU, all arms in ONE process, alternating:

  capped_1024   FusedStep at --batch_size 1024 as bench.py builds it (the capped loss segment)
  wide_1024     the same step with FusedStep.WIDE_FROM = 0: what the wide segment's extra launches cost against the step itself
  wide_<B>      FusedStep at --batch_size B (8192, 32768; what LLMREC_FUSED=wide trains on): replayed graphs of four steps, the device
                sampler inside (bench.py's mode)
  modular_<B>   the per-op autograd path at the same batch (what the drop-in trains on above 4096 without LLMREC_FUSED=wide)

    python tools/fused_wide_probe.py [--batches 8192,32768] [--rounds 5] [--steps 200] [--modular-steps 30] [--out FILE.json]

A window is `steps` steps between two device synchronisations on the host clock; every window is reported, with the median per arm,
edges/s = batch_size / step time (the reference's timer counts batch_size per step) and the longest run of the last step's scatter plan
(bpr_bwd_runs_kernel gives one 16-lane group to a destination row: a popular item is one serial run)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8192,32768")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--modular-steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from llmrec_amd import _lib
    from llmrec_amd.fused import FusedStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    plain_import = bench.import_dropin_models
    cap = _lib.CONST["LLMREC_BPR_MAX_B"]

    def workload(batch: int, wide_from=None):
        """bench.NetflixShaped with --batch_size `batch` on the drop-in's command line (wide_from: FusedStep.WIDE_FROM while it is built)"""
        bench.import_dropin_models = lambda ds, extra=(): plain_import(ds, list(extra) + ["--batch_size", str(batch)])
        old = FusedStep.WIDE_FROM
        try:
            if wide_from is not None:
                FusedStep.WIDE_FROM = wide_from
            wl = bench.NetflixShaped("nf", a.seed, dev)
        finally:
            bench.import_dropin_models = plain_import
            FusedStep.WIDE_FROM = old
        wl.model.train()
        return wl
    batches = [int(b) for b in a.batches.split(",") if b]
    arms = {"capped_1024": workload(1024), "wide_1024": workload(1024, 0)}
    for b in batches:
        arms["wide_%d" % b] = workload(b)
        arms["modular_%d" % b] = workload(b)
    assert not arms["capped_1024"].fused.wide and arms["wide_1024"].fused.wide
    assert all(arms["wide_%d" % b].fused.wide == (arms["wide_%d" % b].fused.b_max > cap) for b in batches)

    def window(name):
        wl = arms[name]
        modular = name.startswith("modular")
        n = a.modular_steps if modular else a.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if modular:
            for _ in range(n):
                wl.step_modular()
        else:
            wl.run_steps(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    for name in arms:                                                     # warm-up: captures, plan caches, autograd's first steps
        window(name)
    times = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name in arms:
            times[name].append(round(window(name), 5))
    median = {k: round(statistics.median(v), 5) for k, v in times.items()}

    def longest_run(wl):
        f = wl.fused
        runlen = f.bpr_plan[3 * f.b_max:].view(torch.int32)[:3 * f.b_max]
        return {"user_side": int(runlen[:f.b_max].max()), "item_side": int(runlen[f.b_max:].max()), "n_valid": int(f.static["n_valid"])}
    fused_arms = [k for k in arms if not k.startswith("modular")]
    out = {"steps_per_window": a.steps, "modular_steps_per_window": a.modular_steps, "device": torch.cuda.get_device_name(dev),
           "b_max": {k: arms[k].fused.b_max for k in fused_arms},
           "entry_point_calls": {k: arms[k].fused.entry_point_calls_per_step for k in fused_arms},
           "ms_per_step": times, "median_ms_per_step": median,
           "edges_per_s": {k: round(arms[k].hp.batch_size / median[k] * 1e3, 1) for k in arms},
           "longest_run": {k: longest_run(arms[k]) for k in fused_arms}}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
