"""Step time of the fused step with dropout inside it (profiles/experiments/fused_dropout.md), on bench.py's Netflix-shaped workload, one
GPU, all arms in ONE process, alternating:

  A        FusedStep(drop_rate=p, drop_seed=seed): replayed graphs of four steps, the device sampler inside (bench.py's mode)
  B        FusedStep at rate 0 with LLMREC_PREPROPAGATE=0 - A's organisation without its four dropout launches
  default  FusedStep at rate 0 as bench.py builds it (pre-propagated where the shape says so): what leaving pre-propagation costs
  C        the per-op autograd path with nn.Dropout(p) (what --drop_rate p trains on without LLMREC_FUSED_DROPOUT=1)

    python tools/fused_dropout_probe.py [--p 0.5] [--rounds 5] [--steps 400] [--modular-steps 100] [--out FILE.json]

A window is `steps` steps between two device synchronisations on the host clock; every window is reported, with the median per arm."""
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
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--modular-steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from llmrec_amd.fused import FusedStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    plain_import = bench.import_dropin_models

    def workload(drop: float, preprop):
        """bench.NetflixShaped with --drop_rate `drop` on the drop-in's command line; drop > 0: its step rebuilt with the dropout inside."""
        if preprop is None:
            os.environ.pop("LLMREC_PREPROPAGATE", None)
        else:
            os.environ["LLMREC_PREPROPAGATE"] = preprop
        bench.import_dropin_models = lambda ds, extra=(): plain_import(ds, list(extra) + ["--drop_rate", str(drop)])
        try:
            wl = bench.NetflixShaped("nf", a.seed, dev)
            if drop > 0:
                f, ar = wl.fused, wl.args
                wl.fused = FusedStep(wl.model, wl.graph, wl.hp, (ar.model_cat_rate, ar.user_cat_rate, ar.item_cat_rate), wl.opt, f.b_max,
                                     drop_rate=drop, drop_seed=a.seed)
        finally:
            bench.import_dropin_models = plain_import
            os.environ.pop("LLMREC_PREPROPAGATE", None)
        wl.model.train()
        return wl
    arms = {"A": workload(a.p, None), "B": workload(0.0, "0"), "default": workload(0.0, None), "C": workload(a.p, None)}
    assert arms["A"].fused.drop_rate == a.p and not arms["A"].fused.preprop and not arms["B"].fused.preprop

    def window(name):
        wl = arms[name]
        n = a.modular_steps if name == "C" else a.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "C":
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
    out = {"p": a.p, "steps_per_window": a.steps, "modular_steps_per_window": a.modular_steps, "device": torch.cuda.get_device_name(dev),
           "entry_point_calls": {k: arms[k].fused.entry_point_calls_per_step for k in ("A", "B", "default")},
           "ms_per_step": times, "median_ms_per_step": {k: round(statistics.median(v), 5) for k, v in times.items()},
           "drop_step": int(arms["A"].fused.drop_step.view(torch.int64).cpu()[0])}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
