"""Times what lifting the 4096-sample batch cap costs: the wide BPR + prune forward (llmrec_bpr_prune_fwd_wide_f32) at growing batch sizes next
to the capped llmrec_bpr_prune_fwd_f32 at 4096 from the same process, and a single-rank ShardedFusedID step at three batch sizes on a synthetic
graph (default: cfg 4's size, 10 M x 1 M x 200 M edges, on one device). Run by hand on the GPU:  python tools/bpr_wide_probe.py [--out profiles/experiments/bpr_wide.md] [--users N --items N --edges N]
Without --part the script is a driver: each part runs in a child process of its own under its own time limit, and a part that fails or runs out
of time ends the run (nothing more is started on the device). --part fwd | step: that part alone, one JSON line on stdout.
Times are HIP events around REPS back-to-back calls after WARM warm-up calls (eager launches, no graph): launch overheads are in them."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [4096, 16384, 65536, 262144, 1048576]
STEP_BATCHES = [1024, 8192, 65536]
D, REMEMBER, WARM, REPS = 64, 0.29, 5, 50
LIMITS = {"fwd": 240, "step": 400}                                      # seconds per part


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _ms(fn, warm=WARM, reps=REPS):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def part_fwd():
    """per size: the whole local forward; its scores launch alone (scores_only = 1); selection + reduction alone (the pass-2 form against
    the batch's own list); write + reduction alone (the same with remember = 1: no threshold to find, the histogram passes are skipped)."""
    import numpy as np
    import torch
    from llmrec_amd import ops
    rng = np.random.default_rng(0)
    U, I = 200_000, 100_000
    Eu = torch.from_numpy((rng.standard_normal((U, D)) * 0.3).astype(np.float32)).cuda()
    Ei = torch.from_numpy((rng.standard_normal((I, D)) * 0.3).astype(np.float32)).cuda()
    rows = []
    for B in SIZES:
        idx = [torch.from_numpy(rng.integers(0, n, size=B)).cuda() for n in (U, I, I)]
        out = torch.zeros(2, device="cuda"); saved = torch.zeros(ops.bpr_saved_floats(B), device="cuda")
        ws = ops.bpr_wide_workspace(B, "cuda")
        head = (ops._p(Eu), ops._ld(Eu), ops._p(Ei), ops._ld(Ei), D, ops._p(idx[0]), ops._p(idx[1]), ops._p(idx[2]), B)

        def wide(remember, global_m, scores_only):
            ops._lib.call("llmrec_bpr_prune_fwd_wide_f32", *head, remember, 1e-5, 1024.0, ops._p(global_m), 0 if global_m is None else B, 0,
                          scores_only, ops._p(out), ops._p(saved), None, ops._p(ws), ws.numel(), ops._stream())

        r = {"B": B, "wide_ms": _ms(lambda: wide(REMEMBER, None, 0)), "scores_ms": _ms(lambda: wide(REMEMBER, None, 1))}
        wide(REMEMBER, None, 1)
        m = saved[B + 4:2 * B + 4].clone()
        r["select_reduce_ms"] = _ms(lambda: (wide(REMEMBER, None, 1), wide(REMEMBER, m, 0))) - r["scores_ms"]   # (pass 2 consumes the sg slots: scores again)
        r["write_reduce_ms"] = _ms(lambda: (wide(1.0, None, 1), wide(1.0, m, 0))) - r["scores_ms"]
        wide(REMEMBER, None, 0)
        r["kept"] = int((saved[:B] != 0).sum()); r["k"] = int(REMEMBER * B)
        if B <= ops.CONST["LLMREC_BPR_MAX_B"]:
            r["capped_ms"] = _ms(lambda: ops._lib.call("llmrec_bpr_prune_fwd_f32", *head, None, REMEMBER, 1e-5, 1024.0, ops._p(out), ops._p(saved),
                                                       ops._stream()))
        rows.append(r)
    return {"d": D, "remember": REMEMBER, "warm": WARM, "reps": REPS, "rows": rows}


def part_step():
    import torch
    from llmrec_amd import dist as ld, synth
    from llmrec_amd.dist_fused import ShardedFusedID
    n_users, n_items, n_edges = _arg("--users", 10_000_000), _arg("--items", 1_000_000), _arg("--edges", 200_000_000)
    t0 = time.perf_counter()
    rows, cols = synth.bipartite_edges_device(n_users, n_items, n_edges, 7, "cuda")
    comm, be = ld.Comm(single=True), ld.HipBackend()
    g = ld.ShardedGraph.build(rows, cols, n_users, n_items, 0, comm, be)
    del rows, cols
    torch.cuda.synchronize()
    res = {"n_users": n_users, "n_items": n_items, "n_edges": n_edges, "d": D, "layers": 2, "build_s": time.perf_counter() - t0, "rows": []}
    for B in STEP_BATCHES:
        # the dense forward: the restricted forward's one-block id sort takes world * 2 * batch_local <= 32768 ids
        st = ShardedFusedID(g, comm, be, D, 2, n_users, seed=1, lr=1e-4, batch_local=B, drop_rate=1 - REMEMBER, decay=1e-5, sparse_forward=False)
        ms = _ms(lambda: st.step(), warm=3, reps=10)                      # the device sampler's batches
        res["rows"].append({"batch_local": B, "step_ms": ms, "edges_per_s": B / ms * 1e3})
        del st
        torch.cuda.empty_cache()
    return res


def _markdown(res):
    f, s = res["fwd"], res["step"]
    out = ["# Wide BPR + prune forward and the row-sharded step beyond 4096 samples (`tools/bpr_wide_probe.py`)", "",
           "MI355X, one device. HIP events around %d back-to-back eager calls after %d warm-up calls; d = %d, remember = %.2f (k = 0.29 B)."
           % (f["reps"], f["warm"], f["d"], f["remember"]),
           "`scores`: the scores launch alone (`scores_only = 1`). `select + reduce`: the pass-2 form against the batch's own list, i.e. init, four",
           "histogram passes, count, write and the one-block `bpr_reduce_kernel`; `write + reduce`: the same with remember = 1, where the passes are",
           "skipped - the difference is the radix select. The last two are differences of two timed sequences (each re-runs the scores launch).", "",
           "| B | wide forward ms | scores ms | select + reduce ms | write + reduce ms | `llmrec_bpr_prune_fwd_f32` ms |", "|---|---|---|---|---|---|"]
    for r in f["rows"]:
        out.append("| %d | %.4f | %.4f | %.4f | %.4f | %s |" % (r["B"], r["wide_ms"], r["scores_ms"], r["select_reduce_ms"], r["write_reduce_ms"],
                                                               "%.4f" % r["capped_ms"] if "capped_ms" in r else "refused (> 4096)"))
    out += ["", "`ShardedFusedID`, one rank, two layers, dense forward (`sparse_forward=False`), device sampler, on a synthetic graph of %d users x %d items"
            % (s["n_users"], s["n_items"]),
            "with %d edges (`synth.bipartite_edges_device`, one seed, built with its CSRs in %.1f s). Not bench.py's cfg-4 line (16 per-block graphs over 8 ranks). 3 warm-up + 10 timed steps."
            % (s["n_edges"], s["build_s"]), "", "| batch_local | step ms | BPR edges/s |", "|---|---|---|"]
    for r in s["rows"]:
        out.append("| %d | %.2f | %.0f |" % (r["batch_local"], r["step_ms"], r["edges_per_s"]))
    return "\n".join(out) + "\n"


def main():
    if "--part" in sys.argv:
        part = sys.argv[sys.argv.index("--part") + 1]
        print(json.dumps({"fwd": part_fwd, "step": part_step}[part]()))
        return
    out = _arg("--out", "")
    passed = [a for k in ("--users", "--items", "--edges") if k in sys.argv for a in (k, sys.argv[sys.argv.index(k) + 1])]
    res = {}
    for part in ("fwd", "step"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part] + passed, capture_output=True, text=True, timeout=LIMITS[part])
        except subprocess.TimeoutExpired:
            sys.exit("bpr_wide_probe: part %s exceeded %d s - stopping" % (part, LIMITS[part]))
        if p.returncode != 0:
            sys.exit("bpr_wide_probe: part %s ended with status %d - stopping\n%s" % (part, p.returncode, p.stderr[-3000:]))
        res[part] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps({part: res[part]}), flush=True)
    text = _markdown(res)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
