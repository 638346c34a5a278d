"""Measures the bytes-per-gathered-row lever of the SpMM: fp32 rows against bf16 rows (llmrec_spmm_xbf16_f32), on one box
in one session. Run by hand on the GPU:  python tools/spmm_bf16_probe.py [--out profiles/experiments/spmm_bf16_rows.md]
Parts, each in a child process of its own under its own time limit; a part that fails or runs out of time ends the run (nothing more is
started on the device). --part NAME runs that part alone and prints one JSON line.
  kernel      both products of a 2 M x 1 M x 40 M-edge graph (rows = users gathering item rows, rows = items gathering user rows) at d = 64
              and 128: llmrec_spmm_f32, llmrec_spmm_xbf16_f32 without and with the Yb shadow, and the conversion pass llmrec_rows_to_bf16
              over the gathered table. One HIP-event pair per call, WARM warm-up calls, then REPS rounds that ALTERNATE the variants;
              median (min .. max). The bf16 result is compared bit for bit with the fp32 kernel on the widened operand at this size.
  bench_fp32  `python bench.py --gpus 1 --workload cfg4` (the one-rank cfg-4-shaped ShardedFusedID step, unchanged bench.py) ...
  bench_bf16  ... and the same command with LLMREC_GATHER_DTYPE=bf16
  loss        two ShardedFusedID objects (fp32 / bf16) over one cfg-4-shaped one-rank graph, same seed, the device sampler's same
              LOSS_STEPS batches: the losses side by side, and the memory the mode adds."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USERS, ITEMS, EDGES = 2_000_000, 1_000_000, 40_000_000
WIDTHS = (64, 128)
WARM, REPS = 5, 25
LOSS_STEPS = 60
BENCH = ["bench.py", "--gpus", "1", "--workload", "cfg4", "--steps", "20", "--warmup", "3"]
LIMITS = {"kernel": 300, "bench_fp32": 420, "bench_bf16": 420, "loss": 300}            # seconds per part


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _alternate(fns, warm=WARM, reps=REPS):
    """{name: [ms per call]}: `reps` rounds, each running every variant once, one event pair per call"""
    import torch
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, fn in fns.items():
            evs[k][r][0].record(); fn(); evs[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def _stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def part_kernel():
    import torch
    from llmrec_amd import ops, synth
    users, items, edges = _arg("--users", USERS), _arg("--items", ITEMS), _arg("--edges", EDGES)
    r, c = synth.bipartite_edges_device(users, items, edges, 7, "cuda")
    res = {"users": users, "items": items, "edges": int(r.numel()), "warm": WARM, "reps": REPS, "rows": []}
    operands = {}
    for name, (rr, cc, n_rows, n_cols) in {"rows = users (gathers item rows)": (r, c, users, items),
                                           "rows = items (gathers user rows)": (c, r, items, users)}.items():
        rp, ci, _ = ops.csr_from_coo(rr, cc, None, n_rows, n_cols)
        operands[name] = ops.Csr(n_rows, n_cols, rp, ci, None, ops.degree_scale(rp), None, {})
    del r, c
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for d in WIDTHS:
        for name, a in operands.items():
            X = torch.empty(a.n_cols, d, device="cuda").uniform_(-0.05, 0.05, generator=gen)
            Xb = ops.rows_to_bf16(X)
            Y, Y2 = torch.empty(a.n_rows, d, device="cuda"), torch.empty(a.n_rows, d, device="cuda")
            Yb = torch.empty(a.n_rows, d, dtype=torch.bfloat16, device="cuda")
            ops.spmm_bf16(a, Xb, out=Y, out_bf16=Yb)
            Xw = Xb.float()
            ops.spmm_raw(a, Xw, out=Y2)
            same = bool(torch.equal(Y, Y2)) and bool(torch.equal(Yb, Y.to(torch.bfloat16)))
            del Xw, Y2
            ms = _alternate({"fp32": lambda: ops.spmm_raw(a, X, out=Y), "bf16": lambda: ops.spmm_bf16(a, Xb, out=Y),
                             "bf16_yb": lambda: ops.spmm_bf16(a, Xb, out=Y, out_bf16=Yb), "to_bf16": lambda: ops.rows_to_bf16(X, out=Xb)})
            nnz = a.nnz
            res["rows"].append({"product": name, "d": d, "n_rows": a.n_rows, "n_cols": a.n_cols, "nnz": nnz, "bit_identical_to_fp32_on_widened": same,
                                "gathered_table_mb": {"fp32": a.n_cols * d * 4 / 1e6, "bf16": a.n_cols * d * 2 / 1e6},
                                **{k: _stat(v) for k, v in ms.items()}})
            del X, Xb, Y, Yb
            torch.cuda.empty_cache()
    return res


def part_bench(mode):
    env = dict(os.environ)
    env.pop("LLMREC_GATHER_DTYPE", None)
    if mode == "bf16":
        env["LLMREC_GATHER_DTYPE"] = "bf16"
    p = subprocess.run([sys.executable] + BENCH, cwd=ROOT, env=env, capture_output=True, text=True, timeout=LIMITS["bench_" + mode] - 20)
    if p.returncode != 0:
        raise SystemExit("bench.py (%s) ended with status %d\n%s" % (mode, p.returncode, p.stderr[-3000:]))
    line = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
    keep = {k: line.get(k) for k in ("ms_per_step", "ms_per_step_hip_events", "value", "steps", "warmup", "loss", "messages", "ingest", "config")}
    keep["command"] = ("LLMREC_GATHER_DTYPE=bf16 " if mode == "bf16" else "") + "python " + " ".join(BENCH)
    return keep


def part_loss():
    import torch
    from llmrec_amd import dist as ld, synth
    from llmrec_amd.dist_fused import ShardedFusedID
    users, items, edges, d = _arg("--loss-users", 1_250_000), _arg("--items", ITEMS), _arg("--loss-edges", 25_000_000), 64
    r, c = synth.bipartite_edges_device(users, items, edges, 7, "cuda")
    comm, be = ld.Comm(single=True), ld.HipBackend()
    g = ld.ShardedGraph.build(r, c, users, items, 0, comm, be)
    del r, c
    out = {"users": users, "items": items, "edges": edges, "d": d, "steps": LOSS_STEPS, "batch": 1024}
    losses, mem = {}, {}
    for mode in ("fp32", "bf16"):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        m0 = torch.cuda.memory_allocated()
        st = ShardedFusedID(g, comm, be, d, 2, users, seed=1, lr=1e-4, batch_local=1024, drop_rate=0.71, decay=1e-5, sparse_forward=False,
                            gather_dtype=mode)
        mem[mode] = torch.cuda.memory_allocated() - m0
        out["shadow_bytes_" + mode] = st.message_bytes_per_step()["bf16_shadow_bytes"]
        losses[mode] = [float(st.step()[0]) for _ in range(LOSS_STEPS)]
        del st
    dev = [abs(a - b) for a, b in zip(losses["fp32"], losses["bf16"])]
    out.update({"losses_fp32": losses["fp32"], "losses_bf16": losses["bf16"], "max_abs_dev": max(dev), "mean_abs_dev": sum(dev) / len(dev),
                "step_of_max_dev": dev.index(max(dev)), "state_bytes_fp32": mem["fp32"], "state_bytes_bf16": mem["bf16"]})
    return out


def _markdown(res):
    k, bf, bb, lo = res["kernel"], res["bench_fp32"], res["bench_bf16"], res["loss"]
    cell = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
    out = ["# Gathering bf16 rows in the SpMM: the bytes-per-row lever, measured (`tools/spmm_bf16_probe.py`)", "",
           "MI355X, one device, one session. Graph: `synth.bipartite_edges_device`, %d users x %d items, %d edges, pattern-only operands with a row"
           % (k["users"], k["items"], k["edges"]),
           "scale. One HIP-event pair per call; %d warm-up calls per variant, then %d rounds that alternate the variants: median ms (min .. max)."
           % (k["warm"], k["reps"]),
           "`fp32` = `llmrec_spmm_f32`; `bf16` = `llmrec_spmm_xbf16_f32` on the bf16 shadow; `+ Yb` = the same call also writing the bf16 shadow of",
           "its output; `to_bf16` = `llmrec_rows_to_bf16` over the gathered table (the pass an item-side operand pays per product in the step).", "",
           "| product | d | gathered table fp32 / bf16 MB | fp32 ms | bf16 ms | bf16 + Yb ms | to_bf16 ms | fp32 / bf16 | fp32 / (bf16 + to_bf16) | bits = fp32 kernel on widen(Xb) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in k["rows"]:
        out.append("| %s | %d | %.0f / %.0f | %s | %s | %s | %s | %.2f | %.2f | %s |" % (
            r["product"], r["d"], r["gathered_table_mb"]["fp32"], r["gathered_table_mb"]["bf16"], cell(r["fp32"]), cell(r["bf16"]), cell(r["bf16_yb"]),
            cell(r["to_bf16"]), r["fp32"]["median"] / r["bf16"]["median"], r["fp32"]["median"] / (r["bf16"]["median"] + r["to_bf16"]["median"]),
            "yes" if r["bit_identical_to_fp32_on_widened"] else "NO"))
    sp = bf["ms_per_step"] / bb["ms_per_step"]
    out += ["", "## The one-rank cfg-4-shaped step (`ShardedFusedID`, unchanged `bench.py`)", "",
            "| mode | command | ms per step (host clock) | ms per step (HIP events) | edges/s | loss of the last step | HBM peak GB |", "|---|---|---|---|---|---|---|"]
    for name, b in (("fp32 (default)", bf), ("bf16", bb)):
        out.append("| %s | `%s` | %.3f | %.3f | %.0f | %s | %.2f |" % (name, b["command"], b["ms_per_step"], b["ms_per_step_hip_events"], b["value"],
                                                                    "%.6f" % b["loss"] if b.get("loss") is not None else "-", (b.get("ingest") or {}).get("hbm_peak_gb", float("nan"))))
    cfg = bf.get("config") or {}
    out += ["", "%d users x %d items, %d edges on the rank, d = %d, %d steps after %d warm-up steps, dense forward, masked last-layer backward. "
            "fp32 / bf16 step time: **%.3f**." % (cfg.get("users_per_gpu", 0), cfg.get("n_items", 0), cfg.get("edges_per_gpu", 0), cfg.get("embed_size", 0),
                                                  bf["steps"], bf["warmup"], sp),
            "", "## Added memory", "",
            "Two preallocated shadows, [U, d] and [I, d] bf16: %d bytes at the loss run's size below (`message_bytes_per_step()[\"bf16_shadow_bytes\"]`); the"
            % lo["shadow_bytes_bf16"],
            "step object's allocations measured %d bytes in fp32 mode and %d in bf16 mode (+%.1f %%)."
            % (lo["state_bytes_fp32"], lo["state_bytes_bf16"], 100.0 * (lo["state_bytes_bf16"] - lo["state_bytes_fp32"]) / max(lo["state_bytes_fp32"], 1)),
            "", "## Loss of both modes over the same %d sampled steps" % lo["steps"], "",
            "%d users x %d items, %d edges, d = %d, batch %d, two layers, dense forward, same seed: the same initial tables and the same device-sampler batches."
            % (lo["users"], lo["items"], lo["edges"], lo["d"], lo["batch"]),
            "Largest |loss_bf16 - loss_fp32| = %.3e (step %d), mean %.3e." % (lo["max_abs_dev"], lo["step_of_max_dev"], lo["mean_abs_dev"]), "",
            "| step | fp32 | bf16 | difference |", "|---|---|---|---|"]
    for s in list(range(0, lo["steps"], max(1, lo["steps"] // 12))) + [lo["steps"] - 1]:
        out.append("| %d | %.7f | %.7f | %+.2e |" % (s, lo["losses_fp32"][s], lo["losses_bf16"][s], lo["losses_bf16"][s] - lo["losses_fp32"][s]))
    return "\n".join(out) + "\n"


PARTS = {"kernel": part_kernel, "bench_fp32": lambda: part_bench("fp32"), "bench_bf16": lambda: part_bench("bf16"), "loss": part_loss}


def main():
    if "--part" in sys.argv:
        print(json.dumps(PARTS[sys.argv[sys.argv.index("--part") + 1]]()))
        return
    out = _arg("--out", "")
    raw = _arg("--json", "")
    passed = [a for k in ("--users", "--items", "--edges", "--loss-users", "--loss-edges") if k in sys.argv for a in (k, sys.argv[sys.argv.index(k) + 1])]
    res = {}
    for part in PARTS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part] + passed, capture_output=True, text=True, timeout=LIMITS[part])
        except subprocess.TimeoutExpired:
            sys.exit("spmm_bf16_probe: part %s exceeded %d s - stopping" % (part, LIMITS[part]))
        if p.returncode != 0:
            sys.exit("spmm_bf16_probe: part %s ended with status %d - stopping\n%s" % (part, p.returncode, (p.stderr or p.stdout)[-3000:]))
        res[part] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps({part: res[part]}), flush=True)
        if raw:
            os.makedirs(os.path.dirname(os.path.abspath(raw)), exist_ok=True)
            with open(raw, "w") as fh:
                json.dump(res, fh)
    text = _markdown(res)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
