"""What a checkpoint costs (profiles/experiments/checkpoint.md), on bench.py's synthetic Netflix-shaped workload, the device-sampler path
(an epoch = n_batch replayed steps + one evaluation), one GPU.

    python tools/checkpoint_probe.py [--epochs 30] [--out FILE.json]          every arm, each in a child process under its own time limit
    python tools/checkpoint_probe.py --arm epoch|request|mask [...]           one arm in this process

  epoch     wall time of an epoch with none of the checkpoint variables in play (this arm imports nothing of the feature, so the same
            file runs on the parent commit: the yardstick)
  request   the same epochs with Checkpointer.request() behind every evaluation: the host time of request(), the device time of the pack
            launch and of the D2H copy (events around them), the writer's crc and write time, how often a request waited; then load()
  mask      the masking replay a load pays: FusedStep._mask_round() 1 000 and 15 000 times, user features only and with the attribute
            matrices

Epochs are timed on the host clock between two device synchronisations, after warm-up epochs (capture, plan caches); every figure is
reported with its spread (min / median / max)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"epoch": 240, "request": 300, "mask": 300}          # seconds per arm


def spread(xs, scale=1.0, digits=4):
    xs = [x * scale for x in xs]
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def workload(flags=(), fused_kw=None, seed=2022):
    import torch
    import bench
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    plain = bench.import_dropin_models
    bench.import_dropin_models = lambda ds, extra=(): plain(ds, list(extra) + list(flags))
    try:
        wl = bench.NetflixShaped("nf", seed, dev)
    finally:
        bench.import_dropin_models = plain
    if fused_kw is not None:
        from llmrec_amd.fused import FusedStep
        ar = wl.args
        wl.fused = FusedStep(wl.model, wl.graph, wl.hp, (ar.model_cat_rate, ar.user_cat_rate, ar.item_cat_rate), wl.opt, wl.fused.b_max,
                             mask_seed=seed, **fused_kw)
    wl.model.train()
    return wl, wl.sh.n_train // wl.hp.batch_size + 1


def timed_epochs(wl, n_batch, epochs, warm, after_eval=None):
    import torch
    out = []
    for e in range(warm + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wl.run_steps(n_batch)
        wl.eval_once()
        if after_eval is not None:
            after_eval(e)
        torch.cuda.synchronize()
        if e >= warm:
            out.append(time.perf_counter() - t0)
    return out


def arm_epoch(a):
    wl, n_batch = workload()
    import torch
    return {"device": torch.cuda.get_device_name(0), "n_batch": n_batch, "epoch_ms": spread(timed_epochs(wl, n_batch, a.epochs, a.warm), 1e3)}


def arm_request(a):
    import torch
    from llmrec_amd import checkpoint
    wl, n_batch = workload()
    plain = spread(timed_epochs(wl, n_batch, a.epochs, a.warm), 1e3)
    with tempfile.TemporaryDirectory() as d:
        ck = checkpoint.Checkpointer([wl.fused, wl.batcher], d)
        ck.time_pack = True
        ck.prepare()
        rec = {"request_host_ms": [], "pack_device_ms": [], "d2h_ms": [], "crc_ms": [], "write_ms": []}

        def collect():                                            # the previous request's figures, once its write is done
            ck.wait()
            rec["pack_device_ms"].append(ck.ev_pack_begin.elapsed_time(ck.ev_packed))
            rec["d2h_ms"].append(ck.ev_packed.elapsed_time(ck.ev_copied))
            rec["crc_ms"].append(1e3 * ck.stats["last_crc_s"])
            rec["write_ms"].append(1e3 * ck.stats["last_write_s"])
        pending = [False]

        def after_eval(e):
            if pending[0]:
                collect()
            ck.request("last.ckpt", {"epoch": e})
            rec["request_host_ms"].append(1e3 * ck.stats["last_request_s"])
            pending[0] = True
        with_req = spread(timed_epochs(wl, n_batch, a.epochs, 2, after_eval), 1e3)
        collect()
        waits_inline = ck.stats["waits"]
        # the same without the probe's own wait(): how often does a request of every epoch find the previous write in flight?
        ck.stats["waits"] = 0
        free = spread(timed_epochs(wl, n_batch, a.epochs, 0, lambda e: ck.request("last.ckpt", {"epoch": e})), 1e3)
        ck.wait()
        loads = []
        for _ in range(5):
            ck.load(os.path.join(d, "last.ckpt"))
            loads.append(ck.stats["last_load_s"])
        size = os.path.getsize(os.path.join(d, "last.ckpt"))
        out = {"device": torch.cuda.get_device_name(0), "n_batch": n_batch, "tensors": len(ck._manifest), "arena_bytes": ck._total, "file_bytes": size,
               "epoch_ms_unset": plain, "epoch_ms_request_every_epoch_probe_waits": with_req, "epoch_ms_request_every_epoch": free,
               "requests_that_waited": {"of": a.epochs, "waited": ck.stats["waits"], "probe_arm": waits_inline},
               "wait_ms_total": round(1e3 * ck.stats["wait_s"], 3), "load_ms": spread(loads, 1e3)}
        out.update({k: spread(v[2:] if len(v) > 4 else v) for k, v in rec.items()})
        ck.close()
    return out


def arm_mask(a):
    import torch
    out = {}
    for name, flags, kw in (("users", ["--mask_rate", "0.1"], dict(mask_rate=0.1)),
                            ("users_and_items", ["--mask", "True", "--mask_rate", "0.1"], dict(mask_rate=0.1, mask_items=True))):
        wl, _ = workload(flags, kw)
        f = wl.fused
        for rounds in (1000, 15000):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                f._mask_round()
            torch.cuda.synchronize()
            out["%s/%d_rounds_s" % (name, rounds)] = round(time.perf_counter() - t0, 4)
        out[name + "/mask_step"] = int(f.mask_step.view(torch.int64).cpu()[0])
        del wl, f
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=sorted(LIMITS), default=None)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm is not None:
        print("RESULT " + json.dumps({"epoch": arm_epoch, "request": arm_request, "mask": arm_mask}[a.arm](a)))
        return 0
    result = {}
    for arm in ("epoch", "request", "mask"):                      # a fresh child per arm; a failed or overdue arm ends the probe
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--epochs", str(a.epochs), "--warm", str(a.warm)],
                               capture_output=True, text=True, timeout=LIMITS[arm])
        except subprocess.TimeoutExpired:
            result[arm] = {"error": "no result within %d s" % LIMITS[arm]}
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            result[arm] = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-2000:]}
            break
        result[arm] = json.loads(line[-1][7:])
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if all("error" not in v for v in result.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
