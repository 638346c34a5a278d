"""Times ops.score_topk against ops.score_topk_filtered (the serving pipeline of csrc/serve.hip, without its exclusion stage) at several
allow fractions, and the filter build alone.

    python tools/serve_probe.py [--big] [--reps 60] [--out FILE.json]

Shape: synth.NF_SHAPE with its train rows, every user queried, d = 64, K = 20 (--big: also 65 536 users x 10^6 items, no train rows).
Device-event times; all variants are warmed up first and then ALTERNATE inside one loop, `reps` rounds (>= 50), so that clock and
thermal drift fall on every variant alike; the median and the 10th / 90th percentile of each are printed as a markdown table and written
as JSON. The filtered calls are given train_nnz and a workspace, so no host read sits inside a timed region."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmrec_amd import ops, synth            # noqa: E402

DEV = "cuda"
FRACTIONS = (1.0, 0.5, 0.1)


def timed(variants, reps, warmup=5):
    """{name: [ms] * reps}: every variant once per round, in the same order."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def shape_table(name, U, I, d, K, train, reps, seed=5):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    Eu = torch.randn(U, d, generator=g, device=DEV) * 0.2
    Ei = torch.randn(I, d, generator=g, device=DEV) * 0.2
    q = torch.arange(U, device=DEV)
    nnz = train.colidx.numel() if train is not None else 0
    rng = np.random.default_rng(seed)
    variants = {"score_topk (unfiltered)": lambda: ops.score_topk(Eu, Ei, q, train, K)}
    kept = {}
    for frac in FRACTIONS:
        allow = torch.tensor((rng.random(I) < frac).astype(np.uint8) if frac < 1.0 else np.ones(I, np.uint8)).to(DEV)
        filt = ops.ItemFilter(allow)
        ws = ops.topk_filtered_workspace(U, I, filt.n_kept, DEV, d, K, nnz)
        label = "filtered, allow %.1f" % frac
        kept[label] = filt.n_kept
        variants[label] = (lambda filt=filt, ws=ws: ops.score_topk_filtered(Eu, Ei, q, train, K, filt, train_nnz=nnz, ws=ws))
        if frac == 0.5:
            variants["ItemFilter build (allow 0.5, with its host read)"] = (lambda allow=allow: ops.ItemFilter(allow))
    # all-allowed must be the unfiltered answer, bit for bit (the probe times what the tests hold)
    a, b = variants["score_topk (unfiltered)"](), variants["filtered, allow 1.0"]()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    ms = timed(variants, reps)
    rows = []
    base = float(np.median(ms["score_topk (unfiltered)"]))
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append({"shape": name, "variant": k, "n_kept": kept.get(k), "median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "vs_unfiltered": float(np.median(v)) / base, "reps": len(v)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 50)
    sh = synth.NF_SHAPE
    rows_, cols_ = synth.bipartite_edges(sh.n_users, sh.n_items, sh.n_train, seed=0)
    rp, ci, _ = ops.csr_from_coo(torch.as_tensor(rows_, dtype=torch.int64).to(DEV), torch.as_tensor(cols_, dtype=torch.int64).to(DEV), None,
                                 sh.n_users, sh.n_items)
    train = ops.Csr(sh.n_users, sh.n_items, rp, ci, None, None, None, ops.SpmmPlan())
    rows = shape_table("netflix %d x %d, train rows" % (sh.n_users, sh.n_items), sh.n_users, sh.n_items, 64, 20, train, reps)
    if a.big:
        rows += shape_table("65536 x 1000000, no train rows", 65536, 1_000_000, 64, 20, None, reps)
    print("| shape | variant | items kept | median ms | p10 | p90 | vs unfiltered |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %s | %.4f | %.4f | %.4f | %.2f x |" % (r["shape"], r["variant"], "-" if r["n_kept"] is None else r["n_kept"], r["median_ms"],
                                                               r["p10_ms"], r["p90_ms"], r["vs_unfiltered"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
