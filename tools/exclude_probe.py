"""Times ops.score_topk_excluded (the serving pipeline of csrc/serve.hip with the exclusion stage of csrc/exclude.hip) against the same
call without exclusion lists, unfiltered and under a filter that keeps a tenth of the items.

    python tools/exclude_probe.py [--big] [--reps 60] [--out FILE.json]

Shape: synth.NF_SHAPE with its train rows, every user queried, d = 64, K = 20 (--big: also 65 536 users x 10^6 items, no train rows).
Per filter setting: no exclusion (exclude=None: the call forwards to ops.score_topk_filtered / ops.score_topk), every exclusion row empty,
and 20 and 200 random ids per query. Device-event times; all variants are warmed up first and then ALTERNATE inside one loop, `reps`
rounds (>= 50), as tools/serve_probe.py does; the median and the 10th / 90th percentile of each are printed as a markdown table and written as
JSON. Every call that takes them is given train_nnz and a workspace, so no host read sits inside a timed region."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmrec_amd import ops, synth            # noqa: E402
from serve_probe import timed                # noqa: E402

DEV = "cuda"
PER_QUERY = (0, 20, 200)


def shape_table(name, U, I, d, K, train, reps, seed=5):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    Eu = torch.randn(U, d, generator=g, device=DEV) * 0.2
    Ei = torch.randn(I, d, generator=g, device=DEV) * 0.2
    q = torch.arange(U, device=DEV)
    nnz = train.colidx.numel() if train is not None else 0
    rng = np.random.default_rng(seed)
    tenth = ops.ItemFilter(torch.tensor((rng.random(I) < 0.1).astype(np.uint8)).to(DEV))
    lists = {}
    for m in PER_QUERY:
        rp = (torch.arange(U + 1, dtype=torch.int64, device=DEV) * m).to(torch.int32)
        lists[m] = (rp, torch.randint(0, I, (U * m,), generator=g, device=DEV, dtype=torch.int32))
    variants, meta = {}, {}
    for label, filt in (("unfiltered", None), ("keep 0.1", tenth)):
        kept = filt.n_kept if filt is not None else I
        base = "%s, no exclusion" % label
        ws = ops.topk_filtered_workspace(U, I, kept, DEV, d, K, nnz) if filt is not None else None
        variants[base] = (lambda filt=filt, ws=ws: ops.score_topk_excluded(Eu, Ei, q, train, K, None, filt, train_nnz=nnz, ws=ws))
        meta[base] = (label, kept, None, base)
        for m in PER_QUERY:
            ws = ops.topk_excluded_workspace(U, I, kept, DEV, d, K, nnz, U * m)
            v = "%s, %s" % (label, "every row empty" if m == 0 else "%d ids per query" % m)
            variants[v] = (lambda filt=filt, ws=ws, e=lists[m]: ops.score_topk_excluded(Eu, Ei, q, train, K, e, filt, train_nnz=nnz, ws=ws))
            meta[v] = (label, kept, U * m, base)
        # empty rows must be the call without them, bit for bit (the probe times what the tests hold)
        a, b = variants[base](), variants["%s, every row empty" % label]()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        c = variants["%s, 200 ids per query" % label]()
        assert not torch.equal(a[0], c[0])
    ms = timed(variants, reps)
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        base = float(np.median(ms[meta[k][3]]))
        rows.append({"shape": name, "variant": k, "n_kept": meta[k][1], "excl_nnz": meta[k][2], "median_ms": float(np.median(v)),
                     "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "over_no_exclusion_ms": float(np.median(v)) - base,
                     "vs_no_exclusion": float(np.median(v)) / base, "reps": len(v)})
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
    print("| shape | variant | items swept | exclusion entries | median ms | p10 | p90 | over no exclusion |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %d | %s | %.4f | %.4f | %.4f | %+.4f ms (%.2f x) |" % (
            r["shape"], r["variant"], r["n_kept"], "-" if r["excl_nnz"] is None else r["excl_nnz"], r["median_ms"], r["p10_ms"], r["p90_ms"],
            r["over_no_exclusion_ms"], r["vs_no_exclusion"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
