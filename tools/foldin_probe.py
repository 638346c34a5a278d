"""Times the fold-in of new users (csrc/foldin.hip) at the Netflix shape: the launches alone, Recommender.recommend_new end to end against
Recommender.recommend for as many existing users with exclusion rows of the same lengths, the one-off FoldInTables.from_model, and the
SpMM of the same graph as the yardstick of the gather rate.

    python tools/foldin_probe.py [--reps 60] [--users 16384] [--out FILE.json]

Shape: synth.NF_SHAPE (13 187 users x 17 366 items, 55 146 train edges), d = 64, L = 2, five attribute keys: C = 10 slices, 2 560 B per
gathered item. Histories of 20 and of 200 distinct ids per new user. Device-event times; all variants are warmed up first and then
ALTERNATE inside one loop of `reps` rounds (>= 50); median, 10th and 90th percentile. The end-to-end lines include the host side of the
call (normalising the lists, the copies to the device): an event pair spans it because the launches wait for it."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmrec_amd import ops, synth            # noqa: E402
from llmrec_amd.serve import Recommender     # noqa: E402

DEV = "cuda"
D, L, KEYS, K = 64, 2, 5, 20
FEATS = dict(image=512, text=768, user=1536, attr=1536)
RATES = (0.55, 0.038, 0.005)


def timed(variants, reps, warmup=5):
    """{name: [ms] * reps}: every variant once per round, in the same order (as tools/serve_probe.py)."""
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


def model_and_graph(sh, seed=0):
    """What FoldInTables.from_model reads of an MM_Model, at the Netflix shape with the real feature widths, and the two normalised
    adjacencies of the synthetic train graph."""
    torch.manual_seed(seed)
    lin = lambda k: torch.nn.Linear(k, D).to(DEV)
    feat = lambda n, k: torch.randn(n, k, device=DEV) * 0.1
    emb = lambda n: SimpleNamespace(weight=torch.randn(n, D, device=DEV) * 0.1)
    model = SimpleNamespace(n_ui_layers=L, item_id_embedding=emb(sh.n_items), user_id_embedding=emb(sh.n_users),
                            image_feats=feat(sh.n_items, FEATS["image"]), text_feats=feat(sh.n_items, FEATS["text"]),
                            user_feats=feat(sh.n_users, FEATS["user"]), item_feats={"k%d" % k: feat(sh.n_items, FEATS["attr"]) for k in range(KEYS)},
                            image_trans=lin(FEATS["image"]), text_trans=lin(FEATS["text"]), user_trans=lin(FEATS["user"]), item_trans=lin(FEATS["attr"]))
    rows, cols = synth.bipartite_edges(sh.n_users, sh.n_items, sh.n_train, seed=seed)
    r, c = torch.as_tensor(rows, dtype=torch.int64).to(DEV), torch.as_tensor(cols, dtype=torch.int64).to(DEV)
    deg = lambda x, n: (torch.bincount(x, minlength=n).double() + 1e-8).pow(-0.5).float()
    ui = ops.SparseOperand.from_coo(r, c, deg(r, sh.n_users)[r], sh.n_users, sh.n_items)
    iu = ops.SparseOperand.from_coo(c, r, deg(c, sh.n_items)[c], sh.n_items, sh.n_users)
    return model, ui, iu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps, n = max(a.reps, 50), a.users
    sh = synth.NF_SHAPE
    model, ui, iu = model_and_graph(sh)
    tables = ops.FoldInTables.from_model(model, ui, iu, RATES)
    rng = np.random.default_rng(1)
    g = torch.Generator(device=DEV)
    g.manual_seed(2)
    rec = Recommender(torch.randn(sh.n_users, D, generator=g, device=DEV) * 0.2, torch.randn(sh.n_items, D, generator=g, device=DEV) * 0.2,
                      None, tables)
    old_users = rng.integers(0, sh.n_users, n)
    X = torch.randn(sh.n_items, D, device=DEV)
    Y = torch.empty(sh.n_users, D, device=DEV)
    variants = {"FoldInTables.from_model (one-off)": lambda: ops.FoldInTables.from_model(model, ui, iu, RATES),
                "spmm ui x [items, 64] (the graph's own product)": lambda: ops.spmm_raw(ui.fwd, X, out=Y)}
    meta = {}
    for m in (20, 200):
        hist = np.sort(np.stack([rng.choice(sh.n_items, size=m, replace=False) for _ in range(n)]), axis=1).astype(np.int32)
        rp = torch.arange(0, n * m + 1, m, dtype=torch.int32, device=DEV)
        ci = torch.from_numpy(hist.reshape(-1)).to(DEV)
        w = ops.fold_in_row_scale(rp)
        out = torch.empty(n, D, device=DEV)
        ws = ops.fold_in_workspace(n, ci.numel(), tables, DEV)
        host_csr = (rp.cpu().numpy(), hist.reshape(-1))
        q = torch.arange(n, device=DEV)
        variants["fold-in launches alone, %d ids" % m] = (lambda rp=rp, ci=ci, w=w, out=out, ws=ws: ops.fold_in_users(tables, rp, ci, row_scale=w, out=out, ws=ws))
        variants["device side of recommend_new, %d ids" % m] = (lambda rp=rp, ci=ci, w=w, out=out, ws=ws, q=q: ops.score_topk_excluded(
            ops.fold_in_users(tables, rp, ci, row_scale=w, out=out, ws=ws), rec.E_i, q, None, K, (rp, ci)))
        variants["device side of recommend, %d ids" % m] = (lambda rp=rp, ci=ci, qq=torch.from_numpy(old_users).to(DEV): ops.score_topk_excluded(
            rec.E_u, rec.E_i, qq, None, K, (rp, ci)))
        variants["recommend_new end to end, %d ids" % m] = (lambda h=host_csr: rec.recommend_new(h, K))
        variants["recommend end to end, %d ids" % m] = (lambda h=host_csr: rec.recommend(old_users, K, exclude_seen=False, exclude=h))
        meta["fold-in launches alone, %d ids" % m] = n * m * tables.C * D * 4
    meta["spmm ui x [items, 64] (the graph's own product)"] = sh.n_train * D * 4
    ms = timed(variants, reps)
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        med = float(np.median(v))
        rows.append({"variant": k, "median_ms": med, "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)),
                     "gathered_bytes": meta.get(k), "gathered_TB_per_s": meta[k] / med / 1e9 if k in meta else None, "reps": len(v)})
    print("%d new users, %d items, d = %d, C = %d (%d B per gathered item), K = %d" % (n, sh.n_items, D, tables.C, tables.C * D * 4, K))
    print("| variant | median ms | p10 | p90 | gathered bytes | TB/s of gathered rows |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.4f | %s | %s |" % (r["variant"], r["median_ms"], r["p10_ms"], r["p90_ms"], r["gathered_bytes"] or "-",
                                                       "%.3f" % r["gathered_TB_per_s"] if r["gathered_TB_per_s"] else "-"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
