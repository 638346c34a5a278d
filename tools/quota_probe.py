"""Times per-group quotas in served lists: ops.score_topk_candidates_capped (csrc/quota.hip) against the uncapped call on the same inputs,
and Recommender.recommend under quotas - the two rounds - at several `overfetch`.

    python tools/quota_probe.py [--big] [--reps 60] [--recommend_reps 12] [--out FILE.json]

Shape: synth.NF_SHAPE with its train rows, every user queried, d = 64, K = 20 (--big: also 65 536 users x 10^6 items, no train rows); 200
random candidates per query, 1000 random groups, caps 1 and 2. The method of tools/candidates_probe.py: device-event times; all variants
of a table are warmed up, then ALTERNATE inside one loop; median and 10th / 90th percentile as a markdown table and as JSON.
  table 1  the uncapped op of the parent commit (the same launches up to the last one) and the capped op at caps 1 and 2, workspaces
           and n_groups passed in: no host read sits inside a timed region. "added" = capped median - uncapped median.
  table 2  Recommender.recommend(users, 20) without quotas, and with caps 1 and 2 at overfetch 2, 4 and 8: the whole call, the host's
           normalisation and the one host read of round 1 included (the events bracket it), and the share of queries sent to round 2.
           The lists at the three overfetch values are asserted equal before timing."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmrec_amd import ops, synth            # noqa: E402
from llmrec_amd.serve import Recommender     # noqa: E402
from serve_probe import timed                # noqa: E402

DEV = "cuda"
PER_QUERY, N_GROUPS, K = 200, 1000, 20
CAPS = (1, 2)
OVERFETCH = (2, 4, 8)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _rows(name, ms, extra):
    out = []
    for k, v in ms.items():
        v = np.asarray(v)
        out.append(dict({"shape": name, "variant": k, "median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                         "p90_ms": float(np.percentile(v, 90)), "reps": len(v)}, **extra.get(k, {})))
    return out


def shape_tables(name, U, I, d, train, reps, recommend_reps, seed=5):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    Eu = torch.randn(U, d, generator=g, device=DEV) * 0.2
    Ei = torch.randn(I, d, generator=g, device=DEV) * 0.2
    q = torch.arange(U, device=DEV)
    group = torch.randint(0, N_GROUPS, (I,), generator=g, device=DEV, dtype=torch.int32)
    cand = ((torch.arange(U + 1, dtype=torch.int64, device=DEV) * PER_QUERY).to(torch.int32),
            torch.randint(0, I, (U * PER_QUERY,), generator=g, device=DEV, dtype=torch.int32))
    ws = ops.score_topk_candidates_workspace(U, K, cand[1].numel(), 0, DEV)
    variants = {"uncapped: score_topk_candidates": lambda: ops.score_topk_candidates(Eu, Ei, q, train, K, cand, ws=ws)}
    for cap in CAPS:
        variants["capped, cap %d" % cap] = lambda cap=cap: ops.score_topk_candidates_capped(Eu, Ei, q, train, K, cand, group, cap, ws=ws, n_groups=N_GROUPS)
    plain = variants["uncapped: score_topk_candidates"]()
    assert _same(ops.score_topk_candidates_capped(Eu, Ei, q, train, K, cand, group, PER_QUERY, ws=ws, n_groups=N_GROUPS), plain)
    extra = {}
    for cap in CAPS:
        extra["capped, cap %d" % cap] = {"lists_that_differ": int((variants["capped, cap %d" % cap]()[0] != plain[0]).any(dim=1).sum())}
    one = _rows(name, timed(variants, reps), extra)
    base = one[0]["median_ms"]
    for r in one[1:]:
        r["added_ms"] = r["median_ms"] - base

    rec = Recommender(Eu, Ei, train)
    users = q
    group_host = group.cpu().numpy()
    variants, extra = {"recommend, no quota": lambda: rec.recommend(users, K)}, {}
    for cap in CAPS:
        lists = None
        for of in OVERFETCH:
            v = "recommend, cap %d, overfetch %d" % (cap, of)
            variants[v] = lambda cap=cap, of=of: rec.recommend(users, K, group_of=group_host, per_group=cap, overfetch=of)
            got = variants[v]()
            extra[v] = {"round2": rec.last_quota["round2"], "queries": U, "round2_share": rec.last_quota["round2"] / U}
            assert lists is None or _same(got, lists), "the lists depend on overfetch"
            lists = got
    two = _rows(name, timed(variants, recommend_reps, warmup=2), extra)
    return one, two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--recommend_reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sh = synth.NF_SHAPE
    rows_, cols_ = synth.bipartite_edges(sh.n_users, sh.n_items, sh.n_train, seed=0)
    rp, ci, _ = ops.csr_from_coo(torch.as_tensor(rows_, dtype=torch.int64).to(DEV), torch.as_tensor(cols_, dtype=torch.int64).to(DEV), None,
                                 sh.n_users, sh.n_items)
    train = ops.Csr(sh.n_users, sh.n_items, rp, ci, None, None, None, ops.SpmmPlan())
    one, two = shape_tables("netflix %d x %d, train rows" % (sh.n_users, sh.n_items), sh.n_users, sh.n_items, 64, train, a.reps, a.recommend_reps)
    if a.big:
        more = shape_tables("65536 x 1000000, no train rows", 65536, 1_000_000, 64, None, a.reps, a.recommend_reps)
        one, two = one + more[0], two + more[1]
    print("| shape | variant | median ms | p10 | p90 | added ms | lists that differ from the uncapped |")
    print("|---|---|---|---|---|---|---|")
    for r in one:
        print("| %s | %s | %.4f | %.4f | %.4f | %s | %s |" % (r["shape"], r["variant"], r["median_ms"], r["p10_ms"], r["p90_ms"],
                                                            "%.4f" % r["added_ms"] if "added_ms" in r else "", r.get("lists_that_differ", "")))
    print()
    print("| shape | variant | median ms | p10 | p90 | queries sent to round 2 | share |")
    print("|---|---|---|---|---|---|---|")
    for r in two:
        print("| %s | %s | %.3f | %.3f | %.3f | %s | %s |" % (r["shape"], r["variant"], r["median_ms"], r["p10_ms"], r["p90_ms"], r.get("round2", ""),
                                                            "%.5f" % r["round2_share"] if "round2_share" in r else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "recommend_reps": a.recommend_reps, "capped_op": one, "recommend": two}, f,
                      indent=1)


if __name__ == "__main__":
    main()
