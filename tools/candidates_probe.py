"""Times ops.score_topk_candidates (csrc/candidates.hip: exact top-K among per-query candidate lists) against the two routes that exist
without it.

    python tools/candidates_probe.py [--big] [--reps 60] [--out FILE.json]
    LLMREC_LIB=llmrec_amd/lib/libllmrec_hip_tools.so python tools/candidates_probe.py --lanes [--big]      # the two lane mappings
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/candidates_probe.py --stages 200 [--big]       # the per-stage split

Shape: synth.NF_SHAPE with its train rows, every user queried, d = 64, K = 20 (--big: also 65 536 users x 10^6 items, no train rows); 20,
200 and 1000 random candidates per query. Yardsticks, measured in the same loop on the same inputs:
  (a) ops.score_topk_excluded over the whole catalogue - a DIFFERENT list (the best of the catalogue): a cost yardstick only;
  (b) ops.scores followed by a torch gather + sort of the candidate columns - the same lists: equality is asserted before timing. It needs
      the [n_users, n_items] score block, so it exists at the small shape only.
Device-event times; all variants are warmed up five times and then ALTERNATE inside one loop, `reps` rounds (>= 50), as
tools/exclude_probe.py does; median and 10th / 90th percentile are printed as a markdown table and written as JSON. Workspaces and sizes are
passed in: no host read sits inside a timed region.
--lanes: only the candidate calls, the score kernel at 1 and at 4 lanes per pair alternating (the tools build reads LLMREC_CAND_LANES per
call); the two must agree bit for bit. --stages M: 20 calls at M candidates per query and nothing else, for a profiler."""
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
PER_QUERY = (20, 200, 1000)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def torch_route(Eu, Ei, q, seen, ids_sorted, K):
    """(b): the whole score block, then the candidate columns: repeats and seen items to -inf, a stable sort by score over ids ascending"""
    S = ops.scores(Eu, Ei, q)
    sc = S.gather(1, ids_sorted)
    sc[:, 1:][ids_sorted[:, 1:] == ids_sorted[:, :-1]] = float("-inf")
    if seen is not None:
        sc[seen.gather(1, ids_sorted)] = float("-inf")
    order = sc.sort(dim=1, descending=True, stable=True).indices[:, :K]
    out_s = sc.gather(1, order)
    out_i = torch.where(torch.isneginf(out_s), torch.full_like(order, -1), ids_sorted.gather(1, order))
    return out_i.to(torch.int32), out_s


def inputs(U, I, d, train, seed=5):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    Eu = torch.randn(U, d, generator=g, device=DEV) * 0.2
    Ei = torch.randn(I, d, generator=g, device=DEV) * 0.2
    q = torch.arange(U, device=DEV)
    lists = {}
    for m in PER_QUERY:
        rp = (torch.arange(U + 1, dtype=torch.int64, device=DEV) * m).to(torch.int32)
        lists[m] = (rp, torch.randint(0, I, (U * m,), generator=g, device=DEV, dtype=torch.int32))
    return Eu, Ei, q, lists


def candidate_call(Eu, Ei, q, train, K, cand, lanes=None):
    ws = ops.score_topk_candidates_workspace(q.numel(), K, cand[1].numel(), 0, DEV)

    def run():
        if lanes is not None:
            os.environ["LLMREC_CAND_LANES"] = str(lanes)
        return ops.score_topk_candidates(Eu, Ei, q, train, K, cand, ws=ws)
    return run


def shape_table(name, U, I, d, K, train, reps, lanes_mode, with_block):
    Eu, Ei, q, lists = inputs(U, I, d, train)
    nnz = train.colidx.numel() if train is not None else 0
    variants, meta = {}, {}
    if lanes_mode:
        for m in PER_QUERY:
            for lanes in (1, 4):
                v = "%d candidates per query, %d lane%s per pair" % (m, lanes, "s" if lanes > 1 else "")
                variants[v] = candidate_call(Eu, Ei, q, train, K, lists[m], lanes)
                meta[v] = U * m
            assert _same(variants["%d candidates per query, 1 lane per pair" % m](), variants["%d candidates per query, 4 lanes per pair" % m]())
    else:
        ws = ops.topk_excluded_workspace(U, I, I, DEV, d, K, nnz, 0)
        empty = (torch.zeros(U + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
        variants["(a) full sweep: score_topk_excluded over the catalogue"] = lambda: ops.score_topk_excluded(Eu, Ei, q, train, K, empty, None, train_nnz=nnz, ws=ws)
        meta["(a) full sweep: score_topk_excluded over the catalogue"] = U * I
        seen = None
        if with_block and train is not None:
            seen = torch.zeros(U, I, dtype=torch.bool, device=DEV)
            rows = torch.repeat_interleave(torch.arange(U, device=DEV), (train.rowptr[1:] - train.rowptr[:-1]).long())
            seen[rows, train.colidx.long()] = True
        for m in PER_QUERY:
            v = "%d candidates per query" % m
            variants[v] = candidate_call(Eu, Ei, q, train, K, lists[m])
            meta[v] = U * m
            if with_block:
                ids_sorted = lists[m][1].view(U, m).long().sort(dim=1).values
                b = "(b) scores + gather + sort, %d candidates per query" % m
                variants[b] = lambda ids_sorted=ids_sorted: torch_route(Eu, Ei, q, seen, ids_sorted, K)
                meta[b] = U * m
                assert _same(variants[v](), variants[b]()), "the torch route gives other lists"
    ms = timed(variants, reps)
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append({"shape": name, "variant": k, "pairs": meta[k], "median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                     "p90_ms": float(np.percentile(v, 90)), "reps": len(v)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--lanes", action="store_true")
    ap.add_argument("--stages", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 50)
    sh = synth.NF_SHAPE
    rows_, cols_ = synth.bipartite_edges(sh.n_users, sh.n_items, sh.n_train, seed=0)
    rp, ci, _ = ops.csr_from_coo(torch.as_tensor(rows_, dtype=torch.int64).to(DEV), torch.as_tensor(cols_, dtype=torch.int64).to(DEV), None,
                                 sh.n_users, sh.n_items)
    train = ops.Csr(sh.n_users, sh.n_items, rp, ci, None, None, None, ops.SpmmPlan())
    if a.lanes and "LLMREC_LIB" not in os.environ:
        raise SystemExit("--lanes needs the tools build: LLMREC_LIB=.../libllmrec_hip_tools.so (python -m llmrec_amd.build --tools)")
    if a.stages:
        U, I, tr = (65536, 1_000_000, None) if a.big else (sh.n_users, sh.n_items, train)
        Eu, Ei, q, lists = inputs(U, I, 64, tr)
        run = candidate_call(Eu, Ei, q, tr, 20, lists[a.stages])
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        return
    rows = shape_table("netflix %d x %d, train rows" % (sh.n_users, sh.n_items), sh.n_users, sh.n_items, 64, 20, train, reps, a.lanes, True)
    if a.big:
        rows += shape_table("65536 x 1000000, no train rows", 65536, 1_000_000, 64, 20, None, reps, a.lanes, False)
    print("| shape | variant | pairs scored | median ms | p10 | p90 |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %d | %.4f | %.4f | %.4f |" % (r["shape"], r["variant"], r["pairs"], r["median_ms"], r["p10_ms"], r["p90_ms"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "lanes_mode": a.lanes, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
