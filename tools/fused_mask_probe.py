"""Step time of the fused step with feature masking and attribute restoration inside it (profiles/experiments/fused_mask.md), on bench.py's
Netflix-shaped workload, one GPU, all arms in ONE process, alternating:

  A        FusedStep(mask_rate=r): --mask_rate r alone - user features masked every forward, the default schedule
  B        FusedStep(mask_rate=r, mask_items=True, att_re_rate=a, decoder, targets): --mask True --mask_rate r --att_re_rate a
  C        FusedStep at rate 0 with LLMREC_PREPROPAGATE=0 - B's order of operations without its masking and restoration launches
  D        FusedStep at rate 0 as bench.py builds it (the default step)
  E        the per-op autograd path with B's flags: Models' torch.randperm masking and Trainer._mask_loss' term

    python tools/fused_mask_probe.py [--rate 0.1] [--att-re-rate 0.1] [--rounds 5] [--steps 400] [--modular-steps 100] [--out FILE.json]

A window is `steps` steps between two device synchronisations on the host clock; every window is reported, with the median per arm.
Masking is cumulative, as in the reference: after some hundred rounds every row holds a column mean. The launches and their sizes do
not depend on the values."""
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
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--att-re-rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--modular-steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import bench
    from llmrec_amd.fused import FusedStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    plain_import = bench.import_dropin_models

    def workload(flags, preprop, fused_kw=None, restore=False):
        """bench.NetflixShaped with `flags` on the drop-in's command line; fused_kw: its step rebuilt with the masking inside; restore: with
        a decoder and the unmasked targets (the model keeps the workload's feature tensors themselves: clone them first)."""
        if preprop is None:
            os.environ.pop("LLMREC_PREPROPAGATE", None)
        else:
            os.environ["LLMREC_PREPROPAGATE"] = preprop
        bench.import_dropin_models = lambda ds, extra=(): plain_import(ds, list(extra) + list(flags))
        try:
            wl = bench.NetflixShaped("nf", a.seed, dev)
            if restore:
                wl.decoder = wl.Models.Decoder(wl.feats["user"].shape[1]).to(dev)
                wl.targets_u = wl.feats["user"].clone()
                wl.targets_i = {k: wl.feats["attr/" + k].clone() for k in wl.keys}
            if fused_kw is not None:
                f, ar = wl.fused, wl.args
                if restore:
                    fused_kw = dict(fused_kw, decoder=wl.decoder, user_targets=wl.targets_u, item_targets=wl.targets_i,
                                    att_re_rate=a.att_re_rate, feat_loss_type=ar.feat_loss_type, alpha_l=ar.alpha_l)
                wl.fused = FusedStep(wl.model, wl.graph, wl.hp, (ar.model_cat_rate, ar.user_cat_rate, ar.item_cat_rate), wl.opt, f.b_max,
                                     mask_seed=a.seed, **fused_kw)
        finally:
            bench.import_dropin_models = plain_import
            os.environ.pop("LLMREC_PREPROPAGATE", None)
        wl.model.train()
        return wl
    user_flags = ["--mask_rate", str(a.rate)]
    mask_flags = ["--mask", "True", "--mask_rate", str(a.rate), "--att_re_rate", str(a.att_re_rate)]
    arms = {"A": workload(user_flags, None, dict(mask_rate=a.rate)),
            "B": workload(mask_flags, None, dict(mask_rate=a.rate, mask_items=True), restore=True),
            "C": workload([], "0"), "D": workload([], None), "E": workload(mask_flags, None, restore=True)}
    assert arms["A"].fused.preprop == arms["D"].fused.preprop and not arms["B"].fused.preprop and not arms["C"].fused.preprop
    assert arms["B"].fused.restore and arms["E"].args.mask and arms["E"].args.mask_rate == a.rate

    def mask_loss(wl, fw):
        """Trainer._mask_loss (main.py) over the workload's decoder and targets."""
        prof_u, att_i, i_nodes, u_nodes = fw[8], fw[11], fw[12], fw[13]
        dec_u, dec_i = wl.decoder(prof_u[u_nodes].detach(), {k: att_i[k][i_nodes] for k in att_i})
        al = wl.args.alpha_l

        def crit(x, y):
            x, y = F.normalize(x, p=2, dim=-1), F.normalize(y, p=2, dim=-1)
            return F.mse_loss(x, y) if wl.args.feat_loss_type == "mse" else (1 - (x * y).sum(dim=-1)).pow_(al).mean()
        loss = crit(dec_u, wl.targets_u[u_nodes.to(dev)])
        for k, key in enumerate(att_i):
            loss = loss + crit(dec_i[k], wl.targets_i[key][i_nodes.to(dev)])
        return a.att_re_rate * loss

    def step_modular(wl):
        u, p, n, nv = wl.batcher.next()
        return wl.engine.train_step(wl.model, wl.opt, wl.graph.ui, wl.graph.iu, u, p, n, wl.hp, n_valid=nv, extra_loss=lambda fw: mask_loss(wl, fw))

    def window(name):
        wl = arms[name]
        n = a.modular_steps if name == "E" else a.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "E":
            for _ in range(n):
                step_modular(wl)
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
    med = {k: round(statistics.median(v), 5) for k, v in times.items()}
    out = {"mask_rate": a.rate, "att_re_rate": a.att_re_rate, "steps_per_window": a.steps, "modular_steps_per_window": a.modular_steps,
           "device": torch.cuda.get_device_name(dev),
           "entry_point_calls": {k: arms[k].fused.entry_point_calls_per_step for k in ("A", "B", "C", "D")},
           "masked_rows": {"users": arms["B"].fused.m_users, "items": arms["B"].fused.m_items},
           "ms_per_step": times, "median_ms_per_step": med,
           "A_minus_D": round(med["A"] - med["D"], 5), "B_minus_C": round(med["B"] - med["C"], 5), "E_over_B": round(med["E"] / med["B"], 3),
           "mask_round": {k: int(arms[k].fused.mask_step.view(torch.int64).cpu()[0]) for k in ("A", "B")},
           "loss_finite": {k: bool(torch.isfinite(arms[k].fused.scal).all()) for k in ("A", "B", "C", "D")}}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
