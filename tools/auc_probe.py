"""Times the full-rank AUC (ops.score_auc, llmrec_score_auc_f32) next to the exact and the bf16 top-K sweeps, and Trainer.test with
--test_flag full against part. Run alone for wall times (HIP events), or under `rocprofv3 --kernel-trace --stats -- python tools/auc_probe.py`
for the kernels. --quick: the Netflix shape only; --out FILE: also write the JSON result there.
Shapes: 13 187 x 17 366 x 64 (the Netflix-shaped set) and 65 536 x 10^6 x 64; random fp32 tables, ~30 train and ~4 held-out items per user."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from llmrec_amd import ops


def _csr(rng, n_users, n_items, deg):
    lens = rng.integers(0, 2 * deg, n_users)
    rp = np.zeros(n_users + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    rows = np.repeat(np.arange(n_users), lens)
    cols = rng.integers(0, n_items, int(rp[-1]))
    order = np.lexsort((cols, rows))
    return torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(cols[order].astype(np.int32)).cuda()


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(n_users, n_items, d, reps):
    rng = np.random.default_rng(0)
    Eu = torch.from_numpy((rng.standard_normal((n_users, d)) * 0.3).astype(np.float32)).cuda()
    Ei = torch.from_numpy((rng.standard_normal((n_items, d)) * 0.3).astype(np.float32)).cuda()
    tr, held = _csr(rng, n_users, n_items, 30), _csr(rng, n_users, n_items, 4)
    train = ops.Csr(n_users, n_items, tr[0], tr[1], None, None, None, ops.SpmmPlan())
    q = torch.arange(n_users, dtype=torch.int64, device="cuda")
    ws = ops.auc_workspace(n_users, n_items, "cuda", d)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    r = {"shape": [n_users, n_items, d]}
    r["auc_ms"] = _ms(lambda: ops.score_auc(Eu, Ei, q, train, held, out=out, ws=ws), reps)
    r["topk_exact_ms"] = _ms(lambda: ops.score_topk(Eu, Ei, q, train, 50, mode="exact"), reps)
    r["topk_bf16_ms"] = _ms(lambda: ops.score_topk(Eu, Ei, q, train, 50, mode="prefilter"), reps)
    r["mean_auc"] = float(out.item()) / n_users
    return r


def trainer_test(reps):
    import e2e_main
    data = os.path.join(tempfile.gettempdir(), "llmrec_e2e")
    e2e_main.write_dataset(data)
    sys.argv = ["main.py", "--dataset", "netflix_valid_item", "--data_path", data + "/", "--epoch", "1", "--debug"]
    import main as M
    M.set_seed(2022)
    tr = M.Trainer(data_config={})
    users = list(M.data_generator.test_set.keys())
    bt = sys.modules["utility.batch_test"]
    out = {"n_users": len(users)}
    for flag in ("part", "full"):
        M.args.test_flag = bt.args.test_flag = flag
        res = tr.test(users, False)                            # capture
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            res = tr.test(users, False)
        out[flag + "_ms"] = (time.perf_counter() - t) / reps * 1e3
        out[flag + "_auc"] = float(res["auc"])
    return out


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {"netflix": kernels(13187, 17366, 64, 10)}
    if not quick:
        res["wide"] = kernels(65536, 1000000, 64, 2)
    res["trainer_test"] = trainer_test(5)
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
