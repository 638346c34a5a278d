"""`python bench.py --gpus N` without a launcher in the environment (the driver's plain command): it must become N ranks - here two
ranks on this box's one GPU through the test hook LLMREC_BENCH_SINGLE_DEVICE=1 + gloo - or refuse with a non-zero exit code; it must
never print a 1-GPU line labelled N (VERDICT r03 missing #2). The plain 1-GPU command runs the timed path and the evaluation leg only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_bench_gpus_2_spawns_two_ranks():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "nf", "--steps", "6", "--warmup", "2", "--no-row-sharded",
                        "--no-cpu-baseline", "--no-kernel-roofline"], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=_env(LLMREC_BENCH_SINGLE_DEVICE="1", LLMREC_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # ONE line, from rank 0
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["n_ranks_seen"] == 2 and line["n_devices_seen"] == 1      # (one device: the test hook)
    assert line["config"]["global_batch"] == 2 * line["config"]["batch_size"]
    assert "torch.distributed.run" in r.stderr


def test_bench_gpus_2_refuses_on_a_one_gpu_box():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 GPUs")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=_env())
    assert r.returncode == 2 and "refused" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_plain_bench_run_leaves_the_side_legs_to_full():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == ("bpr_train_edges_per_sec", "edges/s", True, "f32")
    assert line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["eval"]["value"] > 0
    side = {"parity", "roofline", "spmm_roofline", "exact_f32", "reference_order", "pre_propagated_order", "end_to_end", "ml", "cfg5", "row_sharded",
            "cpu_baseline", "step_in_graph"}
    assert not side & set(line), sorted(side & set(line))
