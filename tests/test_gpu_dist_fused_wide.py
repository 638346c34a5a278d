"""The row-sharded fused ID step (llmrec_amd/dist_fused.py) with batch_local above LLMREC_BPR_MAX_B: HipBackend.bpr_fwd routes both
passes of the prune selection to llmrec_bpr_prune_fwd_wide_f32 (by size only), everything else of the step is size-free. The pattern,
the oracle and the bounds of tests/test_gpu_dist_fused.py:
* one rank of 4 200 (+ 6 augmented) triples against the single-process oracle;
* two PROCESSES of 6 200 triples on one GPU (gloo): the global list of 12 400 exceeds the capped entry point's 3 x 4 096 as well."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import oracle as O

U, I, L, STEPS = 900, 700, 2, 3
B_ONE, B_TWO = 4200, 6200
DROP, DECAY, LR = 0.71, 1e-5, 1e-3
CASES = [(64, 0), (128, 6)]                                             # (d, augmented triples per rank)


def _problem(world, D, n_aug, b_local):
    rng = np.random.default_rng(4)
    deg = rng.integers(1, 30, size=U); deg[7] = 600; deg[U - 3] = 200                     # hubs in both halves
    rows = np.repeat(np.arange(U), deg)
    cols = np.concatenate([rng.choice(I, size=c, replace=False) for c in deg])
    hot = rng.integers(0, U, size=2500); rows = np.concatenate([rows, hot]); cols = np.concatenate([cols, np.full(hot.size, 5)])   # a hub item
    key = np.unique(rows * I + cols); rows, cols = key // I, key % I
    u_tab = (rng.standard_normal((U, D)) * 0.1).astype(np.float32)
    i_tab = (rng.standard_normal((I, D)) * 0.1).astype(np.float32)
    per = (U + world - 1) // world
    batches = []
    for s in range(STEPS):
        per_rank = []
        for r in range(world):
            u0, u1 = r * per, min((r + 1) * per, U)
            pos = rng.integers(0, I, size=b_local); pos[:40] = 5                           # a long run of one gradient row
            us, ns = rng.integers(u0, u1, size=b_local), rng.integers(0, I, size=b_local)
            if n_aug:                                                                      # extra triples for users of the batch
                us, pos, ns = np.concatenate([us, us[:n_aug]]), np.concatenate([pos, rng.integers(0, I, size=n_aug)]), np.concatenate([ns, rng.integers(0, I, size=n_aug)])
            per_rank.append((us, pos, ns))
        batches.append(per_rank)
    return rows, cols, u_tab, i_tab, batches


def _oracle_run(world, D, n_aug, b_local):
    import scipy.sparse as sp
    rows, cols, u_tab, i_tab, batches = _problem(world, D, n_aug, b_local)
    R = sp.csr_matrix((np.ones(rows.size, dtype=np.float32), (rows, cols)), shape=(U, I))
    a_ui, a_iu = O.normalized_graphs(R)
    pu = torch.tensor(u_tab, requires_grad=True); pi = torch.tensor(i_tab, requires_grad=True)
    opt = torch.optim.AdamW([{"params": [pu, pi]}], lr=LR)
    cfg = O.Config(batch_size=world * b_local, decay=DECAY, prune_loss_drop_rate=DROP)
    losses = []
    for per_rank in batches:
        us = np.concatenate([b[0] for b in per_rank]); ps = np.concatenate([b[1] for b in per_rank]); ns = np.concatenate([b[2] for b in per_rank])
        u, i = pu, pi
        ul, il = [u], [i]
        for l in range(L):
            u = torch.sparse.mm(a_ui, i)
            if l == L - 1: u = torch.softmax(u, -1)
            i = torch.sparse.mm(a_iu, u)
            if l == L - 1: i = torch.softmax(i, -1)
            ul.append(u); il.append(i)
        eu, ei = torch.mean(torch.stack(ul), 0), torch.mean(torch.stack(il), 0)
        mf, emb = O.bpr_loss(eu[torch.tensor(us)], ei[torch.tensor(ps)], ei[torch.tensor(ns)], cfg)
        opt.zero_grad(); (mf + emb).backward(); opt.step()
        losses.append(float((mf + emb).detach()))
    return pu.detach().numpy(), pi.detach().numpy(), losses


def _run_rank(rank, world, n_chunks, D, n_aug, b_local):
    from llmrec_amd import _lib, dist as ld
    from llmrec_amd.dist_fused import ShardedFusedID
    assert b_local > _lib.CONST["LLMREC_BPR_MAX_B"]
    rows, cols, u_tab, i_tab, batches = _problem(world, D, n_aug, b_local)
    comm, be = ld.Comm(), ld.HipBackend()
    u0, u1 = ld.user_block(U, rank, world)
    sel = (rows >= u0) & (rows < u1)
    g = ld.ShardedGraph.build(torch.tensor(rows[sel] - u0).cuda(), torch.tensor(cols[sel]).cuda(), u1 - u0, I, u0, comm, be)
    st = ShardedFusedID(g, comm, be, D, L, U, seed=1, lr=LR, batch_local=b_local + n_aug, drop_rate=DROP, decay=DECAY, n_chunks=n_chunks,
                        user_init=torch.tensor(u_tab[u0:u1]), item_init=torch.tensor(i_tab),
                        batch_size_flag=float(world * b_local))                           # the divisor is the FLAG (main.py:340), not B + aug
    losses = []
    for per_rank in batches:
        us, ps, ns = per_rank[rank]
        loss, _ = st.step((torch.tensor(us - u0).cuda(), torch.tensor(ps).cuda(), torch.tensor(ns).cuda()))
        losses.append(float(loss))
        assert float(st.dE_u.abs().max()) == 0.0 and float(st.dE_i.abs().max()) == 0.0    # row-wise clean-up left the scatter targets zero
    assert getattr(be, "_bpr_wide_ws", None) is not None                                  # the selection took the multi-block kernels
    return st, losses


@pytest.mark.parametrize("D,n_aug", CASES)
def test_wide_sharded_step_single_rank_matches_oracle(D, n_aug):
    ref_u, ref_i, ref_losses = _oracle_run(1, D, n_aug, B_ONE)
    st, losses = _run_rank(0, 1, 3, D, n_aug, B_ONE)
    assert np.allclose(losses, ref_losses, rtol=2e-5), (losses, ref_losses)
    got_u, got_i = st.user_tab.detach().cpu().numpy(), st.item_tab.detach().cpu().numpy()
    assert np.abs(got_u - ref_u).max() <= 1e-4 * np.abs(ref_u).max()
    assert np.abs(got_i - ref_i).max() <= 1e-4 * np.abs(ref_i).max()


def _worker(rank, world, port, out_dir, D, n_aug, b_local):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    st, losses = _run_rank(rank, world, 3, D, n_aug, b_local)
    np.savez(os.path.join(out_dir, "g%d.npz" % rank), users=st.user_tab.detach().cpu().numpy(), items=st.item_tab.detach().cpu().numpy(),
             losses=np.array(losses))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_wide_sharded_step_two_processes_one_gpu_match_oracle(tmp_path):
    D, n_aug, world = 64, 0, 2
    assert world * B_TWO > 3 * 4096
    ref_u, ref_i, ref_losses = _oracle_run(world, D, n_aug, B_TWO)
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), D, n_aug, B_TWO), nprocs=world, join=True)
    r = [np.load(tmp_path / ("g%d.npz" % k)) for k in range(world)]
    assert np.array_equal(r[0]["items"], r[1]["items"])                                   # replicas bit-identical (deterministic scatter)
    for j in range(world):
        assert np.allclose(r[j]["losses"], ref_losses, rtol=2e-5)
    got_u = np.concatenate([r[j]["users"] for j in range(world)])
    assert np.abs(got_u - ref_u).max() <= 1e-4 * np.abs(ref_u).max()
    assert np.abs(r[0]["items"] - ref_i).max() <= 1e-4 * np.abs(ref_i).max()
