"""GPU: llmrec_sample_batch_wide (256 BPR slots per block, one block for the augmented triples, a last-block-done ticket for the
step counter) against llmrec_sample_batch, which tests/test_gpu_sampler.py pins to the numpy restatement: users / pos / neg on
[0, n_valid), n_valid and the counter with torch.equal; the padding is zero, the tail of the buffers untouched, the ticket back at 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL, TAIL = -7, 9
N_USERS, N_ITEMS = 2600, 211


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available()
    from llmrec_amd import ops
    rng = np.random.default_rng(77)
    exist = np.arange(1, N_USERS, 2)                                     # 1300 users with train items: a slot is never its own id
    degs = np.zeros(N_USERS, dtype=np.int64)
    rows = {int(u): np.sort(rng.choice(N_ITEMS, size=int(rng.integers(1, 12)), replace=False)) for u in exist}
    for u, r in rows.items():
        degs[u] = len(r)
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    colidx = np.concatenate([rows[u] for u in sorted(rows)])
    csr = ops.Csr(N_USERS, N_ITEMS, torch.tensor(rowptr, dtype=torch.int32, device=DEV), torch.tensor(colidx, dtype=torch.int32, device=DEV),
                  None, None, None)
    aug = {"mixed": (rng.integers(-3, int(1.3 * N_ITEMS), size=N_USERS), rng.integers(-3, int(1.3 * N_ITEMS), size=N_USERS)),
           "all_invalid": (np.full(N_USERS, N_ITEMS), np.full(N_USERS, -1)),
           "none_invalid": (rng.integers(0, N_ITEMS, size=N_USERS), rng.integers(0, N_ITEMS, size=N_USERS))}
    aug = {k: tuple(torch.tensor(x, dtype=torch.int64, device=DEV) for x in v) for k, v in aug.items()}
    return ops, csr, torch.tensor(exist, dtype=torch.int64, device=DEV), aug


def _buffers(B, n_aug):
    u, p, n = (torch.full((B + n_aug + TAIL,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
    return u, p, n, torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)


def _compare(ops, csr, exist, seed, step, B_global, begin, B, n_aug, ap, an, calls=1):
    ref, new = _buffers(B, n_aug), _buffers(B, n_aug)
    s_ref = torch.tensor([step], dtype=torch.int64, device=DEV)
    s_new = s_ref.clone()
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for c in range(calls):
        ops.sample_batch(seed, s_ref, exist, N_ITEMS, csr, B_global, begin, B, n_aug, ap, an, *ref)
        ops.sample_batch_wide(seed, s_new, exist, N_ITEMS, csr, B_global, begin, B, n_aug, ap, an, *new, ticket)
        torch.cuda.synchronize()
        what = (seed, step, B_global, begin, B, n_aug, c)
        nv = int(ref[3])
        assert int(new[3]) == nv and B <= nv <= B + n_aug, what
        assert int(s_new) == int(s_ref) == step + c + 1 and int(ticket) == 0, what
        for a, b in zip(ref[:3], new[:3]):
            assert torch.equal(a[:nv], b[:nv]), what
            assert not bool(b[nv:B + n_aug].any()) and bool((b[B + n_aug:] == SENTINEL).all()), what
    return nv


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 257, 1024])
def test_wide_sampler_equals_the_single_block_sampler(world, B):
    ops, csr, exist, aug = world
    kept = {}
    for n_aug in (0, 1, 102, 300):
        if n_aug > B:
            continue
        for kind, (ap, an) in aug.items():
            if n_aug == 0 and kind != "mixed":
                continue
            nv = _compare(ops, csr, exist, 2022 + B, 5, B, 0, B, n_aug, ap if n_aug else None, an if n_aug else None)
            kept[(n_aug, kind)] = nv - B
    for (n_aug, kind), k in kept.items():
        if kind == "all_invalid":
            assert k == 0
        if kind == "none_invalid":
            assert k == n_aug


def test_wide_sampler_slices_replacement_and_consecutive_calls(world):
    ops, csr, exist, aug = world
    ap, an = aug["mixed"]
    _compare(ops, csr, exist, 9, 2 ** 32 + 7, 1024, 300, 257, 102, ap, an)               # slice_begin != 0, mid-wavefront
    _compare(ops, csr, exist, 9, 0, 64, 63, 1, 1, ap, an)
    few = exist[:40]
    _compare(ops, csr, few, 11, 3, 300, 0, 300, 102, ap, an)                             # B_global > n_exist: users drawn with replacement
    _compare(ops, csr, few, 11, 3, 300, 43, 257, 102, ap, an)
    _compare(ops, csr, exist, 2022, 0, 1024, 0, 1024, 102, ap, an, calls=3)              # three calls in a row: the counter and the ticket


def test_wide_sampler_in_a_replayed_graph(world):
    ops, csr, exist, aug = world
    ap, an = aug["mixed"]
    B, n_aug = 1024, 102
    new = _buffers(B, n_aug)
    step = torch.tensor([40], dtype=torch.int64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture
        ops.sample_batch_wide(2022, step, exist, N_ITEMS, csr, B, 0, B, n_aug, ap, an, *new, ticket)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(step) == 41 and int(ticket) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_batch_wide(2022, step, exist, N_ITEMS, csr, B, 0, B, n_aug, ap, an, *new, ticket)
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(step) == 42 + r and int(ticket) == 0
        ref = _buffers(B, n_aug)
        s_ref = torch.tensor([41 + r], dtype=torch.int64, device=DEV)
        ops.sample_batch(2022, s_ref, exist, N_ITEMS, csr, B, 0, B, n_aug, ap, an, *ref)
        torch.cuda.synchronize()
        nv = int(ref[3])
        assert int(new[3]) == nv
        for a, b in zip(ref[:3], new[:3]):
            assert torch.equal(a[:nv], b[:nv]), r
