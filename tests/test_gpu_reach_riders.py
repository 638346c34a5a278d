"""GPU: the two launches that carry the weight gradient's reach list as riders, against the calls they replace, with torch.equal:
llmrec_bpr_scatter_plan_reach_mark = llmrec_bpr_scatter_plan + the marking half of llmrec_batch_reach_rows;
llmrec_fuse_fwd_multi_sumsq_compact_f32 = llmrec_fuse_fwd_multi_sumsq_f32 + the compacting half (list, count, all-zero scratch).
The marking half leaves nothing behind on its own (the compaction clears the flags), so its reference is the list it leads to."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
p_ = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
N_USERS = [1, 15, 16, 17, 255, 256, 257, 4097, 16385]
N_ITEMS, D, S = 41, 64, 3
SENTINEL = -7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _flags(n):
    return torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=DEV)[:n]     # 16-byte aligned, readable in 16-byte words


def _by_item_csr(rng, n_users):
    """item -> its users; item 0 is a hub with more than 64 * 8 users where there are that many, the last item holds the last user"""
    rows = []
    for it in range(N_ITEMS):
        k = min(n_users, 600) if it == 0 else int(rng.integers(0, min(n_users, 9) + 1))
        us = np.sort(rng.choice(n_users, size=k, replace=False))
        if it == N_ITEMS - 1:
            us = np.union1d(us, [n_users - 1])
        rows.append(us.astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.concatenate(rows + [np.zeros(0, np.int32)]).astype(np.int32)
    if colidx.size == 0:
        colidx = np.zeros(1, np.int32)
    return torch.tensor(rowptr).to(DEV), torch.tensor(colidx).to(DEV)


def _fuse_problems(ops, tabs, outs, keep):
    arr = (ops.FuseFwdProblem * 2)()
    rates = (ctypes.c_float * S)(0.26, 0.26, 0.55)
    keep.append(rates)
    for k in range(2):
        cat, mean = tabs[k]
        norms = [cat[:, j * D:(j + 1) * D] for j in range(S)]
        mp = (ctypes.c_void_p * 1)(mean.data_ptr()); ml = (ctypes.c_int64 * 1)(D)
        npt = (ctypes.c_void_p * S)(*[t.data_ptr() for t in norms]); nl = (ctypes.c_int64 * S)(*[t.stride(0) for t in norms])
        keep.extend((mp, ml, npt, nl))
        pr = arr[k]
        pr.rows, pr.mean_scale, pr.n_mean, pr.n_norm = cat.shape[0], 1.0, 1, S
        pr.mean_terms, pr.mean_ld = ctypes.cast(mp, ctypes.c_void_p), ctypes.cast(ml, ctypes.c_void_p)
        pr.norm_terms, pr.norm_ld, pr.rates = ctypes.cast(npt, ctypes.c_void_p), ctypes.cast(nl, ctypes.c_void_p), ctypes.cast(rates, ctypes.c_void_p)
        pr.out, pr.ldo = outs[k].data_ptr(), outs[k].stride(0)
    return arr


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from llmrec_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("n_users", N_USERS)
def test_plan_and_marks_in_one_launch(ops, n_users):
    from llmrec_amd import _lib
    rng = np.random.default_rng(100 + n_users)
    rowptr, colidx = _by_item_csr(rng, n_users)
    cap, valid = 53, 37                                                  # n_valid < B_cap: the slots behind it are not read
    users = rng.integers(0, n_users, size=cap); pos = rng.integers(0, N_ITEMS, size=cap); neg = rng.integers(0, N_ITEMS, size=cap)
    users[0], pos[0], neg[1] = n_users - 1, N_ITEMS - 1, N_ITEMS - 1      # ids at the last row
    pos[2] = 0                                                           # the hub item
    neg[3], neg[4], pos[5] = N_ITEMS + 5, N_ITEMS, -1                    # out-of-range item ids: ignored by the marks
    users[valid:], pos[valid:], neg[valid:] = 0, 0, 0
    users, pos, neg = (torch.tensor(x).to(DEV) for x in (users, pos, neg))
    nv = torch.tensor([valid], dtype=torch.int32, device=DEV)
    words = 5 * cap                                                      # LLMREC_BPR_PLAN_WORDS
    plan_ref = torch.full((words,), SENTINEL, dtype=torch.int64, device=DEV)
    plan_new = plan_ref.clone()
    flags_ref, flags_new = _flags(n_users), _flags(n_users)
    list_ref = torch.full((n_users + 32,), SENTINEL, dtype=torch.int32, device=DEV)
    list_new = list_ref.clone()
    n_ref, n_new = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    st = _stream()
    _lib.call("llmrec_bpr_scatter_plan", p_(users), p_(pos), p_(neg), cap, p_(nv), p_(plan_ref), st)
    _lib.call("llmrec_batch_reach_rows", n_users, N_ITEMS, p_(users), p_(pos), p_(neg), cap, p_(nv), p_(rowptr), p_(colidx), p_(flags_ref),
              p_(list_ref), p_(n_ref), st)
    _lib.call("llmrec_bpr_scatter_plan_reach_mark", p_(users), p_(pos), p_(neg), cap, p_(nv), p_(plan_new), n_users, N_ITEMS, p_(rowptr),
              p_(colidx), p_(flags_new), st)
    torch.cuda.synchronize()
    assert torch.equal(plan_ref, plan_new)
    n = int(n_ref[0])
    assert n >= 1 and not bool(flags_ref.any())
    want = torch.zeros(n_users, dtype=torch.uint8, device=DEV)
    want[list_ref[:n].long()] = 1
    assert torch.equal((flags_new != 0).to(torch.uint8), want)
    if n_users > 600:
        assert n > 64 * 8                                                # the hub's adjacency list was walked by all eight parts
    # ... and the list from these marks, by the fusion launch's first block
    keep = []
    tabs = [(torch.randn(7, S * D, device=DEV), torch.randn(7, D, device=DEV)) for _ in range(2)]
    outs = [torch.empty(7, D, device=DEV) for _ in range(2)]
    partial = torch.zeros(64, device=DEV)
    n_part = ctypes.c_int32(0)
    _lib.call("llmrec_fuse_fwd_multi_sumsq_compact_f32", 2, _fuse_problems(ops, tabs, outs, keep), D, 2, p_(partial), 64, ctypes.byref(n_part),
              n_users, p_(flags_new), p_(list_new), p_(n_new), st)
    torch.cuda.synchronize()
    assert torch.equal(list_ref, list_new) and torch.equal(n_ref, n_new) and not bool(flags_new.any())


@pytest.mark.parametrize("density", ["none", "all", "some"])
@pytest.mark.parametrize("n_users", N_USERS)
def test_fusion_and_compaction_in_one_launch(ops, n_users, density):
    from llmrec_amd import _lib
    rng = np.random.default_rng(7 * n_users + len(density))
    f = {"none": np.zeros(n_users, bool), "all": np.ones(n_users, bool), "some": rng.random(n_users) < 0.4}[density]
    if density == "some":
        f[n_users - 1] = True                                            # the last row
    f = torch.tensor(f.astype(np.uint8) * rng.integers(1, 256, size=n_users).astype(np.uint8)).to(DEV)   # any non-zero byte is a mark
    rows = [37, n_users]                                                 # item side, user side
    tabs = [(torch.tensor(rng.standard_normal((r, S * D)).astype(np.float32)).to(DEV), torch.tensor(rng.standard_normal((r, D)).astype(np.float32)).to(DEV))
            for r in rows]
    rowptr = torch.zeros(N_ITEMS + 1, dtype=torch.int32, device=DEV); colidx = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = torch.zeros(1, dtype=torch.int64, device=DEV)
    res, keep, st = [], [], _stream()
    for new in (False, True):
        flags = _flags(n_users); flags.copy_(f)
        outs = [torch.full((r, D), float("nan"), device=DEV) for r in rows]
        partial = torch.full((4096,), float("nan"), device=DEV)
        lst = torch.full((n_users + 32,), SENTINEL, dtype=torch.int32, device=DEV)
        cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
        n_part = ctypes.c_int32(0)
        arr = _fuse_problems(ops, tabs, outs, keep)
        if new:
            _lib.call("llmrec_fuse_fwd_multi_sumsq_compact_f32", 2, arr, D, 2, p_(partial), 4096, ctypes.byref(n_part),
                      n_users, p_(flags), p_(lst), p_(cnt), st)
        else:
            _lib.call("llmrec_fuse_fwd_multi_sumsq_f32", 2, arr, D, 2, p_(partial), 4096, ctypes.byref(n_part), st)
            _lib.call("llmrec_batch_reach_rows", n_users, N_ITEMS, p_(ids), p_(ids), p_(ids), 0, None, p_(rowptr), p_(colidx), p_(flags),
                      p_(lst), p_(cnt), st)                              # an empty batch marks nothing: the compacting half alone
        torch.cuda.synchronize()
        res.append((outs[0], outs[1], partial, n_part.value, lst, cnt, flags))
    a, b = res
    assert a[3] == b[3] > 0
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert not bool(b[6].any())                                          # the scratch is all-zero again
    n = int(b[5][0])
    assert n == int((f != 0).sum()) and torch.equal(b[4][:n].long(), torch.nonzero(f).flatten())
    assert bool(torch.isfinite(b[2][:b[3]]).all())


def test_refused_shapes_launch_nothing(ops):
    from llmrec_amd import _lib
    big = _lib.CONST["LLMREC_BPR_MAX_B"] + 1
    n_users = 300
    ids = torch.zeros(big, dtype=torch.int64, device=DEV)
    plan = torch.full((5 * big,), SENTINEL, dtype=torch.int64, device=DEV)
    flags = _flags(n_users); flags[5] = 1
    rowptr = torch.arange(N_ITEMS + 1, dtype=torch.int32, device=DEV); colidx = torch.zeros(N_ITEMS, dtype=torch.int32, device=DEV)
    st = _stream()
    assert not _lib.call_unless_unsupported("llmrec_bpr_scatter_plan_reach_mark", p_(ids), p_(ids), p_(ids), big, None, p_(plan), n_users, N_ITEMS,
                                            p_(rowptr), p_(colidx), p_(flags), st)
    d = 66                                                               # rows that are not whole float4s: outside the compiled family
    keep = []
    tabs = [(torch.randn(9, S * d, device=DEV), torch.randn(9, d, device=DEV)) for _ in range(2)]
    outs = [torch.full((9, d), 3.0, device=DEV) for _ in range(2)]
    arr = (ops.FuseFwdProblem * 2)()
    rates = (ctypes.c_float * S)(0.26, 0.26, 0.55)
    for k in range(2):
        norms = [tabs[k][0][:, j * d:(j + 1) * d] for j in range(S)]
        mp = (ctypes.c_void_p * 1)(tabs[k][1].data_ptr()); ml = (ctypes.c_int64 * 1)(d)
        npt = (ctypes.c_void_p * S)(*[t.data_ptr() for t in norms]); nl = (ctypes.c_int64 * S)(*[t.stride(0) for t in norms])
        keep.extend((mp, ml, npt, nl))
        pr = arr[k]
        pr.rows, pr.mean_scale, pr.n_mean, pr.n_norm = 9, 1.0, 1, S
        pr.mean_terms, pr.mean_ld = ctypes.cast(mp, ctypes.c_void_p), ctypes.cast(ml, ctypes.c_void_p)
        pr.norm_terms, pr.norm_ld, pr.rates = ctypes.cast(npt, ctypes.c_void_p), ctypes.cast(nl, ctypes.c_void_p), ctypes.cast(rates, ctypes.c_void_p)
        pr.out, pr.ldo = outs[k].data_ptr(), d
    partial = torch.full((64,), 5.0, device=DEV)
    lst = torch.full((n_users + 32,), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    n_part = ctypes.c_int32(0)
    assert not _lib.call_unless_unsupported("llmrec_fuse_fwd_multi_sumsq_compact_f32", 2, arr, d, 2, p_(partial), 64, ctypes.byref(n_part),
                                            n_users, p_(flags), p_(lst), p_(cnt), st)
    torch.cuda.synchronize()
    assert bool((plan == SENTINEL).all()) and bool((lst == SENTINEL).all()) and int(cnt[0]) == SENTINEL
    assert int(flags.sum()) == 1 and int(flags[5]) == 1 and bool((partial == 5.0).all()) and all(bool((o == 3.0).all()) for o in outs)
