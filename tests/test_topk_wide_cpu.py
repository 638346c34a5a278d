"""Cut-offs above 64 (llmrec_score_topk_wide_f32), the parts that need no device: the C ABI, the argument checks, the workspace query and the
argument the rounds design rests on - ranks [c p, c (p + 1)) are the top c of (candidates minus the first c p items)."""
import ctypes

import numpy as np
import pytest

from llmrec_amd import _lib
from llmrec_amd._lib import CONST


def test_header_and_library_carry_the_wide_entry_points():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("llmrec_score_topk_wide_workspace_bytes", "llmrec_score_topk_wide_f32"):
        assert name in protos, name
        assert hasattr(lib, name), name
    # the arguments of llmrec_score_topk_mode_f32 with train_nnz in front of the stream
    names = protos["llmrec_score_topk_wide_f32"][2]
    ref = protos["llmrec_score_topk_mode_f32"][2]
    assert names == ref[:-1] + ["train_nnz", ref[-1]]
    assert "llmrec_topk_eval_sums_wide" not in protos           # the wide evaluation sums sit behind llmrec_topk_eval_sums
    assert CONST["LLMREC_TOPK_WIDE_MAX"] == 1024
    assert CONST["LLMREC_TOPK_MAX"] == 64 and CONST["LLMREC_TOPK_PREFILTER_MAX_K"] == 56
    assert CONST["LLMREC_ABI_VERSION"] == 8


def _wide(lib, n_query=4, q=0x1000, Eu=0x2000, Ei=0x3000, K=100, ws=None, ws_bytes=0, mode=0, train_nnz=0, d=64, n_items=500):
    return lib.llmrec_score_topk_wide_f32(n_query, q, Eu, d, Ei, d, n_items, d, None, None, K, 0x4000, 0x5000, ws, ws_bytes, mode, train_nnz, None)


def test_argument_checks_run_without_a_device():
    lib = _lib.load()
    for K in (0, -3, 1025, 4096):
        assert _wide(lib, K=K) == -1, K
        msg = lib.llmrec_last_error()
        assert b"score_topk_wide" in msg and b"1024" in msg, msg
    assert _wide(lib, Ei=None) == -1 and b"score_topk_wide" in lib.llmrec_last_error()
    assert _wide(lib, Eu=None, K=10) == -1 and b"score_topk_wide" in lib.llmrec_last_error()
    assert _wide(lib, mode=2) == -1 and b"score_topk_wide" in lib.llmrec_last_error()
    assert _wide(lib, K=100, ws=None) == -1 and b"workspace" in lib.llmrec_last_error()               # K > 64 cannot run without one
    assert _wide(lib, K=100, ws=0x10008, ws_bytes=1 << 40) == -1 and b"aligned" in lib.llmrec_last_error()
    assert _wide(lib, K=100, ws=0x10000, ws_bytes=1 << 40, train_nnz=-1) == -1
    assert _wide(lib, n_query=1 << 22, K=1024, ws=0x10000, ws_bytes=1 << 50) == -1                     # 2^32 mask entries
    buf = ctypes.create_string_buffer(4096)
    for K in (50, 100, 1024):                                                                           # a workspace that is too small: -3, on both routes
        need = _lib.query("llmrec_score_topk_wide_workspace_bytes", 4, 500, 64, K, 0)
        assert need > 4096
        assert _wide(lib, K=K, ws=ctypes.addressof(buf), ws_bytes=4096) == -3, K
        assert b"score_topk_wide" in lib.llmrec_last_error()
        assert _wide(lib, K=K, ws=ctypes.addressof(buf), ws_bytes=need - 1) == -3, K
    assert _wide(lib, n_query=0, K=100) == 0                                                           # nothing to do: no launch
    # the single-sweep entry keeps its limit and its message
    st = lib.llmrec_score_topk_mode_f32(4, 0x1000, 0x2000, 64, 0x3000, 64, 500, 64, None, None, 65, 0x4000, 0x5000, None, 0, 0, None)
    assert st == -1 and b"score_topk: bad sizes (K <= 64)" in lib.llmrec_last_error()
    # evaluation sums: K up to 1024 passes the size check (the next check, a null list, answers), beyond it does not
    ks = (ctypes.c_int32 * 2)(10, 200)
    out = ctypes.create_string_buffer(64)
    fn = lib.llmrec_topk_eval_sums
    assert fn(4, 0x1000, 1025, 0x2000, 0x3000, 0x4000, 2, ks, 0x10000, 1 << 20, ctypes.addressof(out), None) == -1
    assert b"bad sizes (K <= 1024" in lib.llmrec_last_error(), lib.llmrec_last_error()
    assert fn(4, 0x1000, 1024, None, 0x3000, 0x4000, 2, ks, 0x10000, 1 << 20, ctypes.addressof(out), None) == -1
    assert b"null pointer" in lib.llmrec_last_error()
    assert fn(4, 0x1000, 200, 0x2000, 0x3000, 0x4000, 2, ks, 0x10000, 8, ctypes.addressof(out), None) == -3


def test_workspace_query_restated():
    """llmrec_score_topk_wide_workspace_bytes: the single-sweep workspace up to K = 64; beyond, the formula of the header, restated."""
    up = lambda x: -(-x // 256) * 256
    def extra(n, d, K, nnz):
        d4 = -(-d // 4) * 4
        return up(4 * n * d4) + up(8 * n) + 2 * up(4 * (n + 1)) + up(4 * n) + 256 + 2 * up(4 * (nnz + n * K)) + 2 * up(4 * 64 * n)
    wide = lambda *a: _lib.query("llmrec_score_topk_wide_workspace_bytes", *a)
    for n, items, d, nnz in ((13187, 17366, 64, 68933), (100, 500, 20, 0), (65536, 1_000_000, 64, 3_000_000), (37, 3000, 128, 555), (0, 10, 16, 0)):
        base = _lib.query("llmrec_score_topk_workspace_bytes", n, items, d)
        assert base > 0
        last = 0
        for K in (1, 50, 56, 57, 64, 65, 100, 112, 113, 200, 1000, 1024):
            got = wide(n, items, d, K, nnz)
            assert got == (base if K <= 64 else up(base) + extra(n, d, K, nnz)), (n, items, d, K)
            assert got >= last                                     # monotone in K
            last = got
        assert wide(n, items, d, 100, nnz + 1000) >= wide(n, items, d, 100, nnz)
    for bad in ((-1, 10, 64, 100, 0), (4, 0, 64, 100, 0), (4, 10, 0, 100, 0), (4, 10, 64, 0, 0), (4, 10, 64, 1025, 0), (4, 10, 64, 100, -1),
                (1 << 22, 10, 64, 1024, 0), (4, 10, 64, 100, 1 << 31)):
        assert wide(*bad) == -1, bad


def _rounds(scores, train_row, K, c):
    """The rule llmrec_score_topk_wide_f32 runs, in numpy: take the best c of the unmasked items by (score desc, id asc), join them to the mask,
    repeat. The mask is kept as the library keeps it: an ascending list, duplicates of the train row included."""
    n_items = scores.shape[0]
    mask = np.sort(np.asarray(train_row, dtype=np.int64))
    out_idx = np.full(K, -1, dtype=np.int64)
    out_sc = np.full(K, -np.inf, dtype=np.float32)
    for col in range(0, K, c):
        kp = min(c, K - col)
        assert np.all(np.diff(mask) >= 0)
        cand = np.setdiff1d(np.arange(n_items), mask)
        order = cand[np.lexsort((cand, -scores[cand].astype(np.float64)))][:kp]
        out_idx[col:col + len(order)] = order
        out_sc[col:col + len(order)] = scores[order]
        # the merge of tw_merge_kernel: old entry i -> i + #(new < entry); new id j (ascending) -> j + #(old <= id)
        new = np.sort(order)
        merged = np.empty(len(mask) + len(new), dtype=np.int64)
        merged[np.arange(len(mask)) + np.searchsorted(new, mask, side="left")] = mask
        merged[np.arange(len(new)) + np.searchsorted(mask, new, side="right")] = new
        mask = merged
    return out_idx, out_sc


@pytest.mark.parametrize("c", [56, 64])
def test_rounds_rule_equals_one_sort_over_the_row(c):
    rng = np.random.default_rng(20260 + c)
    for trial in range(40):
        n_items = int(rng.integers(1, 700))
        kind = trial % 4
        if kind == 0:
            scores = rng.integers(-3, 4, n_items).astype(np.float32)               # heavy ties
        elif kind == 1:
            scores = np.zeros(n_items, dtype=np.float32)                           # all equal
            scores[rng.integers(0, n_items, n_items // 2)] = -0.0
        elif kind == 2:
            scores = np.round(rng.standard_normal(n_items), 1).astype(np.float32)
        else:
            scores = rng.standard_normal(n_items).astype(np.float32)
        n_train = int(rng.integers(0, n_items + 1)) if trial % 5 else n_items      # sometimes every item is a train item
        train = rng.integers(0, n_items, n_train)                                  # duplicates included, unsorted
        for K in (65, 100, 113, 200, 1024):
            idx, sc = _rounds(scores, train, K, c)
            cand = np.setdiff1d(np.arange(n_items), train)
            want = cand[np.lexsort((cand, -scores[cand].astype(np.float64)))][:K]
            assert np.array_equal(idx[:len(want)], want), (trial, K)
            assert np.all(idx[len(want):] == -1) and np.all(np.isneginf(sc[len(want):]))
            assert np.array_equal(sc[:len(want)].view(np.uint32), scores[want].view(np.uint32))
