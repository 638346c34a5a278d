"""CPU tests of the full-rank AUC contract (llmrec_score_auc_f32, --test_flag full): the integer pair count of tests/_auc_ref.py against the
reference's roc_auc_score path, and the new entry points' argument checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest

from llmrec_amd import _lib
from tests._auc_ref import auc_counts, reference_auc


def _case(rng, n_items, n_train, n_held, levels=None):
    s = (rng.integers(0, levels, n_items) / 4.0 if levels else rng.standard_normal(n_items)).astype(np.float32)
    train = np.sort(rng.choice(n_items, n_train, replace=False))
    held = np.sort(rng.integers(-2, n_items + 2, n_held))                 # duplicates, out-of-range ids and train items included
    return s, train, held


@pytest.mark.parametrize("levels", [None, 3, 40])
def test_pair_count_equals_roc_auc_score(levels):
    rng = np.random.default_rng(7 + (levels or 0))
    for _ in range(20):
        n = int(rng.integers(5, 300))
        s, train, held = _case(rng, n, int(rng.integers(0, n // 2)), int(rng.integers(1, 40)), levels)
        c2, n_p, n_n, auc = auc_counts(s, train, held, n)
        assert 0 <= c2 <= 2 * n_p * n_n
        ref = reference_auc(s, train, held, n)
        if ref is None:
            pytest.skip("sklearn is not installed")
        assert abs(auc - ref) <= 1e-12, (auc, ref)


def test_signed_zeros_tie_and_one_class_and_non_finite_give_zero():
    s = np.array([0.0, -0.0, 1.0, -1.0, 0.0], dtype=np.float32)
    c2, n_p, n_n, auc = auc_counts(s, [], [1], 5)                          # -0.0 positive ties with the two +0.0 negatives
    assert (c2, n_p, n_n) == (2 * 1 + 2 * 1, 1, 4) and auc == 4 / 8
    assert auc_counts(s, [], [], 5)[3] == 0.0                              # one class: no positive
    assert auc_counts(s, [], [0, 1, 2, 3, 4], 5)[3] == 0.0                 # one class: no negative
    assert auc_counts(s, [0, 1, 2, 3, 4], [2], 5)[1:] == (0, 0, 0.0)       # every item in train
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy(); t[3] = bad
        assert auc_counts(t, [], [2], 5) == (0, 1, 4, 0.0)
        assert auc_counts(t, [3], [2], 5)[3] == 1.0                        # a train item's score does not count
        ref = reference_auc(t, [], [2], 5)
        assert ref is None or ref == 0.0                                   # roc_auc_score raises -> metrics.auc returns 0
    ref = reference_auc(s, [], [1], 5)
    assert ref is None or abs(ref - 0.5) <= 1e-12


def test_argument_errors_of_score_auc():
    lib = _lib.load()
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8 and lib.llmrec_abi_version() == 8
    assert lib.llmrec_score_auc_workspace_bytes(-1, 10, 64) == -1
    assert lib.llmrec_score_auc_workspace_bytes(100, 0, 64) == -1
    assert lib.llmrec_score_auc_workspace_bytes(100, 10, 64) > 0
    p = ctypes.c_void_p(16)                                                # never dereferenced: every case fails validation first
    ws = lib.llmrec_score_auc_workspace_bytes(4, 100, 64)
    cases = [
        ((4, p, p, 64, p, 64, 100, 48 + 8, None, None, p, p, None, None, None, p, ws, None), b"multiple of 16"),
        ((4, p, p, 144, p, 144, 100, 144, None, None, p, p, None, None, None, p, ws, None), b"at most 128"),
        ((4, p, p, 64, p, 64, 0, 64, None, None, p, p, None, None, None, p, ws, None), b"bad sizes"),
        ((4, p, p, 64, p, 64, 100, 64, p, None, p, p, None, None, None, p, ws, None), b"train CSR"),
        ((4, p, p, 64, p, 64, 100, 64, None, None, None, p, None, None, None, p, ws, None), b"null pointer"),
        ((4, p, p, 32, p, 64, 100, 64, None, None, p, p, None, None, None, p, ws, None), b"ld < d"),
        ((4, p, p, 64, p, 64, 100, 64, None, None, p, p, None, None, None, p, ws - 1, None), b"workspace"),
        ((4, p, p, 64, p, 64, 100, 64, None, None, p, p, None, None, None, None, ws, None), b"workspace"),
    ]
    for args, needle in cases:
        st = lib.llmrec_score_auc_f32(*args)
        assert st != 0, needle
        assert needle in lib.llmrec_last_error(), (needle, lib.llmrec_last_error())
    st = lib.llmrec_score_auc_f32(4, p, p, 64, p, 64, 100, 64, None, None, p, p, None, None, None, p, ws - 1, None)
    assert st == _lib.CONST.get("LLMREC_EWORKSPACE", -3)
