"""Ranking per-query candidate lists (csrc/candidates.hip, ops.score_topk_candidates, Recommender.rank / rank_new, recommend.py
--candidates), the parts that need no device: the numpy restatement against one hand-written record, the C ABI and its argument checks,
the workspace formula, the kernels' resources, the host normalisation of `candidates` and the script's arguments."""
import ctypes

import numpy as np
import pytest
import torch

from llmrec_amd import _lib, build
from llmrec_amd._lib import CONST
from tests import _candidates_ref as C
from tests import _serve_ref as R
from tests._hipcc import needs_hipcc, resource_usage
from tests.test_exclude_ref_cpu import ALLOW, EXCL_ROWS, QUERY, TRAIN_ROWS, _csr

ENTRIES = ("llmrec_score_topk_candidates_workspace_bytes", "llmrec_score_topk_candidates_f32")

# the 8 items, the filter (eligible: 1 2 4 7), the train rows, the queries (3 0 3 1) and the exclusion rows of tests/test_exclude_ref_cpu.py
CAND_ROWS = [[5, 2, 1, 1, -1, 8, 3, 6, 0],     # 1 twice; -1; 8 >= n_items; 3 ineligible; 2 a train item of user 3; 1 and 3 excluded -> 0 5 6
             [4, 7, 7, 2, 9],                  # 4 a train item of user 0 -> 2 7
             [],
             [7, 6, 5, 4, 3, 2, 1, 0]]         # train 0 3 5, excluded 0 5 4 -> 1 2 6 7
SCORES = np.array([[0, 0, 0.25, 0, 0, 0, 0, 0.25],             # user 0: items 2 and 7 tie
                   [0, 0.5, 0.5, 0, 0, 0, -1.0, 2.0],          # user 1: items 1 and 2 tie
                   [0, 0, 0, 0, 0, 0, 0, 0],
                   [-0.5, 3.0, 1.0, 1.0, 9.0, 1.5, 0.0, 9.0]], dtype=np.float32)
NINF = -np.inf


def test_the_restatement_against_the_hand_written_record():
    trp, tci = _csr(TRAIN_ROWS)
    erp, eci = _csr(EXCL_ROWS)
    crp, cci = _csr(CAND_ROWS)
    new_id, _, _ = R.id_maps(ALLOW)
    assert C.candidate_set(CAND_ROWS[0], 8).tolist() == [0, 1, 2, 3, 5, 6]
    assert C.candidate_set(CAND_ROWS[0], 8, new_id).tolist() == [1, 2]
    assert C.survivors(CAND_ROWS[0], 8, TRAIN_ROWS[3], EXCL_ROWS[0]).tolist() == [0, 5, 6]
    assert C.survivors(CAND_ROWS[3], 8, TRAIN_ROWS[1], EXCL_ROWS[3], new_id).tolist() == [1, 2, 7]
    ids, sc = C.topk_candidates(SCORES, QUERY, trp, tci, 3, crp, cci, erp, eci)
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    assert ids.tolist() == [[5, 6, 0], [2, 7, -1], [-1, -1, -1], [7, 1, 2]]                          # ties by id
    assert sc.tolist() == [[1.5, 0.0, -0.5], [0.25, 0.25, NINF], [NINF] * 3, [2.0, 0.5, 0.5]]
    ids, sc = C.topk_candidates(SCORES, QUERY, trp, tci, 3, crp, cci, erp, eci, new_id)             # under the filter
    assert ids.tolist() == [[-1, -1, -1], [2, 7, -1], [-1, -1, -1], [7, 1, 2]]
    ids, sc = C.topk_candidates(SCORES, QUERY, None, None, 8, crp, cci)                             # no train side, no exclusion rows
    assert ids[0].tolist() == [1, 5, 2, 3, 6, 0, -1, -1] and sc[0].tolist() == [3.0, 1.5, 1.0, 1.0, 0.0, -0.5, NINF, NINF]
    assert ids[1].tolist() == [2, 7, 4, -1, -1, -1, -1, -1]
    assert ids[3].tolist() == [7, 1, 2, 0, 3, 4, 5, 6]
    ids1, _ = C.topk_candidates(SCORES, QUERY, trp, tci, 1, crp, cci, erp, eci)
    assert ids1.tolist() == [[5], [2], [-1], [7]]
    # order and repeats of a row do not matter
    again = _csr([r[::-1] + r for r in CAND_ROWS])
    a = C.topk_candidates(SCORES, QUERY, trp, tci, 5, crp, cci, erp, eci)
    b = C.topk_candidates(SCORES, QUERY, trp, tci, 5, again[0], again[1], erp, eci)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_entries_are_declared_and_exported_and_the_abi_stays():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(lib, name), name
    assert protos["llmrec_score_topk_candidates_workspace_bytes"][2] == ["n_query", "K", "cand_nnz", "excl_nnz"]
    assert protos["llmrec_score_topk_candidates_workspace_bytes"][0] is ctypes.c_int64
    assert protos["llmrec_score_topk_candidates_f32"][2] == [
        "n_query", "query_users", "Eu", "ldu", "Ei", "ldi", "n_items", "d", "train_rowptr", "train_colidx", "K", "out_idx", "out_score", "workspace",
        "workspace_bytes", "cand_rowptr", "cand_colidx", "cand_nnz", "excl_rowptr", "excl_colidx", "excl_nnz", "new_id", "stream"]
    # the excluded call keeps its signature
    wide = protos["llmrec_score_topk_wide_f32"][2]
    assert protos["llmrec_score_topk_excluded_f32"][2] == wide[:-1] + ["excl_rowptr", "excl_colidx", "excl_nnz", "new_id", "old_id", "n_kept_dev", "n_kept",
                                                                      wide[-1]]
    assert CONST["LLMREC_ABI_VERSION"] == 8 and _lib.load().llmrec_abi_version() == 8
    assert "candidates.hip" in build.SOURCES


def test_workspace_formula_restated():
    ws = lambda *a: _lib.query("llmrec_score_topk_candidates_workspace_bytes", *a)
    for n in (1, 70, 13187, 65536):
        for K in (1, 20, 1500, 30000):
            for cnnz in (0, 1, 63, 64, 2 ** 20 + 1, 13_107_200, (1 << 31) - 1):
                for ennz in (0, 1, 10 ** 4, 3 * 10 ** 6):
                    assert ws(n, K, cnnz, ennz) == C.workspace_bytes(n, K, cnnz, ennz) >= 0, (n, K, cnnz, ennz)
    assert ws(0, 20, 100, 5) == 0 and ws(70, 20, 0, 5) == 0        # nothing to rank: no workspace
    assert ws(70, 20, 1000, 0) == 256 + 2 * 8192 + 2 * 4096 + R.A(1000 + (32 << 20))
    assert ws(70, 20, 1000, 10) == ws(70, 20, 1000, 0) + 2 * 256 + R.A(10 + (32 << 20))
    assert ws(70, 1500, 1000, 0) == ws(70, 20, 1000, 0)            # nothing is sized by K
    for bad in ((-1, 20, 10, 0), (4, 0, 10, 0), (4, -2, 10, 0), (4, 20, -1, 0), (4, 20, 10, -1), (4, 20, 1 << 31, 0), (4, 20, 10, 1 << 31),
                (1 << 20, 1 << 11, 10, 0), (65536, 32768, 10, 0)):
        assert ws(*bad) == -1 == C.workspace_bytes(*bad), bad
    assert ws(65536, 32767, 10, 0) > 0                              # n_query * K one row below 2^31


def _candidates(lib, n_query=4, q=0x1000, Eu=0x2000, Ei=0x3000, d=64, ld=64, n_items=500, K=20, ws=None, ws_bytes=0, rowptr=None, colidx=None,
                crp=0xC000, cci=0xD000, cand_nnz=40, erp=0xA000, eci=0xB000, excl_nnz=10, new_id=0x6000):
    return lib.llmrec_score_topk_candidates_f32(n_query, q, Eu, ld, Ei, ld, n_items, d, rowptr, colidx, K, 0x4000, 0x5000, ws, ws_bytes,
                                                crp, cci, cand_nnz, erp, eci, excl_nnz, new_id, None)


def test_argument_checks_run_without_a_device():
    lib = _lib.load()
    err = lib.llmrec_last_error
    EINVAL = CONST["LLMREC_EINVAL"]
    assert EINVAL == -1
    for K in (0, -3):
        assert _candidates(lib, K=K) == EINVAL and b"score_topk_candidates" in err()
    for d in (0, 129):
        assert _candidates(lib, d=d, ld=129) == EINVAL and b"score_topk_candidates" in err() and b"128" in err()
    assert _candidates(lib, n_query=1 << 20, K=1 << 11) == EINVAL and b"score_topk_candidates" in err() and b"2^31" in err()
    assert _candidates(lib, n_query=65536, K=32768) == EINVAL and b"2^31" in err()
    assert _candidates(lib, cci=None) == EINVAL and b"score_topk_candidates" in err() and b"cand_colidx" in err()
    assert _candidates(lib, crp=None) == EINVAL and b"cand_rowptr" in err()
    assert _candidates(lib, cand_nnz=-1) == EINVAL and b"cand_nnz" in err()
    assert _candidates(lib, cand_nnz=1 << 31) == EINVAL and b"cand_nnz" in err()
    assert _candidates(lib, excl_nnz=-1) == EINVAL and b"excl_nnz" in err()
    assert _candidates(lib, eci=None) == EINVAL and b"excl_colidx" in err()
    assert _candidates(lib, erp=None) == EINVAL and b"excl_rowptr" in err()
    assert _candidates(lib, n_items=0) == EINVAL and _candidates(lib, n_items=1 << 31) == EINVAL
    assert _candidates(lib, Ei=None) == EINVAL and b"null pointer" in err()
    assert _candidates(lib, ld=63) == EINVAL and b"ld < d" in err()
    assert _candidates(lib, rowptr=0x9000) == EINVAL and b"train CSR incomplete" in err()
    assert _candidates(lib, colidx=0x9000) == EINVAL and b"train CSR incomplete" in err()
    for kw in (dict(), dict(erp=None, eci=None, excl_nnz=0), dict(new_id=None)):
        assert _candidates(lib, ws=None, **kw) == EINVAL and b"workspace" in err()
        assert _candidates(lib, ws=0x10008, ws_bytes=1 << 40, **kw) == EINVAL and b"aligned" in err()
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    for K in (20, 5000):
        for kw in (dict(), dict(erp=None, eci=None, excl_nnz=0)):
            need = _lib.query("llmrec_score_topk_candidates_workspace_bytes", 4, K, 40, kw.get("excl_nnz", 10))
            assert need > 4096
            assert _candidates(lib, K=K, ws=base, ws_bytes=4096, **kw) == CONST["LLMREC_EWORKSPACE"] and b"score_topk_candidates" in err()
            assert _candidates(lib, K=K, ws=base, ws_bytes=need - 1, **kw) == CONST["LLMREC_EWORKSPACE"] and str(need).encode() in err()
    assert _candidates(lib, n_query=0) == 0                        # nothing to do: no launch


@needs_hipcc
def test_no_kernel_of_candidates_hip_uses_scratch():
    res = resource_usage("candidates.hip")
    names = ("cd_open_kernel", "cd_keys_kernel", "cd_score_kernelILi4", "cd_write_kernel")
    for name in names:
        assert [k for k in res if name in k], name
    ours = {k: r for k, r in res.items() if "rocprim" not in k and "hipcub" not in k}      # (the vendor radix sort keeps private arrays)
    assert len(ours) == len(names), sorted(ours)
    assert len(res) > len(ours)                                    # the sorts' kernels are in this file
    for kernel, r in ours.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (kernel, r)


def test_the_accepted_forms_of_candidates():
    from llmrec_amd.serve import exclusion_csr
    users = [5, 2, 5, 0]
    want_rp, want_ci = [0, 3, 3, 6, 7], [9, 1, 1, 9, 1, 1, 4]
    forms = {
        "dict": {5: [9, 1, 1], 0: np.array([4]), 7: [3]},          # user 2 has no key: an empty list
        "sequences": [[9, 1, 1], [], (9, 1, 1), torch.tensor([4])],
        "pair": (np.array([0, 3, 3, 6, 7]), [9, 1, 1, 9, 1, 1, 4]),
        "array": np.array([[9, 1, 1], [-1, -1, -1], [9, 1, 1], [4, -1, -1]]),
    }
    for name, form in forms.items():
        rp, ci = exclusion_csr(form, users, 10, what="candidates")
        assert rp.dtype == np.int32 and ci.dtype == np.int32, name
        assert rp.tolist() == want_rp and ci.tolist() == want_ci, name
    for bad, match in (([[1], [2]], "candidates: 2 rows for 4 users"), (np.zeros((3, 2), np.int64), "candidates: 3 rows for 4 users"),
                       ({5: [10]}, r"candidates: ids must lie in \[0, 10\)"), ((np.array([0, 1, 2]), [1, 2]), "candidates: rowptr of 3 entries"),
                       ((np.array([0, 2, 1, 2, 2]), [1, 2]), "candidates: rowptr must rise"), ([[1.5], [], [], []], r"candidates\[0\]: integer"),
                       ({5: [0.5]}, r"candidates\[5\]: integer"), (np.arange(4), "candidates: a dict"), (7, "candidates: a dict")):
        with pytest.raises(ValueError, match=match):
            exclusion_csr(bad, users, 10, what="candidates")


def test_the_script_takes_candidates_and_behaves_as_before_without():
    import recommend
    argv = ["--dataset", "netflix_valid_item", "--checkpoint", "c.ckpt", "--embed_size", "32", "--users", "u.txt", "--topk", "20", "--debug",
            "--candidates", "cand.txt", "--exclude", "pairs.txt", "--out", "o.npz", "--Ks", "[10, 20]", "--mask_rate", "0"]
    rest_want = ["--dataset", "netflix_valid_item", "--embed_size", "32", "--debug", "--Ks", "[10, 20]", "--mask_rate", "0"]
    own, rest = recommend.split_argv(argv)
    assert own.candidates == "cand.txt" and own.exclude == "pairs.txt" and (own.checkpoint, own.users, own.topk, own.out) == ("c.ckpt", "u.txt", 20, "o.npz")
    assert rest == rest_want                                       # untouched, in order
    own, rest = recommend.split_argv([a for a in argv if a not in ("--candidates", "cand.txt")])
    assert own.candidates is None and own.exclude == "pairs.txt" and rest == rest_want
    own, _ = recommend.split_argv(["--checkpoint", "c", "--histories", "h", "--topk", "2000", "--out", "o", "--candidates", "x"])
    assert own.candidates == "x" and own.histories == "h" and own.users is None and own.topk == 2000
    # no abbreviation of --candidates is this script's: it goes on to the drop-in's parser
    own, rest = recommend.split_argv(["--checkpoint", "c", "--users", "u", "--topk", "1", "--out", "o", "--cand", "x", "--candidate", "y"])
    assert own.candidates is None and rest == ["--cand", "x", "--candidate", "y"]
