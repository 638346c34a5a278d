"""Recommending with per-query exclusion lists (csrc/exclude.hip, ops.score_topk_excluded, Recommender.recommend(exclude=...),
recommend.py --exclude), the parts that need no device: the numpy restatement of the merged mask rows against hand-written records, the
workspace formulas, the C ABI and its argument checks, the kernels' resources, the host normalisation of the accepted `exclude` forms and
the script's arguments."""
import ctypes

import numpy as np
import pytest
import torch

from llmrec_amd import _lib, build
from llmrec_amd._lib import CONST
from tests import _exclude_ref as X
from tests import _serve_ref as R
from tests._hipcc import needs_hipcc, resource_usage

ENTRIES = ("llmrec_score_topk_excluded_workspace_bytes", "llmrec_score_topk_excluded_mask_offset", "llmrec_score_topk_excluded_f32")

# one record, written by hand: the 8 items, the filter and the train rows of tests/test_serve_ref_cpu.py
ALLOW = np.array([0, 1, 255, 0, 1, 0, 0, 255], dtype=np.uint8)     # new_id = -1 0 1 -1 2 -1 -1 3
TRAIN_ROWS = [[1, 1, 3, 4],        # compact: 0 0 2
              [0, 3, 5],           # compact: nothing
              [],
              [2, 7, 7]]           # compact: 1 3 3
QUERY = [3, 0, 3, 1]               # unsorted, user 3 twice - with two different exclusion rows
EXCL_ROWS = [[7, 4, -1, 7, 9, 3, 1],   # unsorted; 7 twice; -1; 9 >= n_items; 3 ineligible; 7 is a train entry of user 3 -> compact 0 2 3 3
             [],
             [2],                      # a train entry of user 3 -> compact 1
             [0, 5, 4, 4]]             # 0 and 5 ineligible -> compact 2 2
MERGED_ROWPTR = [0, 7, 10, 14, 16]
MERGED_COLIDX = [0, 1, 2, 3, 3, 3, 3,      # train 1 3 3 + exclusions 0 2 3 3
                 0, 0, 2,                  # the train row alone
                 1, 1, 3, 3,               # train 1 3 3 + exclusion 1
                 2, 2]                     # exclusions alone
IDENT_ROWPTR = [0, 8, 12, 16, 23]
IDENT_COLIDX = [1, 2, 3, 4, 7, 7, 7, 7,    # train 2 7 7 + exclusions 1 3 4 7 7
                1, 1, 3, 4,
                2, 2, 7, 7,
                0, 0, 3, 4, 4, 5, 5]       # train 0 3 5 + exclusions 0 4 4 5


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.asarray([c for r in rows for c in r], dtype=np.int32)


def test_merged_rows_against_the_hand_written_record():
    trp, tci = _csr(TRAIN_ROWS)
    erp, eci = _csr(EXCL_ROWS)
    new_id, _, _ = R.id_maps(ALLOW)
    rp, ci = X.merged_rows(trp, tci, QUERY, erp, eci, new_id)
    assert rp.tolist() == MERGED_ROWPTR and ci.tolist() == MERGED_COLIDX
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    # the identity numbering: no filter
    rp, ci = X.merged_rows(trp, tci, QUERY, erp, eci, None, n_items=8)
    assert rp.tolist() == IDENT_ROWPTR and ci.tolist() == IDENT_COLIDX
    every, _, _ = R.id_maps(np.ones(8, np.uint8))                   # a filter that keeps every item numbers the items as they are
    rp2, ci2 = X.merged_rows(trp, tci, QUERY, erp, eci, every)
    assert rp2.tolist() == IDENT_ROWPTR and ci2.tolist() == IDENT_COLIDX
    # every exclusion row empty, or no exclusion CSR: the compact mask rows of the filtered call
    want = R.mask_rows(trp, tci, QUERY, new_id)
    for e in (_csr([[]] * 4), (None, None)):
        rp, ci = X.merged_rows(trp, tci, QUERY, e[0], e[1], new_id)
        assert rp.tolist() == want[0].tolist() and ci.tolist() == want[1].tolist()
    # no train side: the sorted kept exclusions
    rp, ci = X.merged_rows(None, None, QUERY, erp, eci, new_id)
    assert rp.tolist() == [0, 4, 4, 5, 7] and ci.tolist() == [0, 2, 3, 3, 1, 2, 2]
    none, _, _ = R.id_maps(np.zeros(8, np.uint8))                   # no eligible item: every row loses every entry
    rp, ci = X.merged_rows(trp, tci, QUERY, erp, eci, none)
    assert rp.tolist() == [0] * 5 and ci.size == 0


def test_merged_rows_are_ascending_and_keep_every_kept_entry():
    rng = np.random.default_rng(11)
    I, U, n = 300, 40, 70
    new_id, _, _ = R.id_maps((rng.random(I) < 0.5).astype(np.uint8))
    trp, tci = _csr([np.sort(rng.integers(0, I, rng.integers(0, 30))).tolist() for _ in range(U)])
    q = rng.integers(0, U, n)
    erp, eci = _csr([rng.integers(-1, I + 3, m).tolist() for m in rng.choice([0, 1, 63, 64, 65, 200], n)])
    for nid in (new_id, None):
        rp, ci = X.merged_rows(trp, tci, q, erp, eci, nid, n_items=I)
        for k in range(n):
            row = ci[rp[k]:rp[k + 1]]
            assert np.all(np.diff(row) >= 0)
            ids = np.concatenate([tci[trp[q[k]]:trp[q[k] + 1]], eci[erp[k]:erp[k + 1]]]).astype(np.int64)
            ids = ids[(ids >= 0) & (ids < I)]
            kept = ids if nid is None else nid[ids][nid[ids] >= 0]
            assert np.array_equal(np.sort(kept), row)


def test_entries_are_declared_and_exported_and_the_abi_stays():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(lib, name), name
    wide = protos["llmrec_score_topk_wide_f32"][2]
    assert wide[-2:] == ["train_nnz", "stream"]
    assert protos["llmrec_score_topk_excluded_f32"][2] == wide[:-1] + ["excl_rowptr", "excl_colidx", "excl_nnz", "new_id", "old_id", "n_kept_dev", "n_kept",
                                                                      wide[-1]]
    sizes = ["n_query", "n_items", "n_kept", "d", "K", "train_nnz", "excl_nnz"]
    assert protos["llmrec_score_topk_excluded_workspace_bytes"][2] == sizes and protos["llmrec_score_topk_excluded_mask_offset"][2] == sizes
    # the filtered call keeps its signature
    assert protos["llmrec_score_topk_filtered_f32"][2] == wide[:-1] + ["new_id", "old_id", "n_kept_dev", "n_kept", wide[-1]]
    assert CONST["LLMREC_ABI_VERSION"] == 8 and _lib.load().llmrec_abi_version() == 8
    assert "exclude.hip" in build.SOURCES and "serve.hip" in build.SOURCES


def test_workspace_formulas_restated():
    ws = lambda *a: _lib.query("llmrec_score_topk_excluded_workspace_bytes", *a)
    off = lambda *a: _lib.query("llmrec_score_topk_excluded_mask_offset", *a)
    for n, items, kept, d, nnz in ((13187, 17366, 1737, 64, 68933), (203, 3000, 3000, 20, 6000), (40, 6181, 37, 16, 0), (65536, 1_000_000, 100_000, 128, 3_000_000),
                                   (1, 1, 1, 1, 0), (0, 10, 5, 16, 0)):
        for K in (1, 20, 56, 64, 65, 130, 1024):
            for ennz in (0, 1, 10 ** 4, 3 * 10 ** 6):
                wide = _lib.query("llmrec_score_topk_wide_workspace_bytes", n, kept, d, K, nnz + ennz)
                assert wide >= 0
                assert ws(n, items, kept, d, K, nnz, ennz) == X.excluded_workspace_bytes(n, items, kept, d, nnz, ennz, wide), (n, items, kept, d, K, ennz)
                assert off(n, items, kept, d, K, nnz, ennz) == X.mask_offset(n, items, kept, d, nnz, ennz, wide)
                assert off(n, items, kept, d, K, nnz, ennz) + R.A(4 * (n + 1)) + R.A(4 * (nnz + ennz)) + 256 == ws(n, items, kept, d, K, nnz, ennz)
        assert ws(n, items, 0, d, 20, nnz, 5) == 0 and off(n, items, 0, d, 20, nnz, 5) == -1      # no eligible item: no sweep, no workspace
        assert ws(n, items, kept, d, 20, nnz, 1000) > ws(n, items, kept, d, 20, nnz, 0)
    for bad in ((-1, 10, 5, 64, 20, 0, 0), (4, 0, 0, 64, 20, 0, 0), (4, 10, 11, 64, 20, 0, 0), (4, 10, -1, 64, 20, 0, 0), (4, 10, 5, 0, 20, 0, 0),
                (4, 10, 5, 129, 20, 0, 0), (4, 10, 5, 64, 0, 0, 0), (4, 10, 5, 64, 1025, 0, 0), (4, 10, 5, 64, 20, -1, 0), (4, 10, 5, 64, 20, 0, -1),
                (4, 1 << 31, 5, 64, 20, 0, 0), (1 << 22, 10, 5, 64, 1024, 0, 0), (4, 10, 5, 64, 20, 0, 1 << 31),
                # the 2^31 sum, at every K: train_nnz + excl_nnz + n_query * K
                (4, 10, 5, 64, 20, (1 << 30), (1 << 30) - 80), (4, 10, 5, 64, 100, (1 << 30), (1 << 30) - 400), (1 << 20, 10, 5, 64, 1024, 1 << 29, 1 << 29)):
        assert ws(*bad) == -1 and off(*bad) == -1, bad
    assert ws(4, 10, 5, 64, 20, (1 << 30), (1 << 30) - 81) > 0      # one below the sum's limit


def _excluded(lib, n_query=4, q=0x1000, Eu=0x2000, Ei=0x3000, d=64, ld=64, n_items=500, K=20, ws=None, ws_bytes=0, mode=0, train_nnz=0,
              erp=0xA000, eci=0xB000, excl_nnz=10, new_id=0x6000, old_id=0x7000, n_kept_dev=0x8000, n_kept=100, rowptr=None, colidx=None):
    return lib.llmrec_score_topk_excluded_f32(n_query, q, Eu, ld, Ei, ld, n_items, d, rowptr, colidx, K, 0x4000, 0x5000, ws, ws_bytes, mode, train_nnz,
                                              erp, eci, excl_nnz, new_id, old_id, n_kept_dev, n_kept, None)


def test_argument_checks_run_without_a_device():
    lib = _lib.load()
    err = lib.llmrec_last_error
    nomaps = dict(new_id=None, old_id=None, n_kept_dev=None)
    for K in (0, -3, 1025):
        assert _excluded(lib, K=K) == -1 and b"score_topk_excluded" in err() and b"1024" in err()
    assert _excluded(lib, n_kept=-1) == -1 and b"n_kept" in err()
    assert _excluded(lib, n_kept=501) == -1 and b"n_kept" in err()
    assert _excluded(lib, mode=2) == -1 and b"mode" in err()
    assert _excluded(lib, Ei=None) == -1 and b"null pointer" in err()
    assert _excluded(lib, ld=63) == -1 and b"ld < d" in err()
    assert _excluded(lib, rowptr=0x9000) == -1 and b"train CSR incomplete" in err()
    assert _excluded(lib, colidx=0x9000) == -1 and b"train CSR incomplete" in err()
    assert _excluded(lib, excl_nnz=-1) == -1 and b"excl_nnz" in err()
    assert _excluded(lib, eci=None) == -1 and b"excl_colidx" in err()
    assert _excluded(lib, erp=None) == -1 and b"excl_rowptr" in err()
    for part in ("new_id", "old_id", "n_kept_dev"):                # maps partly null
        assert _excluded(lib, **{part: None}) == -1 and b"maps" in err(), part
        assert _excluded(lib, n_kept=500, **{k: v for k, v in nomaps.items() if k != part}) == -1 and b"maps" in err(), part
    assert _excluded(lib, **nomaps) == -1 and b"n_kept = 100 != n_items" in err()      # null maps with n_kept != n_items
    assert _excluded(lib, d=129, ld=129) == CONST["LLMREC_EUNSUPPORTED"]
    assert _excluded(lib, train_nnz=(1 << 31) - 50, rowptr=0x9000, colidx=0x9100) == -1 and b"2^31" in err()
    for kw in (dict(), dict(n_kept=500, **nomaps), dict(erp=None, eci=None, excl_nnz=0)):
        assert _excluded(lib, ws=None, **kw) == -1 and b"workspace" in err()
        assert _excluded(lib, ws=0x10008, ws_bytes=1 << 40, **kw) == -1 and b"aligned" in err()
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    for K in (20, 100):
        for kw, kept in ((dict(erp=None, eci=None, excl_nnz=0), 100), (dict(erp=None, eci=None, excl_nnz=0, n_kept=500, **nomaps), 500)):
            need = _lib.query("llmrec_score_topk_excluded_workspace_bytes", 4, 500, kept, 64, K, 0, 0)
            assert need > 4096
            assert _excluded(lib, K=K, ws=base, ws_bytes=4096, **kw) == CONST["LLMREC_EWORKSPACE"] and b"score_topk_excluded" in err()
    assert _excluded(lib, n_query=0) == 0                          # nothing to do: no launch
    assert _excluded(lib, n_query=0, n_kept=500, **nomaps) == 0


@needs_hipcc
def test_no_kernel_of_exclude_hip_uses_scratch():
    res = resource_usage("exclude.hip")
    names = ("ex_keys_kernel", "ex_merge_kernel")
    for name in names:
        assert [k for k in res if name in k], name
    ours = {k: r for k, r in res.items() if "rocprim" not in k and "hipcub" not in k}      # (the vendor radix sort keeps private arrays)
    assert len(ours) == len(names), sorted(ours)
    assert len(res) > len(ours)                                    # the sort's kernels are in this file
    for kernel, r in ours.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (kernel, r)


def test_the_accepted_forms_become_one_csr():
    from llmrec_amd.serve import csr_slice, exclusion_csr
    users = [5, 2, 5, 0]
    assert exclusion_csr(None, users, 10) is None
    want_rp, want_ci = [0, 3, 3, 6, 7], [9, 1, 1, 9, 1, 1, 4]
    forms = {
        "dict": {5: [9, 1, 1], 0: np.array([4]), 7: [3]},          # user 5 twice: both occurrences; user 7 is not listed: ignored
        "sequences": [[9, 1, 1], [], (9, 1, 1), torch.tensor([4])],
        "pair": (np.array([0, 3, 3, 6, 7]), [9, 1, 1, 9, 1, 1, 4]),
        "pair of tensors": (torch.tensor(want_rp, dtype=torch.int32), torch.tensor(want_ci, dtype=torch.int32)),
        "array": np.array([[9, 1, 1], [-1, -1, -1], [9, 1, 1], [4, -1, -1]]),
        "tensor": torch.tensor([[9, -1, 1, 1], [-1, -1, -1, -1], [-1, 9, 1, 1], [-1, -1, 4, -1]]),      # padding anywhere
    }
    for name, form in forms.items():
        rp, ci = exclusion_csr(form, users, 10)
        assert rp.dtype == np.int32 and ci.dtype == np.int32, name
        assert rp.tolist() == want_rp and ci.tolist() == want_ci, name
    rp, ci = exclusion_csr([[3, -1, 2], [-5]], [1, 1], 10)            # a LIST of two lists is two rows; negative entries are padding
    assert rp.tolist() == [0, 2, 2] and ci.tolist() == [3, 2]
    rp, ci = exclusion_csr({}, users, 10)
    assert rp.tolist() == [0] * 5 and ci.size == 0
    rp, ci = exclusion_csr(np.zeros((0, 3), np.int64), [], 10)
    assert rp.tolist() == [0] and ci.size == 0
    # chunks: the rows of a chunk, the row pointers rebased
    full = exclusion_csr(forms["dict"], users, 10)
    for chunk in (1, 2, 3, 4):
        rows = []
        for a in range(0, 4, chunk):
            rp, ci = csr_slice(full, a, min(a + chunk, 4))
            assert rp[0] == 0 and rp[-1] == ci.size and rp.dtype == np.int32 and len(rp) == min(chunk, 4 - a) + 1
            rows += [ci[x:y].tolist() for x, y in zip(rp[:-1], rp[1:])]
        assert rows == [[9, 1, 1], [], [9, 1, 1], [4]], chunk
    for bad, match in (([[1], [2]], "rows"), (np.zeros((3, 2), np.int64), "rows"), ({5: [10]}, r"\[0, 10\)"), ([[1], [2], [3], [99]], r"\[0, 10\)"),
                       (torch.tensor([[10], [0], [0], [0]]), r"\[0, 10\)"), ((np.array([0, 1, 2]), [1, 2]), "rowptr"),
                       ((np.array([0, 2, 1, 2, 2]), [1, 2]), "rowptr"), ((np.array([1, 1, 1, 2, 2]), [1, 2]), "rowptr"),
                       ((np.array([0, 1, 1, 2, 3]), [1, 2]), "rowptr"), ([[1.5], [], [], []], "integer"), (np.arange(4), "expected"), (7, "expected")):
        with pytest.raises(ValueError, match=match):
            exclusion_csr(bad, users, 10)


def test_the_script_reads_its_pairs_and_leaves_the_drop_ins_flags(tmp_path):
    import recommend
    argv = ["--dataset", "netflix_valid_item", "--checkpoint", "c.ckpt", "--embed_size", "32", "--users", "u.txt", "--topk", "20", "--debug",
            "--exclude", "pairs.txt", "--out", "o.npz", "--Ks", "[10, 20]", "--mask_rate", "0"]
    own, rest = recommend.split_argv(argv)
    assert own.exclude == "pairs.txt" and (own.checkpoint, own.users, own.topk, own.out) == ("c.ckpt", "u.txt", 20, "o.npz")
    assert rest == ["--dataset", "netflix_valid_item", "--embed_size", "32", "--debug", "--Ks", "[10, 20]", "--mask_rate", "0"]      # untouched, in order
    assert recommend.split_argv([a for a in argv if a not in ("--exclude", "pairs.txt")])[0].exclude is None
    from utility.parser import parse_args
    a = parse_args(rest)
    assert a.embed_size == 32 and a.debug and a.dataset == "netflix_valid_item"
    # no abbreviation of --exclude is this script's: it goes on to the drop-in's parser, which refuses it
    own, rest = recommend.split_argv(["--checkpoint", "c", "--users", "u", "--topk", "1", "--out", "o", "--excl", "x", "--ex", "y"])
    assert own.exclude is None and rest == ["--excl", "x", "--ex", "y"]
    (tmp_path / "pairs.txt").write_text("3 7\n1 2\n\n3 5\n  9 9  \n3 7\n")
    np.save(str(tmp_path / "pairs.npy"), np.array([[3, 7], [1, 2], [3, 5], [9, 9], [3, 7]], dtype=np.int32))
    for name in ("pairs.txt", "pairs.npy"):
        pairs = recommend.read_pairs(str(tmp_path / name))
        assert pairs.dtype == np.int64 and pairs.tolist() == [[3, 7], [1, 2], [3, 5], [9, 9], [3, 7]], name
        lists = recommend.exclusion_lists(pairs, np.array([3, 1, 3, 4]))      # user 9 is not listed: ignored
        assert {u: v.tolist() for u, v in lists.items()} == {3: [7, 5, 7], 1: [2]}
    (tmp_path / "empty.txt").write_text("\n")
    assert recommend.read_pairs(str(tmp_path / "empty.txt")).shape == (0, 2)
    assert recommend.exclusion_lists(recommend.read_pairs(str(tmp_path / "empty.txt")), np.array([1])) == {}
    (tmp_path / "bad.txt").write_text("3 7 1\n")
    np.save(str(tmp_path / "bad.npy"), np.arange(6))
    for name in ("bad.txt", "bad.npy"):
        with pytest.raises(SystemExit):
            recommend.read_pairs(str(tmp_path / name))
