"""Recommending under an item allow-list (csrc/serve.hip, ops.ItemFilter / ops.score_topk_filtered, llmrec_amd/serve.py, recommend.py), the
parts that need no device: the numpy restatement of the id maps and the compact mask rows against hand-written records, the workspace
formulas, the C ABI and its argument checks, the kernels' resources, the flag-vector logic and the script's argument split."""
import ctypes

import numpy as np
import pytest
import torch

from llmrec_amd import _lib, build
from llmrec_amd._lib import CONST
from tests import _serve_ref as R
from tests._hipcc import needs_hipcc, resource_usage

ENTRIES = ("llmrec_item_filter_workspace_bytes", "llmrec_item_filter_build", "llmrec_score_topk_filtered_workspace_bytes",
           "llmrec_score_topk_filtered_mask_offset", "llmrec_score_topk_filtered_f32")

# one record, written by hand: 8 items, the eligible bytes 1 / 255 / 1 / 255
ALLOW = np.array([0, 1, 255, 0, 1, 0, 0, 255], dtype=np.uint8)
NEW_ID = [-1, 0, 1, -1, 2, -1, -1, 3]
OLD_ID = [1, 2, 4, 7]
TRAIN_ROWS = [[1, 1, 3, 4],        # a duplicated pair, one ineligible entry -> 0 0 2
              [0, 3, 5],           # loses every entry
              [],
              [2, 7, 7]]           # -> 1 3 3
QUERY = [3, 0, 3, 1]               # unsorted, user 3 twice
MASK_ROWPTR = [0, 3, 6, 9, 9]
MASK_COLIDX = [1, 3, 3, 0, 0, 2, 1, 3, 3]


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.asarray([c for r in rows for c in r], dtype=np.int32)


def test_id_maps_against_the_hand_written_record():
    new_id, old_id, n_kept = R.id_maps(ALLOW)
    assert new_id.tolist() == NEW_ID and old_id.tolist() == OLD_ID and n_kept == 4
    assert new_id.dtype == np.int32 and old_id.dtype == np.int32
    for allow, want in ((np.zeros(5, np.uint8), ([-1] * 5, [], 0)), (np.full(3, 255, np.uint8), ([0, 1, 2], [0, 1, 2], 3)),
                        (np.array([0, 0, 7], np.uint8), ([-1, -1, 0], [2], 1)), (np.zeros(0, np.uint8), ([], [], 0))):
        new_id, old_id, n_kept = R.id_maps(allow)
        assert (new_id.tolist(), old_id.tolist(), n_kept) == want
    # the two maps invert each other, and the compact numbering is monotone in the item id (what keeps ascending rows ascending and the
    # tie-break by id intact)
    rng = np.random.default_rng(7)
    allow = rng.integers(0, 3, 5000).astype(np.uint8) * 127
    new_id, old_id, n_kept = R.id_maps(allow)
    assert np.array_equal(new_id[old_id], np.arange(n_kept)) and np.all(np.diff(old_id) > 0)
    assert np.array_equal(new_id >= 0, allow != 0)


def test_mask_rows_against_the_hand_written_record():
    rp, ci = _csr(TRAIN_ROWS)
    new_id, _, _ = R.id_maps(ALLOW)
    mrp, mci = R.mask_rows(rp, ci, QUERY, new_id)
    assert mrp.tolist() == MASK_ROWPTR and mci.tolist() == MASK_COLIDX
    none, _, _ = R.id_maps(np.zeros(8, np.uint8))                   # no eligible item: every row loses every entry
    mrp, mci = R.mask_rows(rp, ci, QUERY, none)
    assert mrp.tolist() == [0] * 5 and mci.size == 0
    every, _, _ = R.id_maps(np.ones(8, np.uint8))                   # every item eligible: the train rows themselves
    mrp, mci = R.mask_rows(rp, ci, QUERY, every)
    assert mci.tolist() == TRAIN_ROWS[3] + TRAIN_ROWS[0] + TRAIN_ROWS[3] + TRAIN_ROWS[1]


def test_entries_are_declared_and_exported_and_the_abi_stays():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(lib, name), name
    assert protos["llmrec_item_filter_build"][2] == ["n_items", "allow", "new_id", "old_id", "n_kept_dev", "workspace", "workspace_bytes", "stream"]
    wide = protos["llmrec_score_topk_wide_f32"][2]
    assert protos["llmrec_score_topk_filtered_f32"][2] == wide[:-1] + ["new_id", "old_id", "n_kept_dev", "n_kept", wide[-1]]
    assert protos["llmrec_score_topk_filtered_workspace_bytes"][2] == ["n_query", "n_items", "n_kept", "d", "K", "train_nnz"]
    assert CONST["LLMREC_ABI_VERSION"] == 8 and _lib.load().llmrec_abi_version() == 8
    assert CONST["LLMREC_FILTER_TILE"] == 2048
    assert "serve.hip" in build.SOURCES


def test_workspace_formulas_restated():
    tile = CONST["LLMREC_FILTER_TILE"]
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 37, 17366, 1_000_000, (1 << 31) - 1):
        assert _lib.query("llmrec_item_filter_workspace_bytes", n) == R.filter_workspace_bytes(n, tile), n
    assert _lib.query("llmrec_item_filter_workspace_bytes", -1) == -1 and _lib.query("llmrec_item_filter_workspace_bytes", 1 << 31) == -1
    ws = lambda *a: _lib.query("llmrec_score_topk_filtered_workspace_bytes", *a)
    off = lambda *a: _lib.query("llmrec_score_topk_filtered_mask_offset", *a)
    for n, items, kept, d, nnz in ((13187, 17366, 1737, 64, 68933), (203, 3000, 3000, 20, 6000), (40, 6181, 37, 16, 0), (65536, 1_000_000, 100_000, 128, 3_000_000),
                                   (1, 1, 1, 1, 0), (0, 10, 5, 16, 0)):
        for K in (1, 20, 56, 64, 65, 130, 1024):
            wide = _lib.query("llmrec_score_topk_wide_workspace_bytes", n, kept, d, K, nnz)
            assert wide >= 0
            assert ws(n, items, kept, d, K, nnz) == R.filtered_workspace_bytes(n, kept, d, nnz, wide), (n, items, kept, d, K)
            assert off(n, items, kept, d, K, nnz) == R.mask_offset(n, kept, d, nnz, wide)
        assert ws(n, items, 0, d, 20, nnz) == 0 and off(n, items, 0, d, 20, nnz) == -1         # no eligible item: no sweep, no workspace
        assert ws(n, items, kept, d, 20, nnz + 1000) >= ws(n, items, kept, d, 20, nnz)
    for bad in ((-1, 10, 5, 64, 20, 0), (4, 0, 0, 64, 20, 0), (4, 10, 11, 64, 20, 0), (4, 10, -1, 64, 20, 0), (4, 10, 5, 0, 20, 0), (4, 10, 5, 129, 20, 0),
                (4, 10, 5, 64, 0, 0), (4, 10, 5, 64, 1025, 0), (4, 10, 5, 64, 20, -1), (4, 1 << 31, 5, 64, 20, 0), (1 << 22, 10, 5, 64, 1024, 0)):
        assert ws(*bad) == -1, bad


def _filtered(lib, n_query=4, q=0x1000, Eu=0x2000, Ei=0x3000, d=64, ld=64, n_items=500, K=20, ws=None, ws_bytes=0, mode=0, train_nnz=0,
              new_id=0x6000, old_id=0x7000, n_kept_dev=0x8000, n_kept=100, rowptr=None, colidx=None):
    return lib.llmrec_score_topk_filtered_f32(n_query, q, Eu, ld, Ei, ld, n_items, d, rowptr, colidx, K, 0x4000, 0x5000, ws, ws_bytes, mode, train_nnz,
                                              new_id, old_id, n_kept_dev, n_kept, None)


def test_argument_checks_run_without_a_device():
    lib = _lib.load()
    err = lib.llmrec_last_error
    for K in (0, -3, 1025):
        assert _filtered(lib, K=K) == -1 and b"score_topk_filtered" in err() and b"1024" in err()
    assert _filtered(lib, n_kept=-1) == -1 and b"n_kept" in err()
    assert _filtered(lib, n_kept=501) == -1 and b"n_kept" in err()
    assert _filtered(lib, mode=2) == -1 and b"mode" in err()
    assert _filtered(lib, Ei=None) == -1 and b"null pointer" in err()
    assert _filtered(lib, ld=63) == -1 and b"ld < d" in err()
    assert _filtered(lib, old_id=None) == -1 and b"maps" in err()
    assert _filtered(lib, rowptr=0x9000) == -1 and b"train CSR incomplete" in err()
    assert _filtered(lib, d=129, ld=129) == CONST["LLMREC_EUNSUPPORTED"]
    assert _filtered(lib, ws=None) == -1 and b"workspace" in err()
    assert _filtered(lib, ws=0x10008, ws_bytes=1 << 40) == -1 and b"aligned" in err()
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    for K in (20, 100):
        need = _lib.query("llmrec_score_topk_filtered_workspace_bytes", 4, 500, 100, 64, K, 0)
        assert need > 4096
        assert _filtered(lib, K=K, ws=base, ws_bytes=4096) == CONST["LLMREC_EWORKSPACE"] and b"score_topk_filtered" in err()
    assert _filtered(lib, n_query=0) == 0                          # nothing to do: no launch
    build_ = lib.llmrec_item_filter_build
    assert build_(-1, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 1 << 20, None) == -1 and b"item_filter_build" in err()
    assert build_(1 << 31, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 1 << 20, None) == -1
    assert build_(10, None, 0x2000, 0x3000, 0x4000, 0x5000, 1 << 20, None) == -1 and b"null pointer" in err()
    assert build_(10, 0x1000, 0x2000, 0x3000, None, 0x5000, 1 << 20, None) == -1
    assert build_(10, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 8, None) == CONST["LLMREC_EWORKSPACE"]


@needs_hipcc
def test_no_kernel_of_serve_hip_uses_scratch():
    res = resource_usage("serve.hip")
    names = ("if_count_kernel", "if_scan_kernel", "if_write_kernel", "sv_users_kernel", "sv_items_kernel", "sv_count_kernel", "sv_rowptr_kernel",
             "sv_train_rows_kernel", "sv_finish_kernel")
    for name in names:
        assert [k for k in res if name in k], name
    assert len(res) == len(names)
    for kernel, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (kernel, r)


def test_flag_vector_logic():
    from llmrec_amd.serve import allow_flags
    assert allow_flags(6) is None
    f = allow_flags(6, allow_items=[4, 1, 1])
    assert f.dtype == torch.uint8 and f.tolist() == [0, 1, 0, 0, 1, 0]
    assert allow_flags(6, deny_items=np.array([0, 5])).tolist() == [0, 1, 1, 1, 1, 0]
    assert allow_flags(6, allow_items=torch.tensor([1, 2, 4]), deny_items=[2, 3]).tolist() == [0, 1, 0, 0, 1, 0]     # allowed and not denied
    assert allow_flags(6, allow_items=[]).tolist() == [0] * 6                                                         # an empty allow list: nothing
    assert allow_flags(6, deny_items=[]).tolist() == [1] * 6
    for kw in (dict(allow_items=[6]), dict(allow_items=[-1]), dict(deny_items=[0, 99]), dict(allow_items=torch.tensor([2, 6])),
               dict(allow_items=[1], deny_items=np.array([-2]))):
        with pytest.raises(ValueError, match=r"\[0, 6\)"):
            allow_flags(6, **kw)
    with pytest.raises(ValueError, match="integer"):
        allow_flags(6, allow_items=[1.5])


def test_the_script_splits_its_arguments_from_the_drop_ins(tmp_path):
    import recommend
    argv = ["--dataset", "netflix_valid_item", "--checkpoint", "c.ckpt", "--embed_size", "32", "--users", "u.txt", "--topk", "20", "--debug",
            "--out", "o.npz", "--deny_items", "d.npy", "--Ks", "[10, 20]", "--include_seen", "--mask_rate", "0"]
    own, rest = recommend.split_argv(argv)
    assert (own.checkpoint, own.users, own.topk, own.out, own.deny_items, own.allow_items, own.include_seen) == ("c.ckpt", "u.txt", 20, "o.npz", "d.npy", None, True)
    assert rest == ["--dataset", "netflix_valid_item", "--embed_size", "32", "--debug", "--Ks", "[10, 20]", "--mask_rate", "0"]      # untouched, in order
    from utility.parser import parse_args
    a = parse_args(rest)
    assert a.embed_size == 32 and a.debug and a.dataset == "netflix_valid_item"
    recommend.refuse_masking(a)
    # no abbreviation swallows a flag of the drop-in: --check / --top are not this script's
    with pytest.raises(SystemExit):
        recommend.split_argv(["--check", "c.ckpt", "--users", "u", "--topk", "1", "--out", "o"])
    with pytest.raises(SystemExit):                                # one list or the other
        recommend.split_argv(argv + ["--allow_items", "a.txt"])
    for flags in (["--mask", "True"], ["--mask_rate", "0.1"]):
        with pytest.raises(SystemExit, match="masking round"):
            recommend.refuse_masking(parse_args(rest[:-2] + flags))
    (tmp_path / "ids.txt").write_text("3\n1\n\n4\n")
    np.save(str(tmp_path / "ids.npy"), np.array([5, 9], dtype=np.int32))
    assert recommend.read_ids(str(tmp_path / "ids.txt")).tolist() == [3, 1, 4] and recommend.read_ids(str(tmp_path / "ids.npy")).dtype == np.int64
    assert recommend.read_ids(str(tmp_path / "ids.npy")).tolist() == [5, 9]
