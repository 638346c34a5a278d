"""The checkpoint's file format and its pure half (llmrec_amd/checkpoint.py), the host arithmetic of the arena's layout
(llmrec_pack_arena_bytes) and the snapshot kernel's resource usage - everything that needs no GPU. Bit-exact throughout: no tolerances."""
import ctypes
import json
import os
import pickle
import random
import struct
import warnings
import zlib

import numpy as np
import pytest

from llmrec_amd import _lib, checkpoint as C
from tests._hipcc import needs_hipcc, resource_usage


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in C.CHECKPOINT_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def test_both_entry_points_are_declared_and_exported_and_the_abi_stays():
    protos = _lib.parse_header()
    assert "llmrec_pack_arena_bytes" in protos and "llmrec_pack_segments" in protos
    assert protos["llmrec_pack_arena_bytes"][0] is ctypes.c_int64 and len(protos["llmrec_pack_segments"][1]) == 8
    lib = _lib.load()
    assert lib.llmrec_pack_arena_bytes and lib.llmrec_pack_segments
    assert lib.llmrec_abi_version() == 8 and _lib.CONST["LLMREC_ABI_VERSION"] == 8
    assert _lib.CONST["LLMREC_PACK_MAX_SEGMENTS"] == 64 and _lib.CONST["LLMREC_PACK_ALIGN"] == 256 == C.PACK_ALIGN
    assert len(_lib.STRUCT) == 17                              # no struct joined the header: the table is parallel host arrays
    assert C.CHECKPOINT_SWITCHES == ("LLMREC_CHECKPOINT", "LLMREC_CHECKPOINT_EVERY", "LLMREC_RESUME")


def _arena_bytes(sizes, offsets=True):
    lib = _lib.load()
    n = len(sizes)
    b = (ctypes.c_int64 * max(n, 1))(*sizes)
    o = (ctypes.c_int64 * max(n, 1))(*([-7] * max(n, 1)))
    total = lib.llmrec_pack_arena_bytes(n, b, o if offsets else None)
    return total, list(o[:n])


def test_arena_layout_offsets_and_sizes():
    sizes = [0, 1, 255, 256, 257, 0, 3, 1 << 33, 5, 0]
    total, offs = _arena_bytes(sizes)
    want, want_total = C.layout(sizes)
    assert offs == want and total == want_total
    assert all(o % 256 == 0 for o in offs) and total % 256 == 0
    assert offs[:7] == [0, 0, 256, 512, 768, 1280, 1280]        # 0 bytes take no room; 1 and 255 one unit, 256 one, 257 two
    assert offs[8] == offs[7] + (1 << 33) and offs[8] > 1 << 32 and total == offs[8] + 256        # 64-bit offsets
    for k, s in enumerate(sizes[:-1]):
        assert offs[k] + s <= offs[k + 1]                       # disjoint, in order
    assert _arena_bytes([]) == (0, [])
    many, offs = _arena_bytes([7] * 130)                        # more segments than one launch takes: still one arena
    assert many == 130 * 256 and offs == [256 * i for i in range(130)]


def test_arena_layout_refuses_bad_arguments():
    lib = _lib.load()
    assert _arena_bytes([4, -1, 4])[0] == -1
    assert _arena_bytes([4], offsets=False)[0] == -1
    assert lib.llmrec_pack_arena_bytes(1, None, (ctypes.c_int64 * 1)()) == -1
    assert lib.llmrec_pack_arena_bytes(-1, (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)()) == -1
    assert _arena_bytes([(1 << 63) - 1])[0] == -1 and _arena_bytes([1 << 62, 1 << 62])[0] == -1   # beyond 2^63
    with pytest.raises(ValueError):
        C.layout([1, -1])


# -- the file ---------------------------------------------------------------------------------------
FLAGS = {"seed": 2022, "lr": 1e-4, "batch_size": 1024, "epoch": 1000, "verbose": 5, "debug": True, "gpu_id": 0, "data_path": "./data/",
         "title": "t", "point": "", "early_stopping_patience": 7, "mask": False, "mask_rate": 0.0, "dataset": "netflix"}
ROWPTR, COLIDX = np.array([0, 2, 3, 3], dtype=np.int64), np.array([1, 4, 0], dtype=np.int64)
STEP_OPTIONS = {"drop_rate": 0.0, "check_zero": False, "multi_stream": False, "gemm": "bf16x3", "preprop": True, "wgrad_rows": True,
                "inline_adamw": True, "fold": True, "bwd_mask": True, "bwd_zero_skip": True, "host_chain": True, "host_wgrad": True}


def _case(seed=0):
    """(header, arena, tensors): three tensors laid out in a numpy arena, as the device half does it."""
    rng = np.random.RandomState(seed)
    tensors = {"param/w": rng.standard_normal((5, 3)).astype(np.float32), "step/flag_u": rng.randint(0, 255, size=7).astype(np.uint8),
               "step/epoch_sums": rng.standard_normal(3)}
    tensors["param/w"].view(np.uint32)[0, 0] = 0x7fc00123          # a NaN pattern, -0.0 and a denormal travel as bits
    tensors["param/w"].view(np.uint32)[0, 1] = 0x80000000
    tensors["param/w"].view(np.uint32)[0, 2] = 0x00000001
    entries = [(n, str(t.dtype), t.shape, t.nbytes) for n, t in tensors.items()]
    offsets, total = C.layout([e[3] for e in entries])
    arena = np.zeros(total, dtype=np.uint8)
    for (n, t), off in zip(tensors.items(), offsets):
        arena[off:off + t.nbytes] = np.frombuffer(t.tobytes(), dtype=np.uint8)
    fp = C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, COLIDX)
    host = {"epoch": 3, "_global_step": 44, "best_recall": 0.1 + 0.2, "stopping_step": 2,
            "test_ret": {"recall": np.array([0.01, 0.02, 0.03]), "auc": 0.0}, "generators": C.capture_generators()}
    header = C.build_header(C.manifest_of(entries, offsets), total, zlib.crc32(arena), 8, "fused", True, STEP_OPTIONS, fp, host, [{"act_expected": 96}])
    return header, arena, tensors


def test_header_and_arena_round_trip(tmp_path):
    header, arena, tensors = _case()
    path = str(tmp_path / "a.ckpt")
    C.write_file(path, header, arena)
    assert not os.path.exists(path + ".tmp")
    got, buf = C.read_file(path)
    assert got == json.loads(C.encode_header(header).decode()) and bytes(buf) == arena.tobytes()
    assert got["host"]["best_recall"] == 0.1 + 0.2 and got["host"]["test_ret"]["recall"] == [0.01, 0.02, 0.03]      # floats exactly
    for e in got["manifest"]:
        t = tensors[e["name"]]
        assert e["offset"] % 256 == 0 and e["bytes"] == t.nbytes and e["dtype"] == str(t.dtype) and tuple(e["shape"]) == t.shape
        back = np.frombuffer(bytes(buf[e["offset"]:e["offset"] + e["bytes"]]), dtype=t.dtype).reshape(t.shape)
        assert back.tobytes() == t.tobytes()
    pinned = np.zeros(len(arena), dtype=np.uint8)                  # the device half reads straight into pinned memory
    _, buf2 = C.read_file(path, into=lambda n: pinned[:n])
    assert buf2 is not None and pinned.tobytes() == arena.tobytes()
    assert C.check_compatible(got, {"abi": 8, "route": "fused", "device_sampler": True, "step_options": STEP_OPTIONS,
                                    "fingerprint": C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, COLIDX)}) == []


def test_the_fingerprint_leaves_out_what_does_not_change_a_step():
    fp = C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, COLIDX)
    assert set(fp["flags"]) == set(FLAGS) - set(C.FINGERPRINT_SKIP) and not set(C.FINGERPRINT_SKIP) & set(fp["flags"])
    assert set(C.FINGERPRINT_SKIP) == {"epoch", "verbose", "debug", "gpu_id", "data_path", "title", "point", "early_stopping_patience"}
    from utility.parser import FLAGS as ALL
    assert set(C.FINGERPRINT_SKIP) <= {f[0] for f in ALL}
    assert C.fingerprint(dict(FLAGS, epoch=4, data_path="/x/", debug=False), 3, 5, 3, ROWPTR, COLIDX) == fp
    other = C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, np.array([1, 3, 0], dtype=np.int64))
    assert other["csr_crc32"] != fp["csr_crc32"]


def test_equal_inputs_give_byte_equal_files(tmp_path):
    random.seed(5); np.random.seed(5)
    h1, a1, _ = _case()
    random.seed(5); np.random.seed(5)
    h2, a2, _ = _case()
    C.write_file(str(tmp_path / "1"), h1, a1)
    C.write_file(str(tmp_path / "2"), h2, a2)
    one, two = open(str(tmp_path / "1"), "rb").read(), open(str(tmp_path / "2"), "rb").read()
    assert one == two and len(one) == 20 + len(C.encode_header(h1)) + len(a1)
    assert one[:8] == b"LLMRECKP" and struct.unpack("<IQ", one[8:20]) == (C.FORMAT_VERSION, len(C.encode_header(h1)))


def _written(tmp_path):
    header, arena, _ = _case()
    path = str(tmp_path / "x.ckpt")
    C.write_file(path, header, arena)
    return path, open(path, "rb").read(), header


def test_each_rejection_names_its_cause(tmp_path):
    path, blob, header = _written(tmp_path)
    bad = str(tmp_path / "bad.ckpt")

    def rejects(data, word):
        open(bad, "wb").write(data)
        with pytest.raises(C.CheckpointError, match=word):
            C.read_file(bad)
    rejects(blob[:-1], "truncated")
    rejects(blob[:40], "truncated")
    rejects(blob[:10], "truncated")
    rejects(b"", "truncated")
    flipped = bytearray(blob); flipped[-3] ^= 0x10
    rejects(bytes(flipped), "crc mismatch")
    rejects(b"LLMRECKQ" + blob[8:], "wrong magic")
    rejects(blob[:8] + struct.pack("<I", C.FORMAT_VERSION + 1) + blob[12:], "wrong format version")
    rejects(blob + b"\0", "longer")
    assert C.read_file(path)[0]["route"] == "fused"               # the untouched file still reads


def test_each_mismatch_lists_its_keys_and_strict_false_warns(tmp_path):
    path, _, _ = _written(tmp_path)
    header, _ = C.read_file(path)
    fp = C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, COLIDX)
    base = {"abi": 8, "route": "fused", "device_sampler": True, "step_options": STEP_OPTIONS, "fingerprint": fp}
    cases = {
        "fingerprint.flags.lr": dict(base, fingerprint=C.fingerprint(dict(FLAGS, lr=2e-4), 3, 5, 3, ROWPTR, COLIDX)),
        "fingerprint.n_items": dict(base, fingerprint=C.fingerprint(FLAGS, 3, 6, 3, ROWPTR, COLIDX)),
        "fingerprint.csr_crc32": dict(base, fingerprint=C.fingerprint(FLAGS, 3, 5, 3, ROWPTR, COLIDX[::-1].copy())),
        "route": dict(base, route="modular"),
        "device_sampler": dict(base, device_sampler=False),
        "step_options.gemm": dict(base, step_options=dict(STEP_OPTIONS, gemm="f32")),
        "abi": dict(base, abi=9),
    }
    for key, expect in cases.items():
        with pytest.raises(C.CheckpointError) as e:
            C.check_compatible(header, expect)
        assert key in str(e.value) and "differ" in str(e.value), (key, str(e.value))
        assert C.differing_keys({k: header[k] for k in base}, json.loads(json.dumps(expect))) == [key]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert C.check_compatible(header, expect, strict=False) == [key]
        assert len(w) == 1 and key in str(w[0].message)
    with pytest.raises(C.CheckpointError, match="param/w"):
        C.check_manifest(header["manifest"], [dict(e, shape=[3, 5]) if e["name"] == "param/w" else e for e in header["manifest"]])
    C.check_manifest(header["manifest"], header["manifest"])


def test_a_failed_write_leaves_the_previous_file_intact(tmp_path, monkeypatch):
    path, blob, header = _written(tmp_path)
    other, arena, _ = _case(seed=1)

    def boom(*a):
        raise OSError("disk full")
    monkeypatch.setattr(os, "replace", boom)
    with pytest.raises(OSError, match="disk full"):
        C.write_file(path, other, arena)
    monkeypatch.undo()
    assert open(path, "rb").read() == blob and not os.path.exists(path + ".tmp")
    assert C.read_file(path)[0]["crc32"] == header["crc32"]


def test_the_file_holds_no_pickle(tmp_path):
    path, blob, _ = _written(tmp_path)
    hlen = struct.unpack("<Q", blob[12:20])[0]
    assert isinstance(json.loads(blob[20:20 + hlen].decode("utf-8")), dict)      # the header parses as JSON
    for payload in (blob, blob[20:], blob[20 + hlen:]):
        with pytest.raises(Exception):
            pickle.loads(payload)
    src = open(C.__file__).read()
    assert "import pickle" not in src and "torch.save" not in src and "torch.load" not in src


def test_generator_states_round_trip_through_json():
    import torch
    random.seed(11); np.random.seed(12); torch.manual_seed(13)
    random.random(); np.random.randint(0, 10, size=3); np.random.standard_normal(); torch.rand(3)     # (a cached gaussian too)
    state = json.loads(json.dumps(C.capture_generators()))
    draw = lambda: (random.sample(range(1000), 20), random.random(), np.random.randint(0, 1 << 30, size=8).tolist(),
                    float(np.random.standard_normal()), torch.rand(5).tolist(), torch.randperm(9).tolist())
    uninterrupted = draw()
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    C.restore_generators(state)
    assert draw() == uninterrupted


@needs_hipcc
def test_the_snapshot_kernel_uses_no_scratch_and_no_lds():
    res = resource_usage("snapshot.hip")
    assert len(res) == 1
    for name, r in res.items():
        assert "pack_segments_kernel" in name
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size [bytes/block]"] == 0, (name, r)
