"""Checkpoints: a run stopped and resumed equals the uninterrupted run, bit for bit.

Two halves.

PURE (module level; imports neither torch nor the library - tests/test_checkpoint_format_cpu.py holds it to its word on the CPU): the
FILE FORMAT, and the host generators' states.

    offset 0   8 bytes   MAGIC  b"LLMRECKP"
           8   4 bytes   FORMAT_VERSION, little-endian uint32
          12   8 bytes   H = the header's length, little-endian uint64
          20   H bytes   the header: one JSON object (UTF-8, sorted keys, no insignificant white space)
      20 + H   A bytes   the arena, verbatim: the bytes llmrec_pack_segments(direction 0) left in device memory. A = header["arena_bytes"].

No pickle anywhere: reading a checkpoint executes nothing. The header holds
    manifest      [{name, dtype, shape, offset, bytes}] of every segment of the arena (offsets are multiples of PACK_ALIGN = 256);
    arena_bytes, crc32   the arena's length and zlib.crc32;
    abi           LLMREC_ABI_VERSION of the library that packed it;
    route         "fused" / "fused_wide" / "modular" (step_options.route), device_sampler: whether the sampler runs on the device;
    step_options  the resolved StepOptions record of the step (None on the per-op path);
    fingerprint   the configuration (fingerprint()): every flag that changes the arithmetic, the graph's sizes and a crc32 of its CSR;
    host          the host state as the caller handed it in (Trainer: epoch, _global_step, best_recall, stopping_step, test_ret) plus
                  "generators": python's, numpy's and torch's CPU and device generator states (hex);
    parts_host    per state owner, what it keeps on the host (FusedStep.host_state()).
Equal states give byte-equal arenas (the padding is zero-filled) and so byte-equal files. A file is written as <name>.tmp, fsync'ed and
renamed into place (os.replace): a failed write leaves the previous file intact.

DEVICE (Checkpointer): the snapshot costs the training stream ONE launch (two beyond 64 tensors) - llmrec_pack_segments into a device
arena. A side stream then waits for an event, copies the arena into pinned memory in one asynchronous D2H copy and records a second event;
a single writer thread waits for that event, takes the crc and writes the file. The owners of the state list it themselves
(state_tensors(): FusedStep, FusedAdamW, DeviceBatcher); this module knows no internals.

Opt-in by environment, as every other opt-in of the project (CHECKPOINT_SWITCHES; main.py reads them):
    LLMREC_CHECKPOINT=<dir>        best.ckpt whenever the test recall improves, last.ckpt when train() ends
    LLMREC_CHECKPOINT_EVERY=<n>    also last.ckpt every n epochs (default 0: never)
    LLMREC_RESUME=<file>           load before the first step and continue at the saved epoch + 1
"""
from __future__ import annotations

import binascii
import json
import os
import struct
import warnings
import zlib
from typing import Callable, Mapping, Optional, Sequence

MAGIC = b"LLMRECKP"
FORMAT_VERSION = 1
PACK_ALIGN = 256                      # LLMREC_PACK_ALIGN (tests compare layout() with llmrec_pack_arena_bytes)
_PREFIX = struct.Struct("<8sIQ")
# the variables main.py reads for this feature (kept out of step_options' tuples: tests that build a step clear these themselves)
CHECKPOINT_SWITCHES = ("LLMREC_CHECKPOINT", "LLMREC_CHECKPOINT_EVERY", "LLMREC_RESUME")
# flags that do not change what a step computes: the run's length and reporting, where the data and the device are
FINGERPRINT_SKIP = ("epoch", "verbose", "debug", "gpu_id", "data_path", "title", "point", "early_stopping_patience")


class CheckpointError(RuntimeError):
    """A checkpoint that cannot be read, or does not belong to this run; the message names the cause."""


# -- layout -------------------------------------------------------------------------------------------
def layout(nbytes: Sequence[int]):
    """(offsets, arena_bytes): llmrec_pack_arena_bytes in Python - each segment at the next multiple of PACK_ALIGN."""
    offsets, total = [], 0
    for b in nbytes:
        if b < 0:
            raise ValueError("layout: a negative size")
        offsets.append(total)
        total = -(-(total + int(b)) // PACK_ALIGN) * PACK_ALIGN
    return offsets, total


def manifest_of(entries, offsets):
    """entries: [(name, dtype string, shape, bytes)] -> the header's manifest."""
    names = [e[0] for e in entries]
    if len(set(names)) != len(names):
        raise ValueError("manifest_of: duplicate names %s" % sorted(n for n in set(names) if names.count(n) > 1))
    return [{"name": n, "dtype": str(dt), "shape": [int(x) for x in shape], "offset": int(off), "bytes": int(b)}
            for (n, dt, shape, b), off in zip(entries, offsets)]


# -- fingerprint ------------------------------------------------------------------------------------
def fingerprint(flags: Mapping, n_users: int, n_items: int, nnz: int, rowptr, colidx):
    """flags: {name: value} of utility/parser.FLAGS (an argparse namespace's vars()); rowptr / colidx: the training CSR as anything
    with the buffer protocol (numpy arrays). The flags of FINGERPRINT_SKIP stay out."""
    crc = zlib.crc32(memoryview(colidx).cast("B"), zlib.crc32(memoryview(rowptr).cast("B")))
    return {"flags": {k: _plain(v) for k, v in sorted(flags.items()) if k not in FINGERPRINT_SKIP},
            "n_users": int(n_users), "n_items": int(n_items), "nnz": int(nnz), "csr_crc32": int(crc)}


def _plain(v):
    """A value as JSON keeps it: numpy scalars and arrays become python numbers and lists."""
    if hasattr(v, "tolist"):
        return v.tolist()
    if isinstance(v, Mapping):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


# -- file -------------------------------------------------------------------------------------------
def build_header(manifest, arena_bytes: int, crc32: int, abi: int, route: str, device_sampler: bool, step_options, fingerprint_, host,
                 parts_host=None):
    return {"manifest": manifest, "arena_bytes": int(arena_bytes), "crc32": int(crc32), "abi": int(abi), "route": route,
            "device_sampler": bool(device_sampler), "step_options": _plain(step_options), "fingerprint": _plain(fingerprint_),
            "host": _plain(host), "parts_host": _plain(parts_host)}


def encode_header(header) -> bytes:
    return json.dumps(header, sort_keys=True, separators=(",", ":"), allow_nan=True).encode("utf-8")


def write_file(path: str, header, arena) -> None:
    """The file, atomically: <path>.tmp, fsync, os.replace. arena: bytes-like of header["arena_bytes"] bytes."""
    arena = memoryview(arena).cast("B")
    if arena.nbytes != header["arena_bytes"]:
        raise ValueError("write_file: the arena has %d bytes, the header says %d" % (arena.nbytes, header["arena_bytes"]))
    blob = encode_header(header)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(_PREFIX.pack(MAGIC, FORMAT_VERSION, len(blob)))
            f.write(blob)
            f.write(arena)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def read_file(path: str, into: Optional[Callable] = None):
    """(header, arena) of a verified file. into(n): a writable buffer of n bytes for the arena (pinned memory; default a bytearray).
    CheckpointError: a short file, a wrong magic or version, a header that is not JSON, a crc mismatch."""
    with open(path, "rb") as f:
        prefix = f.read(_PREFIX.size)
        if len(prefix) < _PREFIX.size:
            raise CheckpointError("%s: truncated file (%d bytes: no room for the %d-byte prefix)" % (path, len(prefix), _PREFIX.size))
        magic, version, hlen = _PREFIX.unpack(prefix)
        if magic != MAGIC:
            raise CheckpointError("%s: wrong magic %r (not a checkpoint of this project)" % (path, magic))
        if version != FORMAT_VERSION:
            raise CheckpointError("%s: wrong format version %d (this reader knows %d)" % (path, version, FORMAT_VERSION))
        blob = f.read(hlen)
        if len(blob) < hlen:
            raise CheckpointError("%s: truncated file (the header has %d of %d bytes)" % (path, len(blob), hlen))
        try:
            header = json.loads(blob.decode("utf-8"))
            n = int(header["arena_bytes"])
            want = int(header["crc32"])
            header["manifest"]
        except (ValueError, KeyError, TypeError) as e:
            raise CheckpointError("%s: the header is not this format's JSON object (%s)" % (path, e))
        buf = into(n) if into is not None else bytearray(n)
        view = memoryview(buf).cast("B")
        got = f.readinto(view) if n else 0
        if got < n or view.nbytes != n:
            raise CheckpointError("%s: truncated file (the arena has %d of %d bytes)" % (path, got or 0, n))
        if f.read(1):
            raise CheckpointError("%s: %d bytes expected, the file is longer" % (path, _PREFIX.size + hlen + n))
    crc = zlib.crc32(view)
    if crc != want:
        raise CheckpointError("%s: crc mismatch (the arena's crc32 is %08x, the header says %08x): corrupt payload" % (path, crc, want))
    return header, buf


def differing_keys(a, b, prefix=""):
    """The dotted keys at which two JSON-like values differ."""
    if isinstance(a, Mapping) and isinstance(b, Mapping):
        out = []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                out.append(prefix + str(k))
            else:
                out += differing_keys(a[k], b[k], prefix + str(k) + ".")
        return out
    return [] if a == b else [prefix.rstrip(".")]


def check_compatible(header, expect, strict: bool = True):
    """A checkpoint against the run that loads it: expect = {abi, route, device_sampler, step_options, fingerprint}. A mismatch raises
    CheckpointError listing the keys that differ; strict=False: one warning instead. Returns the list."""
    mine = json.loads(json.dumps(_plain({k: expect.get(k) for k in ("abi", "route", "device_sampler", "step_options", "fingerprint")})))
    theirs = {k: header.get(k) for k in mine}
    bad = differing_keys(theirs, mine)
    if bad:
        msg = "the checkpoint was written by another configuration; these differ (saved != this run): " + ", ".join(
            "%s (%r != %r)" % (k, _dig(theirs, k), _dig(mine, k)) for k in bad)
        if strict:
            raise CheckpointError(msg)
        warnings.warn("checkpoint: " + msg + " - loading anyway (strict=False)")
    return bad


def _dig(d, dotted):
    for k in dotted.split("."):
        if not isinstance(d, Mapping) or k not in d:
            return None
        d = d[k]
    return d


def check_manifest(saved, current):
    """The saved manifest against the loading run's own: equal names, dtypes, shapes, sizes and offsets, in order."""
    if saved != current:
        a, b = {e["name"]: e for e in saved}, {e["name"]: e for e in current}
        bad = [n for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
        raise CheckpointError("the checkpoint's tensors are not this run's: %s%s" % (
            ", ".join("%s (saved %s, here %s)" % (n, _brief(a.get(n)), _brief(b.get(n))) for n in bad[:8]),
            "" if bad else "the same tensors in another order"))


def _brief(e):
    return "absent" if e is None else "%s%s@%d" % (e["dtype"], e["shape"], e["offset"])


# -- host generators --------------------------------------------------------------------------------
def capture_generators(device=None):
    """Python's random, numpy's global RandomState and torch's CPU (and, with a device, that device's) generator, as JSON values.
    Data.sample() and the augmented triples draw from the first two; the per-op path's dropout from torch's."""
    import random
    import numpy as np
    import torch
    v, words, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"python": {"version": v, "words": binascii.hexlify(struct.pack("<%dI" % len(words), *words)).decode(), "gauss": gauss},
           "numpy": {"kind": kind, "keys": binascii.hexlify(np.ascontiguousarray(keys, dtype="<u4").tobytes()).decode(), "pos": int(pos),
                     "has_gauss": int(has_gauss), "cached": float(cached)},
           "torch_cpu": binascii.hexlify(torch.get_rng_state().numpy().tobytes()).decode(), "torch_device": None}
    if device is not None and torch.cuda.is_available():
        out["torch_device"] = binascii.hexlify(torch.cuda.get_rng_state(device).numpy().tobytes()).decode()
    return out


def restore_generators(state, device=None):
    import random
    import numpy as np
    import torch
    py, npy = state["python"], state["numpy"]
    raw = binascii.unhexlify(py["words"])
    random.setstate((py["version"], struct.unpack("<%dI" % (len(raw) // 4), raw), py["gauss"]))
    np.random.set_state((npy["kind"], np.frombuffer(binascii.unhexlify(npy["keys"]), dtype="<u4").copy(), npy["pos"], npy["has_gauss"], npy["cached"]))
    as_state = lambda h: torch.from_numpy(np.frombuffer(binascii.unhexlify(h), dtype=np.uint8).copy())
    torch.set_rng_state(as_state(state["torch_cpu"]))
    if state.get("torch_device") is not None and device is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(as_state(state["torch_device"]), device)


# -- device half ------------------------------------------------------------------------------------
def _flatten_parts(parts):
    return list(parts) if isinstance(parts, (list, tuple)) else [parts]


class Checkpointer:
    """Checkpointer(step_or_parts, directory): step_or_parts is a state owner or a list of them - anything with state_tensors() ->
    [(name, tensor)] (FusedStep, FusedAdamW, DeviceBatcher, ...; optionally host_state() / prepare_load(saved) / finish_load(host)), or
    a plain [(name, tensor)] list. describe: {abi, route, device_sampler, step_options, fingerprint} of the run (written into every
    header and checked by load()); log: a callable for the wait / replay lines.

    request(name, host_state)  enqueue a snapshot of the state as it stands at this point of the current stream, to be written as
                               <directory>/<name>. Does not synchronise the host with the device unless a write is still in flight.
    wait()                     block until the last requested file is in place (re-raises what the writer met).
    save(path, host_state)     request + wait.
    load(path, strict=True)    read and verify the file, one H2D copy, one unpack launch, the host generators; returns the host state.
    stats: what a measurement wants - requests, waits, seconds spent in request() / waiting / crc / writing."""

    def __init__(self, step_or_parts, directory: Optional[str] = None, describe: Optional[Mapping] = None, log: Optional[Callable] = None):
        import queue
        self.parts = _flatten_parts(step_or_parts)
        if self.parts and isinstance(self.parts[0], tuple):                 # a plain [(name, tensor)] list is one part
            self.parts = [_TensorList(self.parts)]
        from . import _lib
        self.directory, self.log = directory, log
        self.describe = {"abi": _lib.CONST["LLMREC_ABI_VERSION"], "route": None, "device_sampler": False, "step_options": None, "fingerprint": None}
        self.describe.update(describe or {})
        self.stats = {"requests": 0, "waits": 0, "request_s": 0.0, "wait_s": 0.0, "crc_s": 0.0, "write_s": 0.0, "last_request_s": 0.0,
                      "last_crc_s": 0.0, "last_write_s": 0.0}
        self._layout_key = self._arena = self._pinned = self._side = None
        self._queue, self._thread, self._error = queue.Queue(), None, None
        import threading
        self._idle = threading.Event()
        self._idle.set()
        self.ev_packed = self.ev_copied = None                             # the two events of the last request (ev_pack_begin: timing only)
        self.time_pack = False                                              # measurement: also record an event ahead of the pack launch
        self.ev_pack_begin = None

    # .. plumbing ..
    def _tensors(self):
        out = []
        for part in self.parts:
            out += list(part.state_tensors())
        return out

    def _prepare(self, named):
        """The arena's layout for these tensors; (re)allocates the device arena, the pinned buffer and the side stream when it changed."""
        import torch
        from . import ops
        key = tuple((n, t.data_ptr(), str(t.dtype), tuple(t.shape)) for n, t in named)
        if key != self._layout_key:
            self.wait()
            sizes = [t.numel() * t.element_size() for _, t in named]
            offsets, total = ops.pack_layout(sizes)
            dev = named[0][1].device
            self._manifest = manifest_of([(n, str(t.dtype).replace("torch.", ""), tuple(t.shape), b) for (n, t), b in zip(named, sizes)], offsets)
            self._offsets, self._total = offsets, total
            self._arena = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
            self._pinned = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()[:total]
            self._side = torch.cuda.Stream(device=dev)
            self.ev_packed, self.ev_copied = torch.cuda.Event(), torch.cuda.Event()
            self.ev_pack_begin = torch.cuda.Event(enable_timing=True)
            self._layout_key = key
        return self._offsets

    def prepare(self):
        """Allocate now (the first request does it otherwise)."""
        self._prepare(self._tensors())

    def _writer(self):
        import time
        while True:
            job = self._queue.get()
            if job is None:
                return
            path, header, event = job
            try:
                event.synchronize()                                         # the D2H copy has landed in the pinned buffer
                view = self._pinned.numpy()
                t0 = time.perf_counter()
                header["crc32"] = zlib.crc32(view)
                t1 = time.perf_counter()
                write_file(path, header, view)
                t2 = time.perf_counter()
                self.stats["last_crc_s"], self.stats["last_write_s"] = t1 - t0, t2 - t1
                self.stats["crc_s"] += t1 - t0
                self.stats["write_s"] += t2 - t1
            except BaseException as e:                                      # handed to the next wait()
                self._error = e
            finally:
                self._idle.set()

    def _header(self, host_state, device):
        import json as _json
        from . import _lib
        d = self.describe
        host = dict(host_state or {})
        host["generators"] = capture_generators(device)
        parts_host = [part.host_state() if hasattr(part, "host_state") else None for part in self.parts]
        h = build_header(self._manifest, self._total, 0, d.get("abi", _lib.CONST["LLMREC_ABI_VERSION"]), d.get("route"), d.get("device_sampler", False),
                         d.get("step_options"), d.get("fingerprint"), host, parts_host)
        return _json.loads(_json.dumps(h))                                 # a copy the writer owns

    # .. the interface ..
    def request(self, name: str, host_state=None):
        import threading
        import time
        import torch
        from . import ops
        t0 = time.perf_counter()
        if not self._idle.is_set():                                        # at most one write in flight: this request waits for it
            self._on_wait()
            self._idle.wait()
            waited = time.perf_counter() - t0
            self.stats["waits"] += 1
            self.stats["wait_s"] += waited
            if self.log is not None:
                self.log("checkpoint: request(%s) waited %.1f ms for the previous write" % (name, 1e3 * waited))
        self._raise_pending()
        named = self._tensors()
        offsets = self._prepare(named)
        path = name if self.directory is None else os.path.join(self.directory, name)
        header = self._header(host_state, named[0][1].device)
        cur = torch.cuda.current_stream()
        if self.time_pack:
            self.ev_pack_begin.record(cur)
            self.ev_packed = torch.cuda.Event(enable_timing=True)
            self.ev_copied = torch.cuda.Event(enable_timing=True)
        ops.pack_segments([t for _, t in named], offsets, self._arena, 0)  # the ONE launch on the training stream (two beyond 64 tensors)
        self.ev_packed.record(cur)
        self._side.wait_event(self.ev_packed)
        with torch.cuda.stream(self._side):
            self._pinned.copy_(self._arena, non_blocking=True)             # ONE asynchronous D2H copy
            self.ev_copied.record(self._side)
        if self._thread is None:
            self._thread = threading.Thread(target=self._writer, name="llmrec-checkpoint-writer", daemon=True)
            self._thread.start()
        self._idle.clear()
        self._queue.put((path, header, self.ev_copied))
        dt = time.perf_counter() - t0
        self.stats["requests"] += 1
        self.stats["request_s"] += dt
        self.stats["last_request_s"] = dt

    def _on_wait(self):
        """Called when a request finds the previous write still in flight, before it blocks (tests hook it)."""

    def _raise_pending(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def wait(self):
        self._idle.wait()
        self._raise_pending()

    def save(self, path: str, host_state=None):
        self.request(path, host_state)
        self.wait()

    def close(self):
        """wait(), then end the writer thread."""
        try:
            self.wait()
        finally:
            if self._thread is not None:
                self._queue.put(None)
                self._thread.join()
                self._thread = None

    def load(self, path: str, strict: bool = True):
        import time
        import torch
        from . import ops
        t0 = time.perf_counter()
        self.wait()
        named = self._tensors()
        offsets = self._prepare(named)

        def into(n):
            if n != self._total:
                raise CheckpointError("%s: the arena has %d bytes, this run's state %d" % (path, n, self._total))
            return self._pinned.numpy()
        header, _ = read_file(path, into)
        check_compatible(header, self.describe, strict)
        check_manifest(header["manifest"], self._manifest)
        self._arena.copy_(self._pinned, non_blocking=True)                 # ONE H2D copy
        views = {e["name"]: self._arena[e["offset"]:e["offset"] + e["bytes"]].view(t.dtype).view(t.shape)
                 for e, (_, t) in zip(self._manifest, named)}
        saved = views.get
        for part in self.parts:
            if hasattr(part, "prepare_load"):
                part.prepare_load(saved)
        ops.pack_segments([t for _, t in named], offsets, self._arena, 1)  # ONE launch: the arena's bytes into the live tensors
        parts_host = header.get("parts_host") or [None] * len(self.parts)
        for part, host in zip(self.parts, parts_host):
            if hasattr(part, "finish_load"):
                part.finish_load(host)
        host = dict(header["host"])
        gens = host.pop("generators", None)
        if gens is not None:
            restore_generators(gens, named[0][1].device)
        torch.cuda.current_stream().synchronize()                          # the pinned buffer and the arena are free again
        self.stats["last_load_s"] = time.perf_counter() - t0
        for part in self.parts:
            rep = getattr(part, "replayed_mask_rounds", None)
            if rep is not None and self.log is not None:
                self.log("checkpoint: replayed %d masking rounds in %.1f ms" % (rep[0], 1e3 * rep[1]))
        return host


class _TensorList:
    def __init__(self, named):
        self._named = list(named)

    def state_tensors(self):
        return self._named
