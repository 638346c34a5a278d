"""llmrec_pack_segments (csrc/snapshot.hip) against torch byte views, torch.equal on uint8: every size at which the kernel changes
path (the 16-byte body, the 4-byte body, byte heads and tails, one 32 KiB chunk -1 / exact / +1, several chunks), tensor-side pointers
0, 1, 4 and 8 bytes off an aligned base, canaries around everything that may be written, the zero-filled padding, 64 segments in one
launch and more through the wrapper's chunking, and every refusal. Payloads are bits: NaN patterns, -0.0 and denormals travel unchanged."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from llmrec_amd import _lib, ops

CHUNK = 256 * 16 * 8                                             # one block's share of a segment
SIZES = [0, 1, 3, 4, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
GUARD = 64                                                       # canary bytes on either side of a tensor
SPECIAL = [0x7fc00123, 0xffc00001, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000]    # NaNs, -0.0, denormals, inf


def _payload(n, gen):
    t = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=gen)
    words = torch.tensor(SPECIAL, dtype=torch.int64).to(torch.int32).view(torch.uint8) if n >= 4 * len(SPECIAL) else None
    if words is not None:
        t[:words.numel()] = words
        t[n - words.numel():] = words
    return t.cuda()


def _tensor_in_guard(n, mis, fill):
    """(buffer, view): n bytes at `mis` bytes past a 16-byte aligned address inside a buffer pre-filled with `fill`."""
    buf = torch.full((n + 2 * GUARD + 16,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + mis:GUARD + mis + n]
    assert n == 0 or view.data_ptr() % 16 == mis % 16          # (an empty view has no address)
    return buf, view


def _guards_intact(buf, view, n, fill):
    lo = view.data_ptr() - buf.data_ptr()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all())


def _arena(total):
    """(buffer, arena): `total` bytes between two 256-byte canary zones of 0xA5, everything pre-filled with 0xA5."""
    buf = torch.full((total + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[256:256 + total]


def _expected(payloads, offsets, total):
    want = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for p, off in zip(payloads, offsets):
        want[off:off + p.numel()] = p
    return want


def _round_trip(sizes, mis_of, seed):
    gen = torch.Generator().manual_seed(seed)
    payloads = [_payload(n, gen) for n in sizes]
    offsets, total = ops.pack_layout(sizes)
    # direction 0
    srcs = [_tensor_in_guard(n, mis_of(i), 0x5C) for i, n in enumerate(sizes)]
    for (_, v), p in zip(srcs, payloads):
        v.copy_(p)
    abuf, arena = _arena(total)
    launches = ops.pack_segments([v for _, v in srcs], offsets, arena, 0)
    want = _expected(payloads, offsets, total)
    assert torch.equal(arena, want)                              # the segments where they belong, every padding byte 0
    assert bool((abuf[:256] == 0xA5).all()) and bool((abuf[256 + total:] == 0xA5).all())       # nothing outside [0, arena_bytes)
    for (b, v), p in zip(srcs, payloads):
        assert torch.equal(v, p) and _guards_intact(b, v, p.numel(), 0x5C)                      # the sources are only read
    # direction 1, out of the packed arena into fresh destinations: pack then unpack is the identity
    dsts = [_tensor_in_guard(n, mis_of(i), 0x3C) for i, n in enumerate(sizes)]
    before = abuf.clone()
    assert ops.pack_segments([v for _, v in dsts], offsets, arena, 1) == launches
    assert torch.equal(abuf, before)                             # the arena is only read
    for (b, v), p in zip(dsts, payloads):
        assert torch.equal(v, p)
        assert _guards_intact(b, v, p.numel(), 0x3C)             # only the listed range of each destination changed
    return launches


@pytest.mark.parametrize("mis", [0, 1, 4, 8])
def test_every_size_at_every_alignment(mis):
    assert _round_trip(SIZES, lambda i: mis, seed=mis) == 1


def test_mixed_alignments_and_an_unpack_of_arbitrary_arena_bytes():
    """Direction 1 from an arena whose padding is NOT zero: only the listed ranges reach the destinations."""
    sizes = [17, CHUNK + 1, 3, 2 * CHUNK + 5, 16]
    mis = [3, 12, 0, 5, 8]
    offsets, total = ops.pack_layout(sizes)
    gen = torch.Generator().manual_seed(7)
    abuf, arena = _arena(total)
    arena.copy_(torch.randint(0, 256, (total,), dtype=torch.uint8, generator=gen))
    dsts = [_tensor_in_guard(n, m, 0x3C) for n, m in zip(sizes, mis)]
    ops.pack_segments([v for _, v in dsts], offsets, arena, 1)
    for (b, v), n, off in zip(dsts, sizes, offsets):
        assert torch.equal(v, arena[off:off + n]) and _guards_intact(b, v, n, 0x3C)


@pytest.mark.parametrize("n,launches", [(64, 1), (65, 2), (130, 3)])
def test_64_segments_in_one_launch_and_more_through_the_wrapper(n, launches):
    small = [1, 0, 255, 256, 257, 40, 4096, 7, 513, 16]
    sizes = [small[i % len(small)] for i in range(n)]
    sizes[n // 2] = CHUNK + 3
    assert _round_trip(sizes, lambda i: (0, 4, 1, 8)[i % 4], seed=n) == launches


def test_typed_tensors_travel_as_bytes():
    ts = [torch.tensor(SPECIAL, dtype=torch.int64).to(torch.int32).view(torch.float32).cuda(), torch.arange(5, dtype=torch.float64, device="cuda") / 3,
          torch.tensor([2 ** 40 + 1], dtype=torch.int64, device="cuda").view(torch.uint64), torch.arange(7, dtype=torch.uint8, device="cuda"),
          torch.tensor([-3], dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float32, device="cuda")]
    offsets, total = ops.pack_layout([t.numel() * t.element_size() for t in ts])
    arena = torch.empty(total, dtype=torch.uint8, device="cuda")
    ops.pack_segments(ts, offsets, arena, 0)
    back = [torch.zeros_like(t) for t in ts]
    ops.pack_segments(back, offsets, arena, 1)
    for a, b in zip(ts, back):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_every_refusal_returns_its_status_and_writes_nothing():
    lib = _lib.load()
    EINVAL = _lib.CONST["LLMREC_EINVAL"]
    abuf, arena = _arena(1024)
    buf, t = _tensor_in_guard(300, 0, 0x5C)
    stream = ops._stream()

    def status(n, ptrs, sizes, offs, a=arena.data_ptr(), a_bytes=1024, direction=0):
        k = max(len(ptrs), 1)
        return lib.llmrec_pack_segments(n, (ctypes.c_void_p * k)(*ptrs), (ctypes.c_int64 * k)(*sizes), (ctypes.c_int64 * k)(*offs),
                                        ctypes.c_void_p(a), a_bytes, direction, stream)
    p = t.data_ptr()
    many = [p] * 65
    for direction in (0, 1):
        assert status(-1, [p], [300], [0], direction=direction) == EINVAL
        assert status(65, many, [1] * 65, [0] * 65, direction=direction) == EINVAL
        assert status(1, [None], [300], [0], direction=direction) == EINVAL              # a null pointer with non-zero bytes
        assert status(1, [p], [-1], [0], direction=direction) == EINVAL                  # a negative size
        assert status(1, [p], [300], [128], direction=direction) == EINVAL               # an offset that is no multiple of 256
        assert status(1, [p], [300], [-256], direction=direction) == EINVAL
        assert status(1, [p], [300], [768], direction=direction) == EINVAL               # passes arena_bytes (768 + 300 > 1024)
        assert status(1, [p], [300], [1280], direction=direction) == EINVAL
        assert status(1, [p], [300], [0], a=arena.data_ptr() + 4, direction=direction) == EINVAL      # the arena is not 16-byte aligned
        assert status(1, [p], [300], [0], a_bytes=-1, direction=direction) == EINVAL
    assert status(1, [p], [300], [0], direction=2) == EINVAL and status(1, [p], [300], [0], direction=-1) == EINVAL
    assert status(2, [p, p], [300, 300], [0, 256], direction=0) == EINVAL                # two writers of arena bytes [256, 300)
    assert b"pack_segments" in lib.llmrec_last_error()
    torch.cuda.synchronize()
    assert bool((abuf == 0xA5).all()) and bool((buf == 0x5C).all())                     # nothing was written anywhere
    assert status(1, [None], [0], [0], direction=1) == 0                                 # a null pointer with zero bytes is legal
    assert status(0, [], [], [], direction=1) == 0
    torch.cuda.synchronize()
    assert bool((abuf == 0xA5).all())
    assert status(0, [], [], [], direction=0) == 0                                       # no segment: the arena is all padding
    torch.cuda.synchronize()
    assert bool((arena == 0).all()) and bool((abuf[:256] == 0xA5).all()) and bool((abuf[1280:] == 0xA5).all())
