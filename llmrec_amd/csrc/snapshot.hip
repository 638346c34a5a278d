// snapshot.hip - the checkpoint's one launch: up to LLMREC_PACK_MAX_SEGMENTS byte ranges of device memory copied into one arena
// (direction 0, with every byte of the arena that belongs to no segment set to zero) or back out of it (direction 1). The table of
// segments travels to the kernel by value (as zero_multi_kernel's, rowops.hip): no device-side table, no host synchronisation, so the
// launch can sit on the training stream between two graph replays. Pure data movement: no atomics, no LDS, no scratch; every access is
// a plain vector load or store of 16, 4 or 1 bytes.
//
// Geometry: one block of 256 lanes per PACK_CHUNK = 32 KiB of a segment (8 x 16 bytes per lane: the eight loads are issued before the
// first store), then - direction 0 - one block per 32 KiB of each gap between the segments (sorted by arena offset on the host). The
// arena side of a chunk is always 16-byte aligned (arena base 16-byte aligned, offsets multiples of 256, the chunk a multiple of 16); the
// tensor side of EVERY chunk of a segment has the alignment of the segment's pointer, which picks the path:
//   16-byte aligned   16-byte accesses on both sides, the last len % 16 bytes one by one;
//    4-byte aligned   4-byte accesses on both sides, the last len % 4 bytes one by one;
//   otherwise         4-byte accesses on the arena side, four byte accesses on the tensor side, the tail one by one (uint8 views at
//                     odd addresses; no tensor of the training state is one).
#include "common.h"

namespace llmrec {

constexpr int PACK_THREADS = 256;
constexpr int PACK_VECS = 8;                                             // 16-byte pieces per lane and chunk
constexpr int64_t PACK_CHUNK = (int64_t)PACK_THREADS * 16 * PACK_VECS;   // 32 KiB

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));               // 16 bytes as one register quad

struct PackTable {
    unsigned char* ptr[LLMREC_PACK_MAX_SEGMENTS];      // tensor side, in ascending order of `off`
    int64_t bytes[LLMREC_PACK_MAX_SEGMENTS];
    int64_t off[LLMREC_PACK_MAX_SEGMENTS];
    int32_t seg_block[LLMREC_PACK_MAX_SEGMENTS + 1];   // first block of segment k; [n]: the first block of the gaps
    int32_t gap_block[LLMREC_PACK_MAX_SEGMENTS + 2];   // first block of gap j (ahead of segment j; gap n: behind the last); [n + 1]: the grid
    int32_t n, direction;
    int64_t arena_bytes;
};

// the last k in [0, count) with begin[k] <= b (begin ascending, begin[0] <= b): empty members share their successor's first block.
// (A macro over the table's member, not a function of a pointer to it: the table stays in the kernel-argument segment.)
#define PACK_OWNER(k, begin, count, b)                        \
    int k = 0;                                                \
    for (int hi__ = (count); hi__ - k > 1;) {                 \
        const int mid__ = (k + hi__) >> 1;                    \
        if ((b) >= begin[mid__]) k = mid__; else hi__ = mid__; \
    }

__device__ __forceinline__ void pack_zero(unsigned char* p, int64_t len) {
    const int tid = threadIdx.x;
    int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15);
    if (head > len) head = len;
    if (tid < head) p[tid] = 0;
    u32x4* v = reinterpret_cast<u32x4*>(p + head);
    const int64_t nvec = (len - head) / 16;
#pragma unroll
    for (int j = 0; j < PACK_VECS; ++j) {
        const int64_t i = (int64_t)j * PACK_THREADS + tid;
        if (i < nvec) v[i] = u32x4{0u, 0u, 0u, 0u};
    }
    unsigned char* tail = p + head + nvec * 16;
    if (tid < len - head - nvec * 16) tail[tid] = 0;
}

__global__ __launch_bounds__(PACK_THREADS) void pack_segments_kernel(PackTable t, unsigned char* __restrict__ arena) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = t.n;
    if (b >= t.seg_block[n]) {                                          // a gap's block (direction 0 only)
        PACK_OWNER(j, t.gap_block, n + 1, b)
        const int64_t start = j == 0 ? 0 : t.off[j - 1] + t.bytes[j - 1];
        const int64_t end = j == n ? t.arena_bytes : t.off[j];
        const int64_t begin = start + (int64_t)(b - t.gap_block[j]) * PACK_CHUNK;
        const int64_t len = end - begin < PACK_CHUNK ? end - begin : PACK_CHUNK;
        if (len > 0) pack_zero(arena + begin, len);
        return;
    }
    PACK_OWNER(k, t.seg_block, n, b)
    const int64_t begin = (int64_t)(b - t.seg_block[k]) * PACK_CHUNK;
    const int64_t left = t.bytes[k] - begin;
    const int64_t len = left < PACK_CHUNK ? left : PACK_CHUNK;
    if (len <= 0) return;
    unsigned char* T = t.ptr[k] + begin;
    unsigned char* A = arena + t.off[k] + begin;
    const bool pack = t.direction == 0;
    const unsigned char* src = pack ? T : A;
    unsigned char* dst = pack ? A : T;
    const unsigned mis = (unsigned)((uintptr_t)T & 15);
    int64_t done;
    if (mis == 0) {
        const int64_t nvec = len / 16;
        const u32x4* s = reinterpret_cast<const u32x4*>(src);
        u32x4* d = reinterpret_cast<u32x4*>(dst);
        if (len == PACK_CHUNK) {                                         // a whole chunk: the eight loads are in flight before the first store
            u32x4 r[PACK_VECS];
#pragma unroll
            for (int j = 0; j < PACK_VECS; ++j) r[j] = s[j * PACK_THREADS + tid];
#pragma unroll
            for (int j = 0; j < PACK_VECS; ++j) d[j * PACK_THREADS + tid] = r[j];
        } else {
            for (int64_t i = tid; i < nvec; i += PACK_THREADS) d[i] = s[i];
        }
        done = nvec * 16;
    } else if ((mis & 3) == 0) {
        const int nw = (int)(len / 4);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll 4
        for (int i = tid; i < nw; i += PACK_THREADS) d[i] = s[i];
        done = (int64_t)nw * 4;
    } else {
        const int nw = (int)(len / 4);
        if (pack) {
            uint32_t* d = reinterpret_cast<uint32_t*>(A);
            for (int i = tid; i < nw; i += PACK_THREADS) {
                const unsigned char* q = T + 4 * (int64_t)i;
                d[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            }
        } else {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(A);
            for (int i = tid; i < nw; i += PACK_THREADS) {
                const uint32_t w = s[i];
                unsigned char* q = T + 4 * (int64_t)i;
                q[0] = (unsigned char)w; q[1] = (unsigned char)(w >> 8); q[2] = (unsigned char)(w >> 16); q[3] = (unsigned char)(w >> 24);
            }
        }
        done = (int64_t)nw * 4;
    }
    if (tid < len - done) dst[done + tid] = src[done + tid];            // (< 16 bytes)
}

}  // namespace llmrec

using namespace llmrec;

int64_t llmrec_pack_arena_bytes(int32_t n, const int64_t* bytes_host, int64_t* offsets_host) {
    if (n < 0 || (n > 0 && (!bytes_host || !offsets_host))) return -1;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes_host[i] < 0 || bytes_host[i] > INT64_MAX - total - LLMREC_PACK_ALIGN) return -1;
        offsets_host[i] = total;
        total = align_up(total + bytes_host[i], LLMREC_PACK_ALIGN);
    }
    return total;
}

int llmrec_pack_segments(int32_t n, const void* const* ptr_host, const int64_t* bytes_host, const int64_t* offset_host, void* arena,
                         int64_t arena_bytes, int32_t direction, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n >= 0 && n <= LLMREC_PACK_MAX_SEGMENTS, "pack_segments: n = %d outside [0, %d]", n, LLMREC_PACK_MAX_SEGMENTS);
    LLMREC_CHECK_ARG(direction == 0 || direction == 1, "pack_segments: direction %d is neither 0 (pack) nor 1 (unpack)", direction);
    LLMREC_CHECK_ARG(n == 0 || (ptr_host && bytes_host && offset_host), "pack_segments: a null host array");
    LLMREC_CHECK_ARG(arena_bytes >= 0 && (arena_bytes == 0 || arena) && ((uintptr_t)arena % 16) == 0,
                     "pack_segments: the arena is null, of negative size or not 16-byte aligned");
    int order[LLMREC_PACK_MAX_SEGMENTS];
    for (int i = 0; i < n; ++i) {
        LLMREC_CHECK_ARG(bytes_host[i] >= 0, "pack_segments: segment %d has a negative size", i);
        LLMREC_CHECK_ARG(bytes_host[i] == 0 || ptr_host[i], "pack_segments: segment %d has a null pointer", i);
        LLMREC_CHECK_ARG(offset_host[i] >= 0 && offset_host[i] % LLMREC_PACK_ALIGN == 0, "pack_segments: segment %d: its offset is not a multiple of %d",
                         i, LLMREC_PACK_ALIGN);
        LLMREC_CHECK_ARG(offset_host[i] <= arena_bytes && bytes_host[i] <= arena_bytes - offset_host[i], "pack_segments: segment %d passes the arena's end", i);
        int j = i;                                                       // insertion sort by (offset, size): an empty segment precedes the one at its offset
        for (; j > 0; --j) {
            const int o = order[j - 1];
            if (offset_host[o] < offset_host[i] || (offset_host[o] == offset_host[i] && bytes_host[o] <= bytes_host[i])) break;
            order[j] = o;
        }
        order[j] = i;
    }
    PackTable t = {};
    t.n = n; t.direction = direction; t.arena_bytes = arena_bytes;
    int64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        t.ptr[k] = (unsigned char*)ptr_host[i]; t.bytes[k] = bytes_host[i]; t.off[k] = offset_host[i];
        if (direction == 0 && k > 0)                                     // two writers of one arena byte
            LLMREC_CHECK_ARG(t.off[k - 1] + t.bytes[k - 1] <= t.off[k], "pack_segments: segments %d and %d overlap in the arena", order[k - 1], i);
        t.seg_block[k] = (int32_t)blocks;
        blocks += ceil_div(t.bytes[k], PACK_CHUNK);
        LLMREC_CHECK_ARG(blocks < 0x7fffffffll, "pack_segments: too many bytes for one launch");
    }
    for (int k = n; k <= LLMREC_PACK_MAX_SEGMENTS; ++k) t.seg_block[k] = (int32_t)blocks;
    for (int j = 0; j <= n; ++j) {
        t.gap_block[j] = (int32_t)blocks;
        if (direction == 0) {
            const int64_t start = j == 0 ? 0 : t.off[j - 1] + t.bytes[j - 1];
            const int64_t end = j == n ? arena_bytes : t.off[j];
            blocks += ceil_div(end - start, PACK_CHUNK);
            LLMREC_CHECK_ARG(blocks < 0x7fffffffll, "pack_segments: too many bytes for one launch");
        }
    }
    for (int j = n + 1; j < LLMREC_PACK_MAX_SEGMENTS + 2; ++j) t.gap_block[j] = (int32_t)blocks;
    if (blocks == 0) return LLMREC_OK;
    pack_segments_kernel<<<(unsigned)blocks, PACK_THREADS, 0, (hipStream_t)stream_>>>(t, (unsigned char*)arena);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}
