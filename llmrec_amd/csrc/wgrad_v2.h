// wgrad_v2.h - the weight gradient's second organisation (128-wide k slabs, v_mfma_f32_32x32x16_bf16) as device functions, with the
// argument blocks and helpers it needs: shared by dense.hip (the multi-target launch) and wgrad_host.hip (the same launch hosting an
// SpMM in the CUs it leaves free). Each translation unit compiles its own kernel around wgrad_bf16x3_v2_body, so adding the hosting
// kernel leaves dense.hip's device code as it was.
#pragma once
#include "common.h"
#include "spmm_body.h"

namespace llmrec {

// a GLOBAL-memory pointer known to be the same in every lane, moved into scalar registers (so that loads can use the
// scalar-base + 32-bit-lane-offset form); the address space is kept explicit - a pointer rebuilt from integers would
// otherwise be generic and load through FLAT instructions
typedef const char __attribute__((address_space(1))) * global_cptr;
__device__ __forceinline__ global_cptr uniform_ptr(const void* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (global_cptr)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t uniform_u64(const void* p) {   // the same, as an integer (for buffer descriptors)
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 float4 (rows j = 0..7 of one lane; component c belongs to tile c) -> the three bf16x8 fragments of all four
// tiles. The residual arithmetic runs on the register pairs (x, y) and (z, w) exactly as they were loaded (packed
// subtractions, no moves); only the final v_perm_b32 packing crosses loads. 144 VALU instructions per 32 values.
__device__ __forceinline__ void split32(const float4 (&v)[8], uint4 (&H)[4], uint4 (&M)[4], uint4 (&L)[4]) {
    uint32_t h[8][4], m[8][4], l[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x2 xy = {v[j].x, v[j].y}, zw = {v[j].z, v[j].w};
        h[j][0] = __float_as_uint(xy.x) & 0xffff0000u; h[j][1] = __float_as_uint(xy.y) & 0xffff0000u;
        h[j][2] = __float_as_uint(zw.x) & 0xffff0000u; h[j][3] = __float_as_uint(zw.y) & 0xffff0000u;
        const f32x2 hxy = {__uint_as_float(h[j][0]), __uint_as_float(h[j][1])}, hzw = {__uint_as_float(h[j][2]), __uint_as_float(h[j][3])};
        const f32x2 r1xy = xy - hxy, r1zw = zw - hzw;                       // exact
        m[j][0] = __float_as_uint(r1xy.x) & 0xffff0000u; m[j][1] = __float_as_uint(r1xy.y) & 0xffff0000u;
        m[j][2] = __float_as_uint(r1zw.x) & 0xffff0000u; m[j][3] = __float_as_uint(r1zw.y) & 0xffff0000u;
        const f32x2 mxy = {__uint_as_float(m[j][0]), __uint_as_float(m[j][1])}, mzw = {__uint_as_float(m[j][2]), __uint_as_float(m[j][3])};
        const f32x2 r2xy = r1xy - mxy, r2zw = r1zw - mzw;                   // exact, <= 8 significant bits
        l[j][0] = __float_as_uint(r2xy.x); l[j][1] = __float_as_uint(r2xy.y);
        l[j][2] = __float_as_uint(r2zw.x); l[j][3] = __float_as_uint(r2zw.y);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        H[c] = make_uint4(pack_hi16(h[0][c], h[1][c]), pack_hi16(h[2][c], h[3][c]), pack_hi16(h[4][c], h[5][c]), pack_hi16(h[6][c], h[7][c]));
        M[c] = make_uint4(pack_hi16(m[0][c], m[1][c]), pack_hi16(m[2][c], m[3][c]), pack_hi16(m[4][c], m[5][c]), pack_hi16(m[6][c], m[7][c]));
        L[c] = make_uint4(pack_hi16(l[0][c], l[1][c]), pack_hi16(l[2][c], l[3][c]), pack_hi16(l[4][c], l[5][c]), pack_hi16(l[6][c], l[7][c]));
    }
}

// Consecutive workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2). Blocks that share operand
// rows (all k slabs of one row slab re-read the same dY rows) should share an L2: logical id = the id's position
// within its XCD's stream, so consecutive LOGICAL blocks run on one XCD. (PMC: 1.04 GB fetched per step's weight
// gradients against 0.74 GB algorithmic before - every XCD fetched its own copy of each dY slab.)
__device__ __forceinline__ int xcd_logical_block(int bid, int nblocks) {
    constexpr int XCDS = 8;
    const int per = nblocks / XCDS, rem = nblocks % XCDS;       // XCD x runs per + (x < rem) blocks
    const int x = bid % XCDS, local = bid / XCDS;
    return x * per + (x < rem ? x : rem) + local;
}

struct WgradGroup {
    const float* dY[LLMREC_LINEAR_MAX_PROBLEMS];
    const float* X[LLMREC_LINEAR_MAX_PROBLEMS];
    int64_t lddy[LLMREC_LINEAR_MAX_PROBLEMS];
    int64_t ldx[LLMREC_LINEAR_MAX_PROBLEMS];
    int64_t M[LLMREC_LINEAR_MAX_PROBLEMS];
    const float* db_w[LLMREC_LINEAR_MAX_PROBLEMS];         // [M] or null: the bias gradient is sum_r db_w[r] dY[r] (v2 body only)
    const int32_t* rows[LLMREC_LINEAR_MAX_PROBLEMS];       // or null: ascending ids of the rows of dY that can be non-zero (v2 body only)
    const int32_t* n_rows[LLMREC_LINEAR_MAX_PROBLEMS];     // device scalar: entries of rows[]
    int32_t vec_ok[LLMREC_LINEAR_MAX_PROBLEMS];
    int32_t chunk_begin[LLMREC_LINEAR_MAX_PROBLEMS + 1];   // first partial slab of each problem
    int32_t n_problems;
};

// Several Linears' weight gradients in one launch (llmrec_linear_wgrad_multi_bf16x3): target t owns the logical blocks
// [block_begin[t], block_begin[t + 1]), its own K, slab count and partial buffers; one slab length for all of them, so every
// block of the launch has the same amount of work.
struct WgradMulti {
    WgradGroup g[LLMREC_WGRAD_MAX_TARGETS];
    float* partial[LLMREC_WGRAD_MAX_TARGETS];
    float* partial_db[LLMREC_WGRAD_MAX_TARGETS];
    int32_t K[LLMREC_WGRAD_MAX_TARGETS], n_kslab[LLMREC_WGRAD_MAX_TARGETS], n_slabs[LLMREC_WGRAD_MAX_TARGETS];
    int32_t block_begin[LLMREC_WGRAD_MAX_TARGETS + 1];
    int32_t n_targets;
    int64_t MC;
};

// ---------------------------------------------------------------------------------------------
// Weight gradient, second organisation (round 3): v_mfma_f32_32x32x16_bf16, wave tile = 64 n x 128 k over 16-row steps.
//   * the 32x32x16 MFMA holds the VALU for 8 of its 32 cycles (the 16x16x32 one for 8 of 16, profiles/r02_coexec_mfma_valu.txt) and
//     a 128-wide k slab halves the dY loads / splits per X byte (dY is re-read and re-split by every k slab of a row slab);
//   * lane (i = lane & 31, h = lane >> 5) supplies the rows m0 + 8 h + j (j = 0..7) of ITS columns to the contraction slots
//     (h, j) of both operands: X as float4 at k = k0 + 4 i + c (component c -> B tile c: four interleaved 32-column tiles,
//     one instruction = two rows x 512 contiguous bytes), dY as float2 at n = 2 i + t (component t -> A tile t);
//   * D tile (t, c): column = lane & 31 -> k = k0 + 4 (lane & 31) + c, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -> n = 2 row + t;
//   * the four waves of a block (four consecutive row slabs of one k slab) are summed through LDS by ALL four waves
//     (each adds its quarter of the tile in wave order: deterministic) before one partial slab is written.
// Measured against five other organisations (producer / consumer pairs, loader waves, two waves per SIMD, ...): profiles/experiments/r03_wgrad.md.
// ---------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x16 mfma32_bf16(const uint4& a, const uint4& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ float2 load2_global(global_cptr base, uint32_t byte_off) {
    typedef float raw2 __attribute__((ext_vector_type(2)));
    typedef const raw2 __attribute__((address_space(1))) * graw2;
    const raw2 v = *(graw2)(base + byte_off);
    return make_float2(v.x, v.y);
}
// 8 float2 (rows j = 0..7 of one lane; component t belongs to tile t) -> the three bf16x8 fragments of both tiles
__device__ __forceinline__ void split16(const float2 (&v)[8], uint4 (&H)[2], uint4 (&M)[2], uint4 (&L)[2]) {
    uint32_t h[8][2], m[8][2], l[8][2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x2 xy = {v[j].x, v[j].y};
        h[j][0] = __float_as_uint(xy.x) & 0xffff0000u; h[j][1] = __float_as_uint(xy.y) & 0xffff0000u;
        const f32x2 hxy = {__uint_as_float(h[j][0]), __uint_as_float(h[j][1])};
        const f32x2 r1 = xy - hxy;                                          // exact
        m[j][0] = __float_as_uint(r1.x) & 0xffff0000u; m[j][1] = __float_as_uint(r1.y) & 0xffff0000u;
        const f32x2 mxy = {__uint_as_float(m[j][0]), __uint_as_float(m[j][1])};
        const f32x2 r2 = r1 - mxy;                                          // exact, <= 8 significant bits
        l[j][0] = __float_as_uint(r2.x); l[j][1] = __float_as_uint(r2.y);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        H[t] = make_uint4(pack_hi16(h[0][t], h[1][t]), pack_hi16(h[2][t], h[3][t]), pack_hi16(h[4][t], h[5][t]), pack_hi16(h[6][t], h[7][t]));
        M[t] = make_uint4(pack_hi16(m[0][t], m[1][t]), pack_hi16(m[2][t], m[3][t]), pack_hi16(m[4][t], m[5][t]), pack_hi16(m[6][t], m[7][t]));
        L[t] = make_uint4(pack_hi16(l[0][t], l[1][t]), pack_hi16(l[2][t], l[3][t]), pack_hi16(l[4][t], l[5][t]), pack_hi16(l[6][t], l[7][t]));
    }
}

#ifdef LLMREC_TOOLS_BUILD
// instrumented build (python -m llmrec_amd.build --tools): every wave adds the span of its main loop in shader cycles and in ticks of
// the constant 100 MHz counter -> the EFFECTIVE shader clock of the launch (tools/wgrad_probe.py; profiles/experiments/r03_wgrad.md)
static __device__ unsigned long long g_wgrad_clock[3];      // (one per translation unit; llmrec_tools_wgrad_clock reads dense.hip's)
#endif

typedef const int32_t __attribute__((address_space(4))) * const_i32p;   // constant address space: uniform loads become SCALAR loads
typedef const float __attribute__((address_space(4))) * const_f32p;
constexpr int W2_KW = 128;                                  // k columns per wave
constexpr int W2_RED_FLOATS = 4 * 128 * 64 + 4 * 64;        // LDS of the block's final reduction (129 KB)

// The accumulation loop of one wave over the rows [m_begin, m_end) of one problem. LISTED: the rows are positions in the problem's
// ascending ROW LIST (llmrec_wgrad_problem_t.row_list: the rows of dY that can be non-zero); position p reads row rows[p] of dY and X.
//   dense:  a tile's buffer descriptor = (address of its first row, bytes up to the slab's end), the lane's eight row offsets are constants;
//   listed: one descriptor per operand over the whole tensor; the 16 row ids of a tile arrive by SCALAR loads (their own counter: they
//           do not queue behind the vector loads) one tile ahead of the tile's operand loads, offset = id * row stride + column.
// Either way no row past the end is read as anything but zero (the buffer's range check), so ragged tiles and prefetches past the end
// need no special case.
template <bool LISTED>
__device__ __forceinline__ void wgrad_v2_accumulate(const WgradGroup& g, const int prob, const int kslab, const int nblk, const int64_t m_begin64,
                                                    const int64_t m_end64, const bool want_db, f32x16 (&acc)[2][4], f32x2& dbs2) {
    const int lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const int64_t lddy = g.lddy[prob], ldx = g.ldx[prob], M = g.M[prob];
    // row positions as wave-uniform 32-bit scalars (M < 2^30 is checked by the host)
    const int m_begin = __builtin_amdgcn_readfirstlane((int)m_begin64), m_end = __builtin_amdgcn_readfirstlane((int)m_end64);
    const int n_base = nblk * 64 + 2 * i;                         // this lane's 2 n's: n_base + t
    const int k_base = kslab * W2_KW + 4 * i;                     // this lane's 4 k's: k_base + c
    const uint32_t la = 4u * (uint32_t)lddy, lbx = 4u * (uint32_t)ldx;             // row strides in bytes
    uint32_t offa[8], offb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        offa[j] = (LISTED ? 0u : (uint32_t)(8 * h + j) * la) + 4u * (uint32_t)n_base;
        offb[j] = (LISTED ? 0u : (uint32_t)(8 * h + j) * lbx) + 4u * (uint32_t)k_base;
    }
    const char* dYb = reinterpret_cast<const char*>(uniform_u64(g.dY[prob]));
    const char* Xb = reinterpret_cast<const char*>(uniform_u64(g.X[prob]));
    const const_i32p rl = LISTED ? (const_i32p)uniform_u64(g.rows[prob]) : (const_i32p)0;
    const int n_tiles = (m_end - m_begin + 15) / 16;             // the last tile may be ragged: its missing rows read as zero
    constexpr uint32_t OOB = 0x80000000u;                        // beyond any listed problem's tensor (checked by the host: bytes < 2^31)
    __amdgpu_buffer_rsrc_t ra_all, rb_all;
    if (LISTED) {
        ra_all = __builtin_amdgcn_make_buffer_rsrc((void*)dYb, 0, (int)((uint32_t)M * la), 0x00020000);
        rb_all = __builtin_amdgcn_make_buffer_rsrc((void*)Xb, 0, (int)((uint32_t)M * lbx), 0x00020000);
    }
    // LISTED: the ids of the 16 rows of the tile at position m0 (uniform address: scalar loads); positions past the last tile re-read it
    const int m_last = n_tiles > 0 ? m_begin + 16 * (n_tiles - 1) : m_begin;
    auto load_ids = [&](int m0, int32_t (&ids)[16]) {
        if (LISTED) {
            const const_i32p q = rl + (m0 < m_last ? m0 : m_last);
#pragma unroll
            for (int r = 0; r < 16; ++r) ids[r] = q[r];
        }
    };
    auto load_tile = [&](int m0, const int32_t (&ids)[16], float2 (&aa)[8], float4 (&bb)[8]) {
        if (LISTED) {
            const int left = m_end - m0 - 8 * h;                     // this half's rows j < left are inside the list
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t id = (uint32_t)(h ? ids[8 + j] : ids[j]);
                const bool ok = j < left;
                const u32x2 va = __builtin_amdgcn_raw_buffer_load_b64(ra_all, ok ? id * la + offa[j] : OOB, 0, 0);
                const u32x4 vb = __builtin_amdgcn_raw_buffer_load_b128(rb_all, ok ? id * lbx + offb[j] : OOB, 0, 0);
                aa[j] = make_float2(__uint_as_float(va.x), __uint_as_float(va.y));
                bb[j] = make_float4(__uint_as_float(vb.x), __uint_as_float(vb.y), __uint_as_float(vb.z), __uint_as_float(vb.w));
            }
        } else {
            const int mc = m0 < m_end ? m0 : m_end;                  // wave-uniform; at m_end the buffers are empty: zeros
            const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(dYb + (uint64_t)mc * la), 0, (int)((uint32_t)(m_end - mc) * la), 0x00020000);
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(Xb + (uint64_t)mc * lbx), 0, (int)((uint32_t)(m_end - mc) * lbx), 0x00020000);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32x2 va = __builtin_amdgcn_raw_buffer_load_b64(ra, offa[j], 0, 0);
                const u32x4 vb = __builtin_amdgcn_raw_buffer_load_b128(rb, offb[j], 0, 0);
                aa[j] = make_float2(__uint_as_float(va.x), __uint_as_float(va.y));
                bb[j] = make_float4(__uint_as_float(vb.x), __uint_as_float(vb.y), __uint_as_float(vb.z), __uint_as_float(vb.w));
            }
        }
    };
    // bias gradient: column sums of dY, optionally weighted per row (a pre-propagated operand: db = sum_r (A 1)[r] dY[r]); only the
    // k-slab-0 waves' sums are written, so only they fetch the weights (16 scalar loads per tile, rows clamped into the problem)
    const const_f32p dbw = want_db ? (const_f32p)uniform_u64(g.db_w[prob]) : (const_f32p)0;
    auto mma_tile = [&](int m0, const int32_t (&ids)[16], const float2 (&aa)[8], const float4 (&bb)[8]) {
        if (dbw) {                                                   // wave-uniform
            const int last = (int)M - 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int r0, r1;
                if (LISTED) {                                        // (a position past the end has a zero dY row: any weight will do)
                    r0 = m0 + j < m_end ? ids[j] : 0; r1 = m0 + 8 + j < m_end ? ids[8 + j] : 0;
                } else {
                    r0 = m0 + j < last ? m0 + j : last; r1 = m0 + 8 + j < last ? m0 + 8 + j : last;
                }
                const float w0 = dbw[r0], w1 = dbw[r1];              // uniform addresses: scalar loads
                const float wj = h ? w1 : w0;
                dbs2.x = fmaf(wj, aa[j].x, dbs2.x); dbs2.y = fmaf(wj, aa[j].y, dbs2.y);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const f32x2 v = {aa[j].x, aa[j].y}; dbs2 += v; }
        }
        uint4 bh[4], bm[4], bl[4], ah[2], am[2], al[2];
        split32(bb, bh, bm, bl);
        split16(aa, ah, am, al);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // smallest terms first (as in the forward)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(al[t], bh[c], acc[t][c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(ah[t], bl[c], acc[t][c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(am[t], bm[c], acc[t][c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(am[t], bh[c], acc[t][c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(ah[t], bm[c], acc[t][c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = mfma32_bf16(ah[t], bh[c], acc[t][c]);
        }
    };
    // two register stages rotate statically; the loop body is straight-line (pairs of tiles), an odd last tile follows it.
    // (LISTED: c0 / c1 = the ids of the tiles held in stages 0 / 1 (the bias weights of mma_tile index by them); nx = the ids of the NEXT tile
    //  to load, fetched right after the previous tile's operand loads were issued, i.e. a whole multiply phase ahead of their use)
    float2 a0[8], a1[8];
    float4 b0[8], b1[8];
    int32_t c0[16] = {}, c1[16] = {}, nx[16] = {};
    auto keep = [&](int32_t (&dst)[16]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[r] = nx[r];
    };
    int m0 = m_begin;
    load_ids(m0, nx);
    load_tile(m0, nx, a0, b0); keep(c0);
    load_ids(m0 + 16, nx);
#ifdef LLMREC_TOOLS_BUILD
    const long long clk0 = clock64(), ref0 = wall_clock64();
#endif
    for (int g2 = n_tiles >> 1; g2 > 0; --g2) {
        load_tile(m0 + 16, nx, a1, b1); keep(c1);
        load_ids(m0 + 32, nx);
        __builtin_amdgcn_sched_barrier(0);
        mma_tile(m0, c0, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        load_tile(m0 + 32, nx, a0, b0); keep(c0);
        load_ids(m0 + 48, nx);
        __builtin_amdgcn_sched_barrier(0);
        mma_tile(m0 + 16, c1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        m0 += 32;
    }
#ifdef LLMREC_TOOLS_BUILD
    if (lane == 0) { atomicAdd(&g_wgrad_clock[0], (unsigned long long)(clock64() - clk0)); atomicAdd(&g_wgrad_clock[1], (unsigned long long)(wall_clock64() - ref0)); atomicAdd(&g_wgrad_clock[2], 1ull); }
#endif
    if (n_tiles & 1) mma_tile(m0, c0, a0, b0);
}

__device__ __forceinline__ void wgrad_bf16x3_v2_body(const WgradGroup& g, int N, int K, float* __restrict__ partial,
                                                     float* __restrict__ partial_db, int64_t MC, int n_kslab, int n_slabs, int lb, float* red) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int kslab = lb % n_kslab;
    const int group = lb / n_kslab;
    const int slab_raw = group * 4 + wave;
    const bool active = slab_raw < n_slabs;
    const int slab = active ? slab_raw : n_slabs - 1;             // idle waves of the last group recompute a slab and drop it
    int prob = 0;
    while (prob + 1 < g.n_problems && slab >= g.chunk_begin[prob + 1]) ++prob;
    const int nblk = blockIdx.y;
    const bool listed = g.rows[prob] != nullptr;                  // wave-uniform
    // a listed problem's slabs are equal pieces of the ACTUAL list length (read here), whatever length the host laid the launch out for
    int64_t M = g.M[prob], mc = MC;
    if (listed) {
        M = *reinterpret_cast<const int32_t*>(uniform_u64(g.n_rows[prob]));
        M = M < 0 ? 0 : (M > g.M[prob] ? g.M[prob] : M);
        const int64_t ns = g.chunk_begin[prob + 1] - g.chunk_begin[prob];
        mc = ((M + ns - 1) / ns + 15) / 16 * 16;
        if (mc < 16) mc = 16;
    }
    int64_t m_begin = (int64_t)(slab - g.chunk_begin[prob]) * mc;
    if (m_begin > M) m_begin = (M + 15) / 16 * 16;                // an empty slab (16-aligned: the id loads stay aligned and inside the list's padding)
    const int64_t m_end = (m_begin + mc < M) ? m_begin + mc : (m_begin < M ? M : m_begin);

    f32x16 acc[2][4];                                             // [t][c]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][c][r] = 0.f;
    f32x2 dbs2 = {0.f, 0.f};
    const bool want_db = kslab == 0 && partial_db;
    if (listed) wgrad_v2_accumulate<true>(g, prob, kslab, nblk, m_begin, m_end, want_db, acc, dbs2);
    else wgrad_v2_accumulate<false>(g, prob, kslab, nblk, m_begin, m_end, want_db, acc, dbs2);
    float2 dbs = make_float2(dbs2.x, dbs2.y);
    dbs.x += __shfl_xor(dbs.x, 32, 64); dbs.y += __shfl_xor(dbs.y, 32, 64);
    // element (t, c, r) of lane l at [wave][((t * 4 + c) * 16 + r) * 64 + l]: conflict-free
    float* rw = red + wave * (128 * 64);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) rw[((t * 4 + c) * 16 + r) * 64 + lane] = active ? acc[t][c][r] : 0.f;
    if (h == 0) {
        red[4 * 128 * 64 + wave * 64 + 2 * i + 0] = active ? dbs.x : 0.f;
        red[4 * 128 * 64 + wave * 64 + 2 * i + 1] = active ? dbs.y : 0.f;
    }
    __syncthreads();
    // wave w adds rows t = w >> 1, reg r in [8 (w & 1), +8) of all four waves' tiles, in wave order (slab 4 g, +1, +2, +3)
    float* pw = partial + (int64_t)group * N * K;
    const int t_out = wave >> 1;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * (wave & 1) + rr;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = ((t_out * 4 + c) * 16 + r) * 64 + lane;
            v[c] = ((red[e] + red[128 * 64 + e]) + red[2 * 128 * 64 + e]) + red[3 * 128 * 64 + e];
        }
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int n = nblk * 64 + 2 * row + t_out;
        *reinterpret_cast<float4*>(pw + (int64_t)n * K + kslab * W2_KW + 4 * i) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (kslab == 0 && partial_db && wave == 0) {
        const float* rd = red + 4 * 128 * 64;
        partial_db[(int64_t)group * N + nblk * 64 + lane] = ((rd[lane] + rd[64 + lane]) + rd[128 + lane]) + rd[192 + lane];
    }
}

// wgrad_host.hip: the launch of blocks [0, wg_blocks) = the multi-target weight gradient m and n_cu - wg_blocks persistent guests that
// run the hosted product a (laid out for 256-thread blocks: spmm_prepare_hosted). The caller has made every check.
int wgrad_multi_host_launch(const WgradMulti& m, int N, int wg_blocks, int n_cu, const SpmmArgs& a, hipStream_t stream);

}  // namespace llmrec
