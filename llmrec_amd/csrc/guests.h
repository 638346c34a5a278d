// guests.h - the block bodies of three short launches of the step, over a VIRTUAL block id and with the block size as a compile-time
// parameter, so that each runs as a launch of its own (bpr.hip: 256 / 256 / 1024 threads) or as the leading GUEST blocks of a grouped
// SpMM launch (spmm.hip: llmrec_spmm_multi_guest_f32, 512 threads): the wide sampler (llmrec_sample_batch_wide), the scatter plan with
// the reach marks (llmrec_bpr_scatter_plan_reach_mark) and the loss values (llmrec_bpr_multi_losses_assemble_f32). What a 16-lane group
// or a wavefront does per slot, key or tree - and the order of its additions - does not depend on the block size: only which block
// holds it does. Each body's argument checks and launch geometry live here too, shared by both entry points. reach.h is the precedent.
#pragma once
#include "common.h"
#include "reach.h"

namespace llmrec {

__device__ __forceinline__ int bpr_batch(const int32_t* n_valid_dev, int B_max) {
    int B = n_valid_dev ? n_valid_dev[0] : B_max;
    return B > B_max ? B_max : (B < 0 ? 0 : B);
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 counter-based generator (Salmon et al., SC'11)
// ---------------------------------------------------------------------------------------------
struct Philox {
    uint32_t key[2];
    __device__ Philox(uint64_t seed) { key[0] = (uint32_t)seed; key[1] = (uint32_t)(seed >> 32); }
    __device__ void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) const {
        uint32_t k0 = key[0], k1 = key[1];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
            const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    }
};

__device__ __forceinline__ uint32_t bounded(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// Keyed bijection of [0, n): 4-round Feistel on 2h bits (2^(2h) >= n) with cycle walking.
__device__ inline uint64_t keyed_perm(uint64_t x, uint64_t n, int half_bits, const Philox& ph, uint32_t step_lo, uint32_t step_hi) {
    const uint64_t mask = (1ull << half_bits) - 1;
    do {
        uint64_t L = x >> half_bits, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint32_t o[4];
            ph((uint32_t)R, (uint32_t)(R >> 32) ^ (0xA5A50000u + r), step_lo, step_hi, o);
            const uint64_t f = (((uint64_t)o[1] << 32) | o[0]) & mask;
            const uint64_t nL = R, nR = L ^ f;
            L = nL; R = nR;
        }
        x = (L << half_bits) | R;
    } while (x >= n);
    return x;
}

// one BPR triple of the global batch: user slot b of B (without replacement while B <= n_exist), a uniform
// train item of that user, a uniform non-train item by rejection (binary search in the sorted row)
__device__ __forceinline__ int64_t sample_user(const Philox& ph, uint32_t slo, uint32_t shi, int b, int B, int half_bits,
                                               int64_t n_exist, const int64_t* __restrict__ exist_users) {
    // users: without replacement while B <= n_exist (rd.sample), with replacement otherwise (rd.choice)
    uint64_t slot;
    if ((int64_t)B <= n_exist) {
        slot = keyed_perm((uint64_t)b, (uint64_t)n_exist, half_bits, ph, slo, shi);
    } else {
        uint32_t o[4];
        ph((uint32_t)b, 0x55AA0001u, slo, shi, o);
        slot = ((((uint64_t)o[1] << 32) | o[0]) % (uint64_t)n_exist);
    }
    return exist_users[slot];
}

__device__ __forceinline__ void sample_one(const Philox& ph, uint32_t slo, uint32_t shi, int b, int B, int half_bits,
                                           int64_t n_exist, const int64_t* __restrict__ exist_users, int64_t n_items,
                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                           int64_t& u_out, int64_t& p_out, int64_t& q_out) {
    const int64_t u = sample_user(ph, slo, shi, b, B, half_bits, n_exist, exist_users);
    const int32_t s = rowptr[u], e = rowptr[u + 1];
    uint32_t o[4];
    ph((uint32_t)b, 0x55AA0002u, slo, shi, o);
    const int64_t p = colidx[s + (int32_t)bounded(o[0], (uint32_t)(e - s))];
    int64_t q = 0;
    uint32_t ctr = 0;
    int have = 4;
    for (int tries = 0; tries < 4096; ++tries) {
        if (have == 4) { ph((uint32_t)b, 0x55AA0003u + ctr, slo, shi, o); ++ctr; have = 0; }
        const uint32_t r = o[have++];
        q = n_items <= 0xffffffffll ? (int64_t)bounded(r, (uint32_t)n_items) : (int64_t)(r % (uint64_t)n_items);
        int32_t lo = s, hi = e;                                         // binary search in the sorted row
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (colidx[mid] < q) lo = mid + 1; else hi = mid;
        }
        if (!(lo < e && colidx[lo] == q)) break;                        // not a train item: accept
    }
    u_out = u; p_out = p; q_out = q;
}

// ---------------------------------------------------------------------------------------------
// The wide sampler (llmrec_sample_batch_wide): the BPR slots go to blocks of NT threads - at B = 1024 and NT = 256 no SIMD holds more than one
// sampling wavefront, where the single block stacks four of them on one CU - and ONE further block draws the augmented triples
// on its own: it recomputes the user of each chosen slot (the same keyed permutation / with-replacement draw that wrote users[slot], so
// the same value) instead of waiting for the other blocks, compacts in draw order, pads and writes n_valid. Every block reads the step
// first; after its last use it takes a ticket (device-scope atomic increment), and the block that draws the last one advances the
// counter and puts the ticket word back to 0 - nobody waits for anybody, and a graph replay needs no host action.
// ---------------------------------------------------------------------------------------------
struct SamplerArgs {
    uint64_t seed;
    unsigned long long* step_dev;
    int64_t n_exist;
    const int64_t* exist_users;
    int64_t n_items;
    const int32_t* rowptr;
    const int32_t* colidx;
    int B_global, half_bits_users, slice_begin, B, n_aug, half_bits_batch;
    const int64_t* aug_pos;
    const int64_t* aug_neg;
    int64_t* users;
    int64_t* pos;
    int64_t* neg;
    int32_t* n_valid_dev;
    int32_t* ticket;
    int n_blocks;                                                      // ceil(B / NT) + 1 (guest_blocks)
};

template <int NT>
__device__ __forceinline__ void guest_block(const SamplerArgs& a, int vb, char*) {
    __shared__ int wave_tot[NT / 64];
    __shared__ int base_s;
    const int B = a.B, n_aug = a.n_aug;
    const int64_t n_items = a.n_items;
    int64_t* __restrict__ users = a.users;
    int64_t* __restrict__ pos = a.pos;
    int64_t* __restrict__ neg = a.neg;
    const unsigned long long step = *a.step_dev;
    const uint32_t slo = (uint32_t)step, shi = (uint32_t)(step >> 32);
    const Philox ph(a.seed);
    if (vb + 1 < a.n_blocks) {                                          // block-uniform: NT BPR slots
        const int b = vb * NT + threadIdx.x;
        if (b < B)
            sample_one(ph, slo, shi, a.slice_begin + b, a.B_global, a.half_bits_users, a.n_exist, a.exist_users, n_items, a.rowptr, a.colidx,
                       users[b], pos[b], neg[b]);
    } else {                                                            // the last block: the augmented triples
        if (threadIdx.x == 0) base_s = 0;
        __syncthreads();
        const Philox pa(a.seed ^ 0x9E3779B97F4A7C15ull);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int a0 = 0; a0 < n_aug; a0 += NT) {                        // block-uniform
            const int ai = a0 + threadIdx.x;
            int64_t u = 0, ap = 0, an = 0;
            bool ok = false;
            if (ai < n_aug) {
                const uint64_t slot = keyed_perm((uint64_t)ai, (uint64_t)B, a.half_bits_batch, pa, slo, shi);   // distinct slots of the slice
                u = sample_user(ph, slo, shi, a.slice_begin + (int)slot, a.B_global, a.half_bits_users, a.n_exist, a.exist_users);   // = users[slot]
                ap = a.aug_pos[u]; an = a.aug_neg[u];
                ok = ap >= 0 && an >= 0 && ap < n_items && an < n_items;
            }
            const unsigned long long bal = __ballot(ok);
            const int before = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wave_tot[wv] = __popcll(bal);
            __syncthreads();
            int wave_base = 0, chunk_tot = 0;
            for (int k = 0; k < NT / 64; ++k) { const int t = wave_tot[k]; if (k < wv) wave_base += t; chunk_tot += t; }
            const int base = base_s;
            if (ai < n_aug && ok) {
                const int o = B + base + wave_base + before;
                users[o] = u; pos[o] = ap; neg[o] = an;
            }
            __syncthreads();
            if (threadIdx.x == 0) base_s = base + chunk_tot;
            __syncthreads();
        }
        const int kept = base_s;
        for (int o = B + kept + threadIdx.x; o < B + n_aug; o += NT) { users[o] = 0; pos[o] = 0; neg[o] = 0; }   // padding (never read: beyond n_valid)
        if (threadIdx.x == 0) a.n_valid_dev[0] = B + kept;
    }
    __syncthreads();                                                    // every thread of this block is done with the step's value
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(a.ticket, 1) == a.n_blocks - 1) {                 // the last block: every block has read the counter
            *a.step_dev = step + 1ull;
            atomicExch(a.ticket, 0);
        }
    }
}

// The checks of llmrec_sample_batch_wide (who: the entry point's name in the error text) and the launch geometry for blocks of nt threads.
static inline int guest_prepare(const llmrec_guest_sampler_t& g, int nt, const char* who, SamplerArgs& a, int64_t& blocks, size_t& shmem) {
    LLMREC_CHECK_ARG(g.B >= 1 && g.B_global >= g.B && g.slice_begin >= 0 && g.slice_begin + g.B <= g.B_global && g.n_aug >= 0 && g.n_aug <= g.B &&
                     g.n_exist_users > 0 && g.n_items > 0, "%s: bad sizes", who);
    LLMREC_CHECK_ARG(g.step_dev && g.exist_users && g.train_rowptr && g.train_colidx && g.users && g.pos && g.neg && g.n_valid_dev && g.ticket,
                     "%s: null pointer", who);
    LLMREC_CHECK_ARG(g.n_aug == 0 || (g.aug_pos && g.aug_neg), "%s: augmented pairs missing", who);
    int hb_users = 1, hb_batch = 1;
    while ((1ull << (2 * hb_users)) < (uint64_t)g.n_exist_users) ++hb_users;
    while ((1ull << (2 * hb_batch)) < (uint64_t)g.B) ++hb_batch;
    blocks = ceil_div(g.B, nt) + 1;
    shmem = 0;
    a = SamplerArgs{g.seed, (unsigned long long*)g.step_dev, g.n_exist_users, g.exist_users, g.n_items, g.train_rowptr, g.train_colidx,
                    g.B_global, hb_users, g.slice_begin, g.B, g.n_aug, hb_batch, g.aug_pos, g.aug_neg, g.users, g.pos, g.neg, g.n_valid_dev,
                    g.ticket, (int)blocks};
    return LLMREC_OK;
}

// ---------------------------------------------------------------------------------------------
// The scatter plan's body (the comment on the deterministic gradient scatter in bpr.hip) and, behind its blocks, the reach marks.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t PLAN_NO_ID = 0xffffffffu;
static inline int64_t plan_blocks_for(int B_max, int nt) { return ceil_div(B_max, nt / 16) + ceil_div(2 * (int64_t)B_max, nt / 16); }

// vb: the block's index among the plan's ceil(B_max / (NT / 16)) + ceil(2 B_max / (NT / 16)) blocks; k: 2 B_max keys of LDS
template <int NT>
__device__ __forceinline__ void bpr_plan_block(int vb, uint64_t* k, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                               const int64_t* __restrict__ neg, int B_max,
                                               const int32_t* __restrict__ n_valid_dev, uint64_t* __restrict__ plan) {
    constexpr int GROUPS = NT / 16;
    const int B = bpr_batch(n_valid_dev, B_max);
    const int nbu = (B_max + GROUPS - 1) / GROUPS;
    const bool items = vb >= nbu;
    const int n = items ? 2 * B_max : B_max;
    for (int i = threadIdx.x; i < n; i += NT) {
        const int b = (items && i >= B_max) ? i - B_max : i;
        uint64_t id = PLAN_NO_ID;
        if (b < B) id = (uint64_t)(items ? (i >= B_max ? neg[b] : pos[b]) : users[b]);
        k[i] = (id << 32) | (uint64_t)(uint32_t)i;
    }
    __syncthreads();
    const int gl = threadIdx.x & 15;
    const int i = (vb - (items ? nbu : 0)) * GROUPS + (threadIdx.x >> 4);
    if (i >= n) return;
    const uint64_t me = k[i];
    const uint32_t id = (uint32_t)(me >> 32);
    int below = 0, lower_id = 0, same_id = 0;
    for (int j = gl; j < n; j += 16) {
        const uint64_t kj = k[j];
        const uint32_t idj = (uint32_t)(kj >> 32);
        below += kj < me; lower_id += idj < id; same_id += idj == id;
    }
    below = (int)group_sum<16>((float)below); lower_id = (int)group_sum<16>((float)lower_id); same_id = (int)group_sum<16>((float)same_id);   // < 2^24: exact
    if (gl == 0) {
        const int base = items ? B_max : 0;
        plan[base + below] = me;
        int32_t* runlen = reinterpret_cast<int32_t*>(plan + 3 * (int64_t)B_max);
        runlen[base + below] = (below == lower_id && id != PLAN_NO_ID) ? same_id : 0;
    }
}

struct PlanReachArgs {
    const int64_t* users;
    const int64_t* pos;
    const int64_t* neg;
    int B_max;
    const int32_t* n_valid_dev;
    uint64_t* plan;
    int plan_blocks;
    int64_t n_users, n_items;
    const int32_t* item_rowptr;
    const int32_t* item_colidx;
    uint8_t* flags;
};

// blocks [0, plan_blocks) run the plan's body, the blocks behind them llmrec_batch_reach_rows' marking body (reach.h). Both read the
// sampled batch only and neither reads what the other writes.
template <int NT>
__device__ __forceinline__ void guest_block(const PlanReachArgs& a, int vb, char* smem) {
    if (vb < a.plan_blocks)                                              // block-uniform
        bpr_plan_block<NT>(vb, reinterpret_cast<uint64_t*>(smem), a.users, a.pos, a.neg, a.B_max, a.n_valid_dev, a.plan);
    else
        batch_reach_mark_block<NT>(vb - a.plan_blocks, a.B_max, a.n_valid_dev, a.users, a.pos, a.neg, a.n_users, a.n_items, a.item_rowptr,
                                   a.item_colidx, a.flags);
}

// The checks of llmrec_bpr_scatter_plan_reach_mark; blocks == 0: an empty capacity, nothing to launch.
static inline int guest_prepare(const llmrec_guest_plan_reach_t& g, int nt, const char* who, PlanReachArgs& a, int64_t& blocks, size_t& shmem) {
    blocks = 0; shmem = 0;
    LLMREC_CHECK_ARG(g.B_max >= 0 && g.n_users > 0 && g.n_users < 0x7fffffffll && g.n_items > 0, "%s: bad sizes", who);
    LLMREC_CHECK_ARG(g.item_rowptr && g.item_colidx && g.flags, "%s: null pointer", who);
    if (g.B_max > LLMREC_BPR_MAX_B) { set_error("%s: B_max %d > %d", who, g.B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    if (g.B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(g.users && g.pos && g.neg && g.plan, "%s: null pointer", who);
    const int plan_blocks = (int)plan_blocks_for(g.B_max, nt);
    blocks = plan_blocks + reach_mark_blocks(g.B_max, nt);
    shmem = sizeof(uint64_t) * 2 * (size_t)g.B_max;                      // <= 64 KB of LDS
    a = PlanReachArgs{g.users, g.pos, g.neg, g.B_max, g.n_valid_dev, g.plan, plan_blocks, g.n_users, g.n_items, g.item_rowptr, g.item_colidx,
                      g.flags};
    return LLMREC_OK;
}

// ---------------------------------------------------------------------------------------------
// The logged scalars of a fused step in ONE single-block launch (llmrec_bpr_multi_losses_assemble_f32): the loss values of every
// problem, the feature regulariser from the fusion launch's per-block partial sums, and the assembly of llmrec_loss_assemble_f32
// mode 0. Every sum is bpr_reduce_kernel's / block_tree_sum's: slot v of 1024 is the sum over b = v, v + 1024, ... in ascending order
// from 0.f, then the pairwise tree red[i] += red[i + off], off = 512 ... 1. Here ONE WAVEFRONT owns a tree: lane l holds slots
// l, l + 64, ..., l + 960 in 16 registers, levels 512 ... 64 are register adds r[j] += r[j + off / 64], levels 32 ... 1 are
// __shfl_down adds (only lanes below `off` matter; lane 0 ends with red[0]) - the same additions on the same operands, so the bits of
// out / saved / scal are those of the 1024-slot LDS tree, without its block barriers and its 32 KB of LDS. A round's 16 loads of a lane
// are issued together: the LDS version, and this one while its loads sat in per-slot loops, waited for every load on its own (22 us
// and 21 us on the step's stream against 8.6 us). The 4 n_prob + 1 trees are dealt to the block's NT / 64 wavefronts (16 in the launch
// of its own; 8, two rounds, as a guest).
// ---------------------------------------------------------------------------------------------
struct LossW { float w[LLMREC_BPR_MAX_PROBLEMS]; };
constexpr int LA_SLOTS = 1024;                                          // the tree's slots (bpr_reduce_kernel's block size)
constexpr int LA_TREES = 4 * LLMREC_BPR_MAX_PROBLEMS + 1;
__device__ __forceinline__ float wave_tree_sum_1024(const float* __restrict__ src, int n, int lane) {
    float r[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) r[j] = 0.f;
    for (int base = 0; base < n; base += LA_SLOTS) {                    // wavefront-uniform; a round's 16 loads are issued together
        float x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) { const int b = base + lane + 64 * j; x[j] = b < n ? src[b] : 0.f; }
#pragma unroll
        for (int j = 0; j < 16; ++j) { const int b = base + lane + 64 * j; if (b < n) r[j] += x[j]; }   // (ascending b per slot, from 0.f)
    }
#pragma unroll
    for (int h = 8; h > 0; h >>= 1) {
#pragma unroll
        for (int j = 0; j < h; ++j) r[j] += r[j + h];
    }
    float x = r[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

struct LossesArgs {
    int n_prob, B_max;
    const int32_t* n_valid_dev;
    double remember_rate;
    float decay, bsz;
    float* out_all;
    float* saved_all;
    int saved_stride;
    LossW w;
    const float* partial;
    int n_partial;
    float reg_coef;
    float* scal;
    double* running;
};

template <int NT>
__device__ __forceinline__ void guest_block(const LossesArgs& a, int, char*) {
    __shared__ float tot_s[LA_TREES];                                   // [4 prob + col]: kept, Su, Sp, Sq; [4 n_prob]: the partials' sum
    const int n_prob = a.n_prob, B_max = a.B_max;
    const float* __restrict__ partial = a.partial;
    float* __restrict__ saved_all = a.saved_all;
    const int B = bpr_batch(a.n_valid_dev, B_max);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n_trees = 4 * n_prob + (partial ? 1 : 0);
    for (int tr = wv; tr < n_trees; tr += NT / 64) {                    // wavefront-uniform
        const int tree = partial ? (tr == 0 ? 4 * n_prob : tr - 1) : tr;   // the partials' tree (the longest) is dealt first
        float x;
        if (tree == 4 * n_prob) {
            x = wave_tree_sum_1024(partial, a.n_partial, lane);
        } else {
            const int prob = tree >> 2, col = tree & 3;                   // slots 1 (kept m_b), 2, 3, 4 (squared norms) of `saved`
            x = wave_tree_sum_1024(saved_all + (int64_t)prob * a.saved_stride + B_max + 4 + (int64_t)(col + 1) * B_max, B, lane);
        }
        if (lane == 0) tot_s[tree] = x;
    }
    __syncthreads();                                                    // the one barrier: every tree's total is in LDS
    if (wv != 0) return;
    float mf = 0.f, emb = 0.f;
    if (lane < n_prob) {
        const int prob = lane;
        float* saved = saved_all + (int64_t)prob * a.saved_stride;
        float tot[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) tot[c] = tot_s[4 * prob + c];
        const int k = (int)(a.remember_rate * (double)B);
        mf = -(tot[0] / (float)k);                                       // k == 0 -> nan, as torch's empty mean
        const float reg = 1.0f / (2.0f * tot[1] + 1e-8f) + 1.0f / (2.0f * tot[2] + 1e-8f) + 1.0f / (2.0f * tot[3] + 1e-8f);
        emb = a.decay * (reg / a.bsz);
        a.out_all[prob * 2 + 0] = mf; a.out_all[prob * 2 + 1] = emb;
        saved[B_max + 0] = tot[1]; saved[B_max + 1] = tot[2]; saved[B_max + 2] = tot[3]; saved[B_max + 3] = (float)k;
    }
    float outs[LLMREC_BPR_MAX_PROBLEMS][2];
#pragma unroll
    for (int p = 0; p < LLMREC_BPR_MAX_PROBLEMS; ++p) { outs[p][0] = __shfl(mf, p, 64); outs[p][1] = __shfl(emb, p, 64); }
    if (lane != 0 || !a.scal) return;                                   // (no scal: the loss values only, llmrec_bpr_multi_losses_wide_f32)
    float* scal = a.scal;
    float feat = scal[0];                                              // no partial sums: whatever llmrec_sumsq_f32 left there
    if (partial) feat = a.reg_coef * tot_s[4 * n_prob];
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < LLMREC_BPR_MAX_PROBLEMS; ++p) if (p < n_prob) s += outs[p][0] * a.w.w[p];
    scal[0] = feat;
    scal[2] = outs[0][0]; scal[3] = outs[0][1];
    scal[1] = s + outs[0][1] + feat;
    if (a.running) { a.running[0] += (double)scal[1]; a.running[1] += (double)scal[2]; a.running[2] += (double)scal[3]; }
}

// The checks of llmrec_bpr_multi_losses_assemble_f32: one block, whatever its size.
static inline int guest_prepare(const llmrec_guest_losses_t& g, int, const char* who, LossesArgs& a, int64_t& blocks, size_t& shmem) {
    LLMREC_CHECK_ARG(g.n_problems >= 1 && g.n_problems <= LLMREC_BPR_MAX_PROBLEMS && g.B_max >= 0 && g.out && g.saved && g.w_mf_host && g.scal4,
                     "%s: bad argument", who);
    LLMREC_CHECK_ARG(g.n_partial >= 0 && (g.n_partial == 0 || g.sumsq_partial), "%s: partial sums without a buffer", who);
    if (g.B_max > LLMREC_BPR_MAX_B) { set_error("%s: B_max %d > %d", who, g.B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LossW w = {};
    for (int i = 0; i < g.n_problems; ++i) w.w[i] = g.w_mf_host[i];
    blocks = 1; shmem = 0;
    a = LossesArgs{g.n_problems, g.B_max, g.n_valid_dev, g.remember_rate, g.decay, g.batch_size_flag, g.out, g.saved,
                   (int)LLMREC_BPR_SAVED_FLOATS(g.B_max), w, g.n_partial > 0 ? g.sumsq_partial : nullptr, g.n_partial, g.feat_reg_coef, g.scal4,
                   g.running_sums3};
    return LLMREC_OK;
}

}  // namespace llmrec
