// bpr.hip - R7 fused BPR + prune loss (forward and backward) and R11 the on-device sampler.
// Replaces the three gathers, mul/sum, logsigmoid, the D2H argsort of prune_loss and autograd's
// index_put backward (reference main.py:158-165,232-254,330-342), and Data.sample
// (utility/load_data.py:157-195). One launch, no host synchronisation: the reference pays a
// device->host->device round trip per bpr_loss call (8 per step, main.py:159).
#include "common.h"
#include "guests.h"
#include <hipcub/hipcub.hpp>

namespace llmrec {

constexpr int BPR_THREADS = 1024;

__device__ __forceinline__ float logsigmoid_f(float x) {
    // min(x, 0) - log1p(exp(-|x|)), the form aten::log_sigmoid_forward uses
    return fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
}

// ---------------------------------------------------------------------------------------------
// Forward = three launches over up to LLMREC_BPR_MAX_PROBLEMS (user table, item table) pairs that
// share one (users, pos, neg) batch - the reference evaluates 8 such losses per step
// (main.py:232-254):
//   bpr_scores_kernel  one 16-lane group per (problem, sample): the three row gathers, both dot
//                      products, log-sigmoid, its derivative and the three squared row norms;
//   bpr_rank_kernel    one thread per (problem, sample): rank counting against the B log-sigmoids
//                      staged in LDS (keep the k smallest, ties by lower index);
//   bpr_reduce_kernel  one block per problem: the kept mean and the norm sums by fixed-order
//                      trees (deterministic).
// saved layout per problem (LLMREC_BPR_SAVED_FLOATS(B) floats):
//   [0, B) d(mf)/d(s_b) | [B..B+2] Su, Sp, Sq | [B+3] k | [B+4 + {0..4} * B + b] m, sg, nu, np, nq
// ---------------------------------------------------------------------------------------------
struct BprTables {
    const float* Eu[LLMREC_BPR_MAX_PROBLEMS];
    const float* Ei[LLMREC_BPR_MAX_PROBLEMS];
    int64_t ldu[LLMREC_BPR_MAX_PROBLEMS];
    int64_t ldi[LLMREC_BPR_MAX_PROBLEMS];
    float* dEu[LLMREC_BPR_MAX_PROBLEMS];
    float* dEi[LLMREC_BPR_MAX_PROBLEMS];
    int64_t lddu[LLMREC_BPR_MAX_PROBLEMS];
    int64_t lddi[LLMREC_BPR_MAX_PROBLEMS];
    float g_mf[LLMREC_BPR_MAX_PROBLEMS];
    float g_emb[LLMREC_BPR_MAX_PROBLEMS];
};

// what "a new step begins" means on the device (one thread of the scores launch): a new row stamp and, when given, AdamW's step
// counter / bias corrections (adamw_advance_kernel's arithmetic, rowops.hip)
struct StepBegin {
    int32_t* row_stamp;
    float* adamw_state;
    float lr, b1, b2;
};

__global__ __launch_bounds__(256) void bpr_scores_kernel(BprTables t, int d, const int64_t* __restrict__ users,
                                                         const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                                         int B_max, const int32_t* __restrict__ n_valid_dev,
                                                         float* __restrict__ saved_all, int saved_stride, StepBegin sb) {
    const int B = bpr_batch(n_valid_dev, B_max);
    const int prob = blockIdx.y;
    const int gl = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (sb.row_stamp) sb.row_stamp[0] = (int32_t)((uint32_t)sb.row_stamp[0] + 1u);   // a new step: new stamp
        if (sb.adamw_state) {
            const int tt = __float_as_int(sb.adamw_state[0]) + 1;
            sb.adamw_state[0] = __int_as_float(tt);
            const double bc1 = 1.0 - pow((double)sb.b1, (double)tt);
            const double bc2 = 1.0 - pow((double)sb.b2, (double)tt);
            sb.adamw_state[1] = (float)((double)sb.lr / bc1);
            sb.adamw_state[2] = (float)sqrt(bc2);
        }
    }
    if (b >= B) return;
    float* sc = saved_all + (int64_t)prob * saved_stride + B_max + 4;
    const float* u = t.Eu[prob] + users[b] * t.ldu[prob];
    const float* p = t.Ei[prob] + pos[b] * t.ldi[prob];
    const float* q = t.Ei[prob] + neg[b] * t.ldi[prob];
    float dp = 0.f, dn = 0.f, nu = 0.f, np_ = 0.f, nq = 0.f;
    for (int c = gl; c < d; c += 16) {
        const float uu = u[c], pp = p[c], qq = q[c];
        dp = fmaf(uu, pp, dp); dn = fmaf(uu, qq, dn);
        nu = fmaf(uu, uu, nu); np_ = fmaf(pp, pp, np_); nq = fmaf(qq, qq, nq);
    }
    dp = group_sum<16>(dp); dn = group_sum<16>(dn);
    nu = group_sum<16>(nu); np_ = group_sum<16>(np_); nq = group_sum<16>(nq);
    if (gl == 0) {
        const float x = (dp - dn) + 1e-8f;
        sc[b] = logsigmoid_f(x);
        sc[B_max + b] = 1.0f / (1.0f + expf(x));                      // sigmoid(-x) = d logsigmoid / dx
        sc[2 * B_max + b] = nu; sc[3 * B_max + b] = np_; sc[4 * B_max + b] = nq;
    }
}

__device__ __forceinline__ float block_tree_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = BPR_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// Batch-sharded selection (data-parallel or user-sharded ranks): every rank all-gathers one block of
// LLMREC_BPR_GATHER_FLOATS(P, cap) floats, laid out  [P][cap] m_b | [P][4] Su, Sp, Sq, k | n_valid (as float);
// the global batch is the concatenation of the ranks' valid samples in rank order.
struct BprGather {
    const float* g;        // null: the batch is local
    int n_ranks;           // blocks in g
    int64_t stride;        // floats between two ranks' blocks
    int cap;               // sample capacity per rank (= that rank's B_max)
    int n_prob;            // problems per block (P)
    int my_offset;         // global padded index of this rank's sample 0 (= my_rank * cap)
    int has_tail;          // 0: g is a plain [n_ranks * cap] array of m_b, all valid (single-problem API)
};

__device__ __forceinline__ int gather_valid(const BprGather& ga, int r) {
    if (!ga.has_tail) return ga.cap;
    const int nv = (int)ga.g[r * ga.stride + (int64_t)ga.n_prob * ga.cap + 4 * ga.n_prob];
    return nv > ga.cap ? ga.cap : (nv < 0 ? 0 : nv);
}

__device__ __forceinline__ int gather_batch(const BprGather& ga) {
    int n = 0;
    for (int r = 0; r < ga.n_ranks; ++r) n += gather_valid(ga, r);
    return n;
}

// selection, step 1: rank counting. grid = (ceil(B / 16), problems); each 16-lane group ranks one sample
// against the Bg log-sigmoids staged in LDS and writes d(mf)/d(s_b) (0 when dropped) plus the kept
// m_b into the scratch (slot 1 = sg is consumed here and overwritten with the kept value).
// Padding slots of the gathered layout are staged as +inf: they never precede a real sample.
__global__ __launch_bounds__(256) void bpr_rank_kernel(int B_max, const int32_t* __restrict__ n_valid_dev, double remember_rate,
                                                       float* __restrict__ saved_all, int saved_stride, BprGather ga) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* m_s = reinterpret_cast<float*>(smem);
    const int B = bpr_batch(n_valid_dev, B_max);
    const int prob = blockIdx.y;
    float* saved = saved_all + (int64_t)prob * saved_stride;
    float* sc = saved + B_max + 4;
    int Bg, slots;
    if (ga.g) {
        slots = ga.n_ranks * ga.cap;
        Bg = gather_batch(ga);
        for (int r = 0; r < ga.n_ranks; ++r) {
            const int nv = gather_valid(ga, r);
            const float* src = ga.g + r * ga.stride + (int64_t)prob * ga.cap;
            for (int j = threadIdx.x; j < ga.cap; j += 256) m_s[r * ga.cap + j] = j < nv ? src[j] : __builtin_inff();
        }
    } else {
        slots = Bg = B;
        for (int j = threadIdx.x; j < B; j += 256) m_s[j] = sc[j];
    }
    __syncthreads();
    const int k = (int)(remember_rate * (double)Bg);                   // int((1 - drop) * len) of main.py:161-162
    // one 16-lane group per sample: the lanes split the comparison loop (integer counts: order-independent)
    const int gl = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B_max) return;
    if (b >= B) { if (gl == 0) { saved[b] = 0.f; sc[B_max + b] = 0.f; } return; }
    const float mb = sc[b];
    bool keep = true;
    if (k < Bg) {
        int rank = 0;
        const int me = ga.my_offset + b;
        for (int j = gl; j < slots; j += 16) {
            const float mj = m_s[j];
            rank += (mj < mb) || (mj == mb && j < me);
        }
        rank = (int)group_sum<16>((float)rank);                           // < 2^24: exact
        keep = rank < k;
    }
    if (gl == 0) {
        saved[b] = keep ? (-1.0f / (float)k) * sc[B_max + b] : 0.f;
        sc[B_max + b] = keep ? mb : 0.f;
    }
}

// selection, step 2: one block per problem sums the kept log-sigmoids and the three squared norms
// with fixed-order trees (deterministic) and writes the two loss values. With a gathered layout the
// norms (and the batch size) are the sums over the ranks' blocks in rank order - identical on every
// rank - while out[0] stays this rank's share of mf.
__device__ __forceinline__ void bpr_reduce_problem(int prob, int B_max, const int32_t* __restrict__ n_valid_dev,
                                                   double remember_rate, float decay, float bsz,
                                                   float* __restrict__ out_all, float* __restrict__ saved_all,
                                                   int saved_stride, const BprGather& ga, float* red) {
    const int B = bpr_batch(n_valid_dev, B_max);
    float* saved = saved_all + (int64_t)prob * saved_stride;
    const float* sc = saved + B_max + 4;
    const int Bg = ga.g ? gather_batch(ga) : B;
    const int k = (int)(remember_rate * (double)Bg);
    float part = 0.f, su = 0.f, sp = 0.f, sq = 0.f;
    for (int b = threadIdx.x; b < B; b += BPR_THREADS) {
        part += sc[B_max + b];
        su += sc[2 * B_max + b]; sp += sc[3 * B_max + b]; sq += sc[4 * B_max + b];
    }
    const float kept = block_tree_sum(part, red);
    float Su = block_tree_sum(su, red), Sp = block_tree_sum(sp, red), Sq = block_tree_sum(sq, red);
    if (threadIdx.x == 0) {
        if (ga.g && ga.has_tail) {
            Su = Sp = Sq = 0.f;
            for (int r = 0; r < ga.n_ranks; ++r) {
                const float* nb = ga.g + r * ga.stride + (int64_t)ga.n_prob * ga.cap + 4 * prob;
                Su += nb[0]; Sp += nb[1]; Sq += nb[2];
            }
        }
        out_all[prob * 2 + 0] = -(kept / (float)k);                    // k == 0 -> nan, as torch's empty mean
        const float reg = 1.0f / (2.0f * Su + 1e-8f) + 1.0f / (2.0f * Sp + 1e-8f) + 1.0f / (2.0f * Sq + 1e-8f);
        out_all[prob * 2 + 1] = decay * (reg / bsz);
        saved[B_max + 0] = Su; saved[B_max + 1] = Sp; saved[B_max + 2] = Sq; saved[B_max + 3] = (float)k;
    }
}

__global__ __launch_bounds__(BPR_THREADS) void bpr_reduce_kernel(int B_max, const int32_t* __restrict__ n_valid_dev,
                                                                 double remember_rate, float decay, float bsz,
                                                                 float* __restrict__ out_all, float* __restrict__ saved_all,
                                                                 int saved_stride, BprGather ga) {
    __shared__ float red[BPR_THREADS];
    bpr_reduce_problem(blockIdx.x, B_max, n_valid_dev, remember_rate, decay, bsz, out_all, saved_all, saved_stride, ga, red);
}

// The logged scalars of a fused step in ONE single-block launch (llmrec_bpr_multi_losses_assemble_f32): guests.h's body, its
// 4 n_prob + 1 trees dealt to the block's 16 wavefronts.
__global__ __launch_bounds__(BPR_THREADS) void bpr_losses_assemble_kernel(LossesArgs a) {
    guest_block<BPR_THREADS>(a, 0, nullptr);
}

// pass 1 of the batch-sharded forward: this rank's block of the gathered layout
__global__ __launch_bounds__(256) void bpr_pack_kernel(int n_prob, int B_max, const int32_t* __restrict__ n_valid_dev,
                                                       const float* __restrict__ saved_all, int saved_stride, float* __restrict__ block) {
    const int B = bpr_batch(n_valid_dev, B_max);
    const int total = n_prob * B_max + 4 * n_prob + 1;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        float v;
        if (i < n_prob * B_max) {
            const int p = i / B_max, b = i - p * B_max;
            v = b < B ? saved_all[(int64_t)p * saved_stride + B_max + 4 + b] : __builtin_inff();
        } else if (i < n_prob * B_max + 4 * n_prob) {
            const int j = i - n_prob * B_max;
            v = saved_all[(int64_t)(j >> 2) * saved_stride + B_max + (j & 3)];
        } else {
            v = (float)B;
        }
        block[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// DETERMINISTIC gradient scatter (round 6). The reference's backward is index_put(accumulate) on CPU: given the seed it adds the
// rows several samples share in one fixed order (main.py:232-254,330-342), and same-seed runs agree. Rounds 1 - 5 added the rows
// with fp32 atomicAdd, so two runs of one seed drifted apart (1.0e-3 vs 3.6e-3 in the final E_i of one trajectory on two boxes).
// Now every destination row has ONE owner that adds the row's contributions in a fixed order, without atomics:
//   bpr_plan_kernel      depends on (users, pos, neg, n_valid) only - the fused step runs it right behind the sampler, off the
//                        critical path. Keys  id << 32 | slot  (distinct), sorted by RANK COUNTING: every block stages its side's keys in
//                        LDS, each 16-lane group counts the keys below its own -> the key's sorted position (no serial sorting network:
//                        one round of LDS reads, ceil(3 B / 16) blocks):
//                          plan[0 .. B_max)          user side, slot b          (id = users[b])
//                          plan[B_max .. 3 B_max)    item side, slot b          (id = pos[b])  /  B_max + b  (id = neg[b])
//                        slots of samples b >= n_valid carry the id 0xffffffff and sort to the end. Behind the keys, as int32:
//                          runlen[3 B_max]           at a run's first position: the number of keys with that id; 0 elsewhere (and for id 0xffffffff)
//   bpr_bwd_runs_kernel  one 16-lane group per sorted position and problem; the HEAD of a run of equal ids owns the destination row
//                        and adds, in ascending problem index (problems whose target POINTER is the same - the five attribute problems
//                        of a step share d prof_u - are summed by the first of them) and ascending slot, what rounds 1 - 5
//                        added with atomics; a dropped sample (coefficient 0) of a problem without a regulariser share is skipped, its
//                        contribution being exactly zero. The (problem, member) pairs of a run are taken 16 at a time: lane l fetches
//                        pair l's slot, coefficient and row ids (ONE round of dependent loads for 16 pairs), the pairs that contribute are
//                        compacted into LDS records, and the group then streams the records' rows four at a time.
// Targets of different problems must be identical (same pointer, same leading dimension) or disjoint.
// ---------------------------------------------------------------------------------------------
// (bpr_plan_block and the plan + reach-mark body: guests.h)
__global__ __launch_bounds__(256) void bpr_plan_kernel(const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                                       const int64_t* __restrict__ neg, int B_max,
                                                       const int32_t* __restrict__ n_valid_dev, uint64_t* __restrict__ plan) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bpr_plan_block<256>((int)blockIdx.x, reinterpret_cast<uint64_t*>(smem), users, pos, neg, B_max, n_valid_dev, plan);
}

// The scatter plan and the reach flags of one batch in ONE launch (llmrec_bpr_scatter_plan_reach_mark): blocks [0, plan_blocks) run
// the plan's body, the blocks behind them llmrec_batch_reach_rows' marking body (reach.h). Both read the sampled batch only and
// neither reads what the other writes, so the flags no longer cost a launch of their own on the step's one stream.
__global__ __launch_bounds__(256) void bpr_plan_reach_mark_kernel(PlanReachArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    guest_block<256>(a, (int)blockIdx.x, smem);
}

constexpr int RUN_MAX_SHARE = LLMREC_BPR_MAX_PROBLEMS;
struct RunShare {                                                      // the problems that scatter into this block's target (LDS)
    const float* Eu[RUN_MAX_SHARE]; const float* Ei[RUN_MAX_SHARE]; const float* saved[RUN_MAX_SHARE];
    int64_t ldu[RUN_MAX_SHARE], ldi[RUN_MAX_SHARE];
    float g_mf[RUN_MAX_SHARE], cu[RUN_MAX_SHARE], cp[RUN_MAX_SHARE], cq[RUN_MAX_SHARE];
    int n, any_reg;
};
struct RunRec { const float* a; const float* b; const float* self; float ds, cr; };   // user row: ds (a - b) + cr self ; item row: ds a + cr self

template <int NV, bool VEC> struct RunAcc;
template <int NV> struct RunAcc<NV, true> {                            // lane gl: float4 chunks gl, gl + 16, ... of a 64 NV-column pass
    float4 v[NV];
    __device__ __forceinline__ void load(const float* row, int c0, int d, int gl) {
#pragma unroll
        for (int i = 0; i < NV; ++i) { const int c = c0 + 4 * (gl + 16 * i); v[i] = c < d ? *reinterpret_cast<const float4*>(row + c) : float4{0.f, 0.f, 0.f, 0.f}; }
    }
    __device__ __forceinline__ void store(float* row, int c0, int d, int gl) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) { const int c = c0 + 4 * (gl + 16 * i); if (c < d) *reinterpret_cast<float4*>(row + c) = v[i]; }
    }
};
template <int NV> struct RunAcc<NV, false> {                           // lane gl: columns gl, gl + 16, ... of a 64 NV-column pass
    float v[4 * NV];
    __device__ __forceinline__ void load(const float* row, int c0, int d, int gl) {
#pragma unroll
        for (int i = 0; i < 4 * NV; ++i) { const int c = c0 + gl + 16 * i; v[i] = c < d ? row[c] : 0.f; }
    }
    __device__ __forceinline__ void store(float* row, int c0, int d, int gl) const {
#pragma unroll
        for (int i = 0; i < 4 * NV; ++i) { const int c = c0 + gl + 16 * i; if (c < d) row[c] = v[i]; }
    }
};
template <int NV, bool VEC, bool ITEM, bool REG>
__device__ __forceinline__ void run_add(RunAcc<NV, VEC>& acc, const RunAcc<NV, VEC>& a, const RunAcc<NV, VEC>& b, const RunAcc<NV, VEC>& self,
                                        float ds, float cr) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float4 x = a.v[i], y = ITEM ? float4{0.f, 0.f, 0.f, 0.f} : b.v[i], z = REG ? self.v[i] : float4{0.f, 0.f, 0.f, 0.f};
            acc.v[i].x += fmaf(ds, ITEM ? x.x : x.x - y.x, cr * z.x); acc.v[i].y += fmaf(ds, ITEM ? x.y : x.y - y.y, cr * z.y);
            acc.v[i].z += fmaf(ds, ITEM ? x.z : x.z - y.z, cr * z.z); acc.v[i].w += fmaf(ds, ITEM ? x.w : x.w - y.w, cr * z.w);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4 * NV; ++i)
            acc.v[i] += fmaf(ds, ITEM ? a.v[i] : a.v[i] - b.v[i], cr * (REG ? self.v[i] : 0.f));
    }
}

// the records [0, n) of one group, four at a time (their row loads are independent: up to 12 rows in flight per group)
template <int NV, bool VEC, bool ITEM, bool REG>
__device__ __forceinline__ void run_stream(RunAcc<NV, VEC>& acc, const RunRec* __restrict__ recs, int n, int c0, int d, int gl) {
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        RunAcc<NV, VEC> a[4], b[4], z[4];
        float ds[4], cr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const RunRec r = recs[i + u];
            ds[u] = r.ds; cr[u] = r.cr;
            a[u].load(r.a, c0, d, gl);
            if (!ITEM) b[u].load(r.b, c0, d, gl);
            if (REG) z[u].load(r.self, c0, d, gl);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) run_add<NV, VEC, ITEM, REG>(acc, a[u], b[u], z[u], ds[u], cr[u]);
    }
    for (; i < n; ++i) {
        const RunRec r = recs[i];
        RunAcc<NV, VEC> a, b, z;
        a.load(r.a, c0, d, gl);
        if (!ITEM) b.load(r.b, c0, d, gl);
        if (REG) z.load(r.self, c0, d, gl);
        run_add<NV, VEC, ITEM, REG>(acc, a, b, z, r.ds, r.cr);
    }
}

// grid = (ceil(B_max / 16) + ceil(2 B_max / 16), problems): a block works on ONE side (its 16 positions are all user-side or all item-side)
template <bool VEC, int NV>                                             // NV: 64-column units per pass (1 when d <= 64)
__global__ __launch_bounds__(256) void bpr_bwd_runs_kernel(BprTables t, int n_prob, int d, const int64_t* __restrict__ users,
                                                           const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                                           int B_max, float decay, float bsz, const float* __restrict__ saved_all,
                                                           int saved_stride, const uint64_t* __restrict__ plan,
                                                           const float* __restrict__ grads2_dev) {
    __shared__ RunShare sh;
    __shared__ RunRec recs_s[16][16];
    const int prob = blockIdx.y;
    const int nbu = (B_max + 15) / 16;
    const bool item = (int)blockIdx.x >= nbu;
    float* const dst0 = item ? t.dEi[prob] : t.dEu[prob];
    for (int q = 0; q < prob; ++q)
        if ((item ? t.dEi[q] : t.dEu[q]) == dst0) return;             // an earlier problem owns this target (and sums this one's share): block-uniform
    if (threadIdx.x == 0) {
        int n = 0, any_reg = 0;
        for (int pp = prob; pp < n_prob; ++pp) {
            if ((item ? t.dEi[pp] : t.dEu[pp]) != dst0) continue;
            const float* saved = saved_all + (int64_t)pp * saved_stride;
            const float g_emb = grads2_dev ? grads2_dev[1] : t.g_emb[pp];
            // d emb / d X = decay / bsz * (-1 / (2 S + 1e-8)^2) * 4 X
            const float base = -4.0f * decay / bsz * g_emb;
            const float du_ = 2.0f * saved[B_max] + 1e-8f, dp_ = 2.0f * saved[B_max + 1] + 1e-8f, dq_ = 2.0f * saved[B_max + 2] + 1e-8f;
            sh.Eu[n] = t.Eu[pp]; sh.Ei[n] = t.Ei[pp]; sh.saved[n] = saved; sh.ldu[n] = t.ldu[pp]; sh.ldi[n] = t.ldi[pp];
            sh.g_mf[n] = grads2_dev ? grads2_dev[0] : t.g_mf[pp];
            sh.cu[n] = base / (du_ * du_); sh.cp[n] = base / (dp_ * dp_); sh.cq[n] = base / (dq_ * dq_);
            any_reg |= base != 0.f;
            ++n;
        }
        sh.n = n; sh.any_reg = any_reg;
    }
    __syncthreads();
    const int gl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int side_n = item ? 2 * B_max : B_max, side_base = item ? B_max : 0;
    const int j0 = ((int)blockIdx.x - (item ? nbu : 0)) * 16 + grp;   // position within the side
    if (j0 >= side_n) return;
    const int32_t* runlen = reinterpret_cast<const int32_t*>(plan + 3 * (int64_t)B_max);
    const int len = runlen[side_base + j0];
    if (len <= 0) return;                                              // not the head of a run (or the run of the unused slots)
    const uint64_t* keys = plan + side_base + j0;
    const uint32_t id = (uint32_t)(keys[0] >> 32);
    float* const out = dst0 + (int64_t)id * (item ? t.lddi[prob] : t.lddu[prob]);
    const int total = sh.n * len;
    const bool reg = sh.any_reg != 0;
    RunRec* recs = recs_s[grp];
    const int shift = 16 * (grp & 3);                                  // this group's 16 bits of the wave's ballot
    for (int c0 = 0; c0 < d; c0 += 64 * NV) {
        RunAcc<NV, VEC> acc;
        acc.load(out, c0, d, gl);
        for (int t0 = 0; t0 < total; t0 += 16) {
            const int tt = t0 + gl;
            bool act = false;
            RunRec r = {};
            if (tt < total) {
                const int s_ = tt / len, m_ = tt - s_ * len;
                const uint32_t slot = (uint32_t)keys[m_];
                const bool is_neg = slot >= (uint32_t)B_max;
                const int b = (int)(is_neg ? slot - (uint32_t)B_max : slot);
                const float ds = sh.g_mf[s_] * sh.saved[s_][b];
                if (item) {                                                // d/dEi[p_b] = ds u + cp p ; d/dEi[q_b] = -ds u + cq q
                    r.ds = is_neg ? -ds : ds; r.cr = is_neg ? sh.cq[s_] : sh.cp[s_];
                    act = !(ds == 0.f && r.cr == 0.f);
                    if (act) { r.a = sh.Eu[s_] + users[b] * sh.ldu[s_]; r.b = r.a; r.self = sh.Ei[s_] + (int64_t)id * sh.ldi[s_]; }
                } else {                                                   // d/dEu[u_b] = ds (p - q) + cu u
                    r.ds = ds; r.cr = sh.cu[s_];
                    act = !(ds == 0.f && r.cr == 0.f);
                    if (act) { r.a = sh.Ei[s_] + pos[b] * sh.ldi[s_]; r.b = sh.Ei[s_] + neg[b] * sh.ldi[s_]; r.self = sh.Eu[s_] + (int64_t)id * sh.ldu[s_]; }
                }
            }
            const uint32_t bits = (uint32_t)(__ballot(act) >> shift) & 0xffffu;
            const int n_act = __popc(bits);
            if (act) recs[__popc(bits & ((1u << gl) - 1u))] = r;
            __builtin_amdgcn_wave_barrier();                           // (one wave: its LDS writes and reads execute in order)
            if (item) {
                if (reg) run_stream<NV, VEC, true, true>(acc, recs, n_act, c0, d, gl);
                else run_stream<NV, VEC, true, false>(acc, recs, n_act, c0, d, gl);
            } else {
                if (reg) run_stream<NV, VEC, false, true>(acc, recs, n_act, c0, d, gl);
                else run_stream<NV, VEC, false, false>(acc, recs, n_act, c0, d, gl);
            }
            __builtin_amdgcn_wave_barrier();
        }
        acc.store(out, c0, d, gl);
    }
}

// the norm block of a selection launch (256 threads): thread t of bpr_reduce_kernel's 1024 is emulated by the four slots t, t + 256, ... of
// this block's threads, then the same pairwise tree over 1024 LDS slots, three columns at once -> saved[B_max .. B_max + 2]; k -> [B_max + 3]
__device__ __forceinline__ void sel_norm_block(float* __restrict__ saved, int B, int B_max, int k, float (*red)[BPR_THREADS]) {
    const float* sc = saved + B_max + 4;
    for (int v = threadIdx.x; v < BPR_THREADS; v += 256) {        // the partial sums of bpr_reduce_kernel's thread v
        float su = 0.f, sp = 0.f, sq = 0.f;
        for (int b = v; b < B; b += BPR_THREADS) { su += sc[2 * B_max + b]; sp += sc[3 * B_max + b]; sq += sc[4 * B_max + b]; }
        red[0][v] = su; red[1][v] = sp; red[2][v] = sq;
    }
    __syncthreads();
    for (int off = BPR_THREADS / 2; off > 0; off >>= 1) {         // block_tree_sum's tree, three columns at once
        for (int i = threadIdx.x; i < off; i += 256) {
            red[0][i] += red[0][i + off]; red[1][i] += red[1][i + off]; red[2][i] += red[2][i + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) saved[B_max + threadIdx.x] = red[threadIdx.x][0];
    if (threadIdx.x == 3) saved[B_max + 3] = (float)k;
}

// selection of a LOCAL batch (first launch of llmrec_bpr_multi_select_bwd_f32): grid = (ceil(B_max / 16) + 1, problems).
// Blocks [0, ceil(B_max / 16)): stage the batch's log-sigmoids in LDS and rank their 16 samples as bpr_rank_kernel does (kept
// coefficient -> saved[b], kept value -> slot 1), stamp the rows the batch touches. The LAST block of a problem sums the three
// squared-norm columns with the summation tree of bpr_reduce_kernel - thread t of that 1024-thread launch is emulated by the four
// slots t, t + 256, ... of this block's threads, then the same pairwise tree over 1024 LDS slots - so saved[B_max .. B_max + 2] carry
// the bits the loss launch writes later (the backward launch reads them).
__global__ __launch_bounds__(256) void bpr_select_kernel(const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                                         const int64_t* __restrict__ neg, int B_max,
                                                         const int32_t* __restrict__ n_valid_dev, double remember_rate,
                                                         float* __restrict__ saved_all, int saved_stride,
                                                         uint8_t* __restrict__ flag_u, uint8_t* __restrict__ flag_i,
                                                         const int32_t* __restrict__ row_stamp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* m_s = reinterpret_cast<float*>(smem);                      // [B] (rank blocks) / [3][1024] (the norm block)
    const int B = bpr_batch(n_valid_dev, B_max);
    const int prob = blockIdx.y;
    float* saved = saved_all + (int64_t)prob * saved_stride;
    float* sc = saved + B_max + 4;
    const int k = (int)(remember_rate * (double)B);
    if (blockIdx.x == gridDim.x - 1) {
        sel_norm_block(saved, B, B_max, k, reinterpret_cast<float (*)[BPR_THREADS]>(smem));
        return;
    }
    for (int j = threadIdx.x; j < B; j += 256) m_s[j] = sc[j];
    __syncthreads();
    const int gl = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B_max) return;
    if (b >= B) { if (gl == 0) { saved[b] = 0.f; sc[B_max + b] = 0.f; } return; }
    const float mb = m_s[b];
    bool keep = true;
    if (k < B) {
        int rank = 0;
        for (int j = gl; j < B; j += 16) {
            const float mj = m_s[j];
            rank += (mj < mb) || (mj == mb && j < b);
        }
        rank = (int)group_sum<16>((float)rank);                           // < 2^24: exact
        keep = rank < k;
    }
    const float coef = keep ? (-1.0f / (float)k) * sc[B_max + b] : 0.f;   // every lane of the group reads slot 1 before lane 0 rewrites it
    __builtin_amdgcn_wave_barrier();
    if (gl == 0) {
        saved[b] = coef; sc[B_max + b] = keep ? mb : 0.f;
        if (prob == 0) {                                              // rows this batch touches (same rows for every problem)
            const uint8_t stamp = row_stamp ? LLMREC_ROW_STAMP(row_stamp[0]) : (uint8_t)1;
            if (flag_u) flag_u[users[b]] = stamp;
            if (flag_i) { flag_i[pos[b]] = stamp; flag_i[neg[b]] = stamp; }
        }
    }
}

// the rows the loss backward added into are cleared again (one lane group per sample): the scatter targets stay all-zero between steps
// without a dense memset
__global__ __launch_bounds__(256) void bpr_zero_rows_kernel(BprTables t, int d, const int64_t* __restrict__ users,
                                                            const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                                            int B_max, const int32_t* __restrict__ n_valid_dev) {
    const int B = bpr_batch(n_valid_dev, B_max);
    const int prob = blockIdx.y;
    const int gl = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B) return;
    float* du = t.dEu[prob] + users[b] * t.lddu[prob];
    float* dpp = t.dEi[prob] + pos[b] * t.lddi[prob];
    float* dqq = t.dEi[prob] + neg[b] * t.lddi[prob];
    for (int c = gl; c < d; c += 16) { du[c] = 0.f; dpp[c] = 0.f; dqq[c] = 0.f; }
}

// the same gradient as compact rows (row-sharded step): rows3[0][b] = d/dEu[u_b], rows3[1][b] = d/dEi[p_b], rows3[2][b] = d/dEi[q_b]
__global__ __launch_bounds__(256) void bpr_bwd_rows_kernel(const float* __restrict__ Eu, int64_t ldu,
                                                           const float* __restrict__ Ei, int64_t ldi, int d,
                                                           const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                                           const int64_t* __restrict__ neg, int B_max,
                                                           const int32_t* __restrict__ n_valid_dev, float decay, float bsz,
                                                           const float* __restrict__ saved, const float* __restrict__ grads2,
                                                           float* __restrict__ rows3) {
    int B = n_valid_dev ? n_valid_dev[0] : B_max;
    if (B > B_max) B = B_max;
    const float g_mf = grads2[0], g_emb = grads2[1];
    const float Su = saved[B_max], Sp = saved[B_max + 1], Sq = saved[B_max + 2];
    const float base = -4.0f * decay / bsz * g_emb;
    const float du_ = 2.0f * Su + 1e-8f, dp_ = 2.0f * Sp + 1e-8f, dq_ = 2.0f * Sq + 1e-8f;
    const float cu = base / (du_ * du_), cp = base / (dp_ * dp_), cq = base / (dq_ * dq_);
    const int gl = threadIdx.x & 15;
    const int groups = gridDim.x * (blockDim.x >> 4);
    const int64_t plane = (int64_t)B_max * d;
    for (int b = blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4); b < B_max; b += groups) {
        float* ru = rows3 + (int64_t)b * d;
        if (b >= B) {
            for (int c = gl; c < d; c += 16) { ru[c] = 0.f; ru[plane + c] = 0.f; ru[2 * plane + c] = 0.f; }
            continue;
        }
        const float ds = g_mf * saved[b];
        const float* u = Eu + users[b] * ldu;
        const float* p = Ei + pos[b] * ldi;
        const float* q = Ei + neg[b] * ldi;
        for (int c = gl; c < d; c += 16) {
            const float uu = u[c], pp = p[c], qq = q[c];
            ru[c] = fmaf(ds, pp - qq, cu * uu);
            ru[plane + c] = fmaf(ds, uu, cp * pp);
            ru[2 * plane + c] = fmaf(-ds, uu, cq * qq);
        }
    }
}

// (Philox4x32-10, the keyed permutation and sample_one: guests.h)
__global__ void sample_bpr_kernel(uint64_t seed, uint64_t step, int64_t n_exist, const int64_t* __restrict__ exist_users,
                                  int64_t n_items, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                  int B, int half_bits, int64_t* __restrict__ users, int64_t* __restrict__ pos,
                                  int64_t* __restrict__ neg) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Philox ph(seed);
    sample_one(ph, (uint32_t)step, (uint32_t)(step >> 32), b, B, half_bits, n_exist, exist_users, n_items, rowptr, colidx,
               users[b], pos[b], neg[b]);
}

// The whole mini-batch of one step in ONE single-block launch that a HIP graph can replay: the step counter
// lives on the device and is advanced here. Slots [0, B): this rank's slice [slice_begin, slice_begin + B) of
// the global batch of B_global triples. Slots [B, B + n_aug): the LLM-augmented triples of reference
// main.py:216-224 - n_aug distinct users of the slice (random.sample), their (aug_pos, aug_neg) pair kept
// only if both ids are < n_items; kept pairs first, in draw order, then padding; n_valid = B + kept.
constexpr int SAMPLE_THREADS = 1024;
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_batch_kernel(
    uint64_t seed, unsigned long long* __restrict__ step_dev, int64_t n_exist, const int64_t* __restrict__ exist_users,
    int64_t n_items, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    int B_global, int half_bits_users, int slice_begin, int B, int n_aug, int half_bits_batch,
    const int64_t* __restrict__ aug_pos, const int64_t* __restrict__ aug_neg,
    int64_t* __restrict__ users, int64_t* __restrict__ pos, int64_t* __restrict__ neg, int32_t* __restrict__ n_valid_dev) {
    __shared__ int wave_tot[SAMPLE_THREADS / 64];
    __shared__ int base_s;
    const unsigned long long step = *step_dev;
    const uint32_t slo = (uint32_t)step, shi = (uint32_t)(step >> 32);
    const Philox ph(seed);
    for (int b = threadIdx.x; b < B; b += SAMPLE_THREADS)
        sample_one(ph, slo, shi, slice_begin + b, B_global, half_bits_users, n_exist, exist_users, n_items, rowptr, colidx,
                   users[b], pos[b], neg[b]);
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();                                                    // the slice is written (block-visible); everyone has read the step
    const Philox pa(seed ^ 0x9E3779B97F4A7C15ull);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int a0 = 0; a0 < n_aug; a0 += SAMPLE_THREADS) {               // block-uniform
        const int a = a0 + threadIdx.x;
        int64_t u = 0, ap = 0, an = 0;
        bool ok = false;
        if (a < n_aug) {
            const uint64_t slot = keyed_perm((uint64_t)a, (uint64_t)B, half_bits_batch, pa, slo, shi);   // distinct slots of the slice
            u = users[slot];
            ap = aug_pos[u]; an = aug_neg[u];
            ok = ap >= 0 && an >= 0 && ap < n_items && an < n_items;
        }
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wv] = __popcll(bal);
        __syncthreads();
        int wave_base = 0, chunk_tot = 0;
        for (int k = 0; k < SAMPLE_THREADS / 64; ++k) { const int t = wave_tot[k]; if (k < wv) wave_base += t; chunk_tot += t; }
        const int base = base_s;
        if (a < n_aug && ok) {
            const int o = B + base + wave_base + before;
            users[o] = u; pos[o] = ap; neg[o] = an;
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s = base + chunk_tot;
        __syncthreads();
    }
    const int kept = base_s;
    for (int o = B + kept + threadIdx.x; o < B + n_aug; o += SAMPLE_THREADS) { users[o] = 0; pos[o] = 0; neg[o] = 0; }   // padding (never read: beyond n_valid)
    if (threadIdx.x == 0) { n_valid_dev[0] = B + kept; *step_dev = step + 1ull; }
}

// The same batch by SEVERAL blocks (llmrec_sample_batch_wide): guests.h's body in 256-thread blocks.
constexpr int SAMPLE_WIDE_THREADS = 256;
__global__ __launch_bounds__(SAMPLE_WIDE_THREADS) void sample_batch_wide_kernel(SamplerArgs a) {
    guest_block<SAMPLE_WIDE_THREADS>(a, (int)blockIdx.x, nullptr);
}

// ---------------------------------------------------------------------------------------------
// WIDE selection (llmrec_bpr_prune_fwd_wide_f32): bpr_rank_kernel's decision for a list of ANY length. That kernel stages the whole
// global batch in LDS and compares every sample with every other one - O(B Bg) compares in 64 KB, hence LLMREC_BPR_MAX_B. Here the
// k-th smallest value is found by a most-significant-digit radix select over the order-preserving 32-bit image of m (four 8-bit
// digits), and the ties at that value are resolved by global index:
//   bpr_sel_init_kernel    clears the four 256-bin histograms of the workspace;
//   bpr_sel_hist_kernel    pass p = 0..3, one block per SEL_CHUNK list entries: the prologue picks digit p - 1 from the previous pass's
//                          histogram (every block does, redundantly; block 0 records it), then the block counts digit p of the entries
//                          that carry the digits picked so far - in LDS first, then into the workspace with INTEGER atomics (their sum
//                          does not depend on the order);
//   bpr_sel_count_kernel   picks the last digit -> the threshold image T and r = k - #{m < T}; writes eq[chunk] = #{m == T} of its chunk;
//   bpr_sel_write_kernel   chunk c adds eq[0 .. c), scans its own entries in index order and keeps  m < T  and the r equals of lowest
//                          global index; it writes this rank's samples of the chunk exactly as bpr_rank_kernel does.
// A kernel boundary is the only cross-block hand-over. Nothing here is a float sum: bpr_reduce_kernel, unchanged, produces the values.
// workspace (uint32 words): hist[4][256] | state[p] = (digits picked before pass p, what is left of k in their bucket), p = 1..4 | eq[chunks]
// ---------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 256;
constexpr int SEL_ITEMS = 8;
constexpr int SEL_CHUNK = SEL_THREADS * SEL_ITEMS;                     // list entries per block
constexpr int SEL_PASSES = 4;                                          // 8-bit digits of the 32-bit image
constexpr int SEL_WS_STATE = SEL_PASSES * 256;                         // word offset of state[0] (state[0] itself is never stored: (0, k))
constexpr int SEL_WS_EQ = SEL_WS_STATE + 16;                           // word offset of eq[]

struct SelArgs {
    const float* list;                 // the gathered log-sigmoids; null: the batch is local (the list is saved's m slots)
    int slots;                         // capacity of the list: global_B, or B_max for a local batch
    int B_max;
    const int32_t* n_valid_dev;
    double remember_rate;
    float* saved;
    int my_offset;                     // global index of this rank's sample 0
    uint32_t* ws;
    // the multi-problem form (llmrec_bpr_multi_select_bwd_wide_f32): problem blockIdx.y owns saved + y * saved_stride and ws + y * ws_stride
    int64_t saved_stride, ws_stride;   // floats / words between two problems' blocks (a single problem: gridDim.y = 1)
    int norm_block;                    // the write launch has one more block per problem: sel_norm_block
    const int64_t* users;              // the write launch of problem 0 stamps the batch's rows (any of the three may be absent)
    const int64_t* pos;
    const int64_t* neg;
    uint8_t* flag_u;
    uint8_t* flag_i;
    const int32_t* row_stamp;
};

// the arguments of the block's own problem
__device__ __forceinline__ SelArgs sel_mine(SelArgs a) {
    a.saved += (int64_t)blockIdx.y * a.saved_stride;
    a.ws += (int64_t)blockIdx.y * a.ws_stride;
    return a;
}

struct SelProblem { const float* list; int Bg, k; bool active; };      // active: 0 < k < Bg, a threshold has to be found
__device__ __forceinline__ SelProblem sel_problem(const SelArgs& a) {
    SelProblem s;
    s.list = a.list ? a.list : a.saved + a.B_max + 4;
    s.Bg = a.list ? a.slots : bpr_batch(a.n_valid_dev, a.B_max);
    s.k = (int)(a.remember_rate * (double)s.Bg);                       // bpr_rank_kernel's k
    s.active = s.k > 0 && s.k < s.Bg;
    return s;
}

// ascending image <=> ascending float; -0.0f and +0.0f share one image, as they compare equal
__device__ __forceinline__ uint32_t sel_key(float m) {
    const uint32_t u = m == 0.f ? 0u : __float_as_uint(m);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inclusive scan over the block's SEL_THREADS values (scan: SEL_THREADS words of LDS, free again on return)
__device__ __forceinline__ uint32_t sel_block_scan(uint32_t v, uint32_t* scan) {
    scan[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SEL_THREADS; off <<= 1) {
        const uint32_t w = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0u;
        __syncthreads();
        scan[threadIdx.x] += w;
        __syncthreads();
    }
    const uint32_t r = scan[threadIdx.x];
    __syncthreads();
    return r;
}

// state[p]: digit p - 1 is the bin of hist[p - 1] in which the state[p - 1].y-th smallest entry of the current bucket lies
__device__ __forceinline__ uint2 sel_state(const uint32_t* ws, int p, int k, uint32_t* scan, uint32_t* pick) {
    if (p == 0) return make_uint2(0u, (uint32_t)k);
    const uint32_t prefix = p == 1 ? 0u : ws[SEL_WS_STATE + 2 * (p - 1)];
    const uint32_t rem = p == 1 ? (uint32_t)k : ws[SEL_WS_STATE + 2 * (p - 1) + 1];
    const uint32_t h = ws[(p - 1) * 256 + threadIdx.x];
    const uint32_t incl = sel_block_scan(h, scan);
    if (threadIdx.x == 0) { pick[0] = prefix; pick[1] = 0u; }
    __syncthreads();
    if (incl - h < rem && rem <= incl) {                               // exactly one bin: 1 <= rem <= the bucket's size
        pick[0] = prefix | ((uint32_t)threadIdx.x << (32 - 8 * p));
        pick[1] = rem - (incl - h);
    }
    __syncthreads();
    return make_uint2(pick[0], pick[1]);
}

__global__ __launch_bounds__(SEL_THREADS) void bpr_sel_init_kernel(uint32_t* __restrict__ ws, int64_t ws_stride) {
    ws += (int64_t)blockIdx.y * ws_stride;
    for (int i = threadIdx.x; i < SEL_WS_STATE; i += SEL_THREADS) ws[i] = 0u;
}

__global__ __launch_bounds__(SEL_THREADS) void bpr_sel_hist_kernel(SelArgs a_, int p) {
    const SelArgs a = sel_mine(a_);
    __shared__ uint32_t scan[SEL_THREADS];
    __shared__ uint32_t h[256];
    __shared__ uint32_t pick[2];
    const SelProblem s = sel_problem(a);
    const int base = (int)blockIdx.x * SEL_CHUNK;
    if (!s.active || base >= s.Bg) return;                             // block-uniform (block 0 always stays: Bg > k > 0)
    const uint2 st = sel_state(a.ws, p, s.k, scan, pick);
    if (blockIdx.x == 0 && threadIdx.x == 0 && p > 0) { a.ws[SEL_WS_STATE + 2 * p] = st.x; a.ws[SEL_WS_STATE + 2 * p + 1] = st.y; }
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * p;
    const uint32_t himask = p == 0 ? 0u : 0xffffffffu << (shift + 8);
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int j = base + i * SEL_THREADS + (int)threadIdx.x;
        if (j < s.Bg) {
            const uint32_t key = sel_key(s.list[j]);
            if ((key & himask) == st.x) atomicAdd(&h[(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&a.ws[p * 256 + threadIdx.x], c);
}

__global__ __launch_bounds__(SEL_THREADS) void bpr_sel_count_kernel(SelArgs a_) {
    const SelArgs a = sel_mine(a_);
    __shared__ uint32_t scan[SEL_THREADS];
    __shared__ uint32_t pick[2];
    __shared__ uint32_t cnt;
    const SelProblem s = sel_problem(a);
    const int base = (int)blockIdx.x * SEL_CHUNK;
    if (!s.active) return;
    if (base >= s.Bg) { if (threadIdx.x == 0) a.ws[SEL_WS_EQ + blockIdx.x] = 0u; return; }
    const uint2 st = sel_state(a.ws, SEL_PASSES, s.k, scan, pick);     // (T, r)
    if (threadIdx.x == 0) {
        cnt = 0u;
        if (blockIdx.x == 0) { a.ws[SEL_WS_STATE + 2 * SEL_PASSES] = st.x; a.ws[SEL_WS_STATE + 2 * SEL_PASSES + 1] = st.y; }
    }
    __syncthreads();
    uint32_t c = 0u;
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int j = base + i * SEL_THREADS + (int)threadIdx.x;
        if (j < s.Bg) c += sel_key(s.list[j]) == st.x;
    }
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) a.ws[SEL_WS_EQ + blockIdx.x] = cnt;
}

__global__ __launch_bounds__(SEL_THREADS) void bpr_sel_write_kernel(SelArgs a_) {
    const SelArgs a = sel_mine(a_);
    __shared__ uint32_t scan[SEL_THREADS];
    __shared__ uint32_t before_s;
    const SelProblem s = sel_problem(a);
    const int B = bpr_batch(a.n_valid_dev, a.B_max);
    if (a.norm_block && blockIdx.x == gridDim.x - 1) {                 // (block-uniform) the squared norms' sums, as bpr_select_kernel's last block
        __shared__ float red[3][BPR_THREADS];
        sel_norm_block(a.saved, B, a.B_max, s.k, red);
        return;
    }
    const int base = (int)blockIdx.x * SEL_CHUNK;
    if (base + SEL_CHUNK <= a.my_offset || base >= a.my_offset + a.B_max) return;   // none of this rank's samples in the chunk (block-uniform)
    float* sc = a.saved + a.B_max + 4;
    const int j0 = base + (int)threadIdx.x * SEL_ITEMS;                // SEL_ITEMS consecutive entries per thread: index order
    uint32_t T = 0u, r = 0u, eq_before = 0u, keys[SEL_ITEMS];
    if (s.active) {
        T = a.ws[SEL_WS_STATE + 2 * SEL_PASSES]; r = a.ws[SEL_WS_STATE + 2 * SEL_PASSES + 1];
        if (threadIdx.x == 0) before_s = 0u;
        __syncthreads();
        uint32_t part = 0u;
        for (int c = threadIdx.x; c < (int)blockIdx.x; c += SEL_THREADS) part += a.ws[SEL_WS_EQ + c];
        if (part) atomicAdd(&before_s, part);
        uint32_t mine = 0u;
#pragma unroll
        for (int i = 0; i < SEL_ITEMS; ++i) {
            keys[i] = j0 + i < s.Bg ? sel_key(s.list[j0 + i]) : 0u;
            mine += j0 + i < s.Bg && keys[i] == T;
        }
        const uint32_t incl = sel_block_scan(mine, scan);              // (its barriers also publish before_s)
        eq_before = before_s + incl - mine;
    }
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int j = j0 + i, b = j - a.my_offset;
        bool keep = s.k >= s.Bg;
        if (s.active && j < s.Bg) {                                    // EVERY entry of the list advances the count of equals, whichever rank's
            const bool eq = keys[i] == T;                              // sample it is: a rank's samples need not begin at a thread's first entry
            keep = keys[i] < T || (eq && eq_before < r);
            eq_before += eq;
        }
        if (b < 0 || b >= a.B_max) continue;
        if (b >= B) { a.saved[b] = 0.f; sc[a.B_max + b] = 0.f; continue; }
        const float mb = sc[b];
        a.saved[b] = keep ? (-1.0f / (float)s.k) * sc[a.B_max + b] : 0.f;
        sc[a.B_max + b] = keep ? mb : 0.f;
        if (blockIdx.y == 0) {                                         // rows this batch touches (same rows for every problem)
            const uint8_t stamp = a.row_stamp ? LLMREC_ROW_STAMP(a.row_stamp[0]) : (uint8_t)1;
            if (a.flag_u) a.flag_u[a.users[b]] = stamp;
            if (a.flag_i) { a.flag_i[a.pos[b]] = stamp; a.flag_i[a.neg[b]] = stamp; }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The scatter plan of a batch of ANY size (llmrec_bpr_scatter_plan_wide): bpr_plan_kernel stages a side's keys in LDS (64 KB at
// B_max = 4096) and counts ranks, O(B^2). Here: the keys  id << 32 | slot  of both sides (one launch), one multi-block radix sort per
// side over the whole 64-bit key (the keys are distinct; the sort llmrec_scatter_rows_f32 issues, between two buffers of the
// workspace), then one launch that copies the sorted keys into the plan and writes the run lengths: a position is a head iff its id
// differs from its predecessor's, and the run ends at the upper bound of its id - a binary search, not a walk (a hub item is ONE run
// of up to 2 B positions).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bpr_plan_keys_kernel(const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                                            const int64_t* __restrict__ neg, int B_max,
                                                            const int32_t* __restrict__ n_valid_dev, uint64_t* __restrict__ keys) {
    const int B = bpr_batch(n_valid_dev, B_max);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;          // [0, B_max): the user side; [B_max, 3 B_max): the item side
    if (j >= 3 * (int64_t)B_max) return;
    const bool items = j >= B_max;
    const int i = (int)(items ? j - B_max : j);                        // the slot within the side
    const int b = (items && i >= B_max) ? i - B_max : i;
    uint64_t id = PLAN_NO_ID;
    if (b < B) id = (uint64_t)(items ? (i >= B_max ? neg[b] : pos[b]) : users[b]);
    keys[j] = (id << 32) | (uint64_t)(uint32_t)i;
}

// sorted_u / sorted_i: the sides' sorted keys (B_max / 2 B_max of them, outside the plan)
__global__ __launch_bounds__(256) void bpr_plan_runs_kernel(int B_max, const uint64_t* __restrict__ sorted_u, const uint64_t* __restrict__ sorted_i,
                                                            uint64_t* __restrict__ plan) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= 3 * (int64_t)B_max) return;
    const bool items = j >= B_max;
    const uint64_t* k = items ? sorted_i : sorted_u;
    const int n = items ? 2 * B_max : B_max;
    const int i = (int)(items ? j - B_max : j);
    const uint64_t me = k[i];
    const uint32_t id = (uint32_t)(me >> 32);
    plan[j] = me;
    int len = 0;
    if (id != PLAN_NO_ID && (i == 0 || (uint32_t)(k[i - 1] >> 32) != id)) {
        int lo = i + 1, hi = n;                                        // the first position in (i, n] whose id is above this one's
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((uint32_t)(k[mid] >> 32) > id) hi = mid; else lo = mid + 1;
        }
        len = lo - i;
    }
    reinterpret_cast<int32_t*>(plan + 3 * (int64_t)B_max)[j] = len;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

static int launch_bpr_fwd(const BprTables& t, int n_prob, int d, const int64_t* users, const int64_t* pos, const int64_t* neg,
                          int B_max, const int32_t* n_valid_dev, double remember_rate, float decay, float bsz,
                          float* out, float* saved, const BprGather& ga, bool do_scores, bool do_select, float* pack_out,
                          hipStream_t stream, StepBegin step_begin = StepBegin{}) {
    const int stride = LLMREC_BPR_SAVED_FLOATS(B_max);
    const BprGather none = {};
    if (do_scores && B_max > 0) {
        dim3 grid((unsigned)ceil_div(B_max, 16), (unsigned)n_prob);
        bpr_scores_kernel<<<grid, 256, 0, stream>>>(t, d, users, pos, neg, B_max, n_valid_dev, saved, stride, step_begin);
        LLMREC_LAUNCH_CHECK();
    }
    if (pack_out) {                                                     // local norm sums, then this rank's gather block
        bpr_reduce_kernel<<<n_prob, BPR_THREADS, 0, stream>>>(B_max, n_valid_dev, remember_rate, decay, bsz, out, saved, stride, none);
        LLMREC_LAUNCH_CHECK();
        bpr_pack_kernel<<<ceil_div(n_prob * B_max + 4 * n_prob + 1, 256), 256, 0, stream>>>(n_prob, B_max, n_valid_dev, saved, stride, pack_out);
        LLMREC_LAUNCH_CHECK();
    }
    if (do_select) {
        const size_t shmem = sizeof(float) * (size_t)(ga.g ? ga.n_ranks * ga.cap : (B_max > 0 ? B_max : 1));
        dim3 grid((unsigned)ceil_div(B_max > 0 ? B_max : 1, 16), (unsigned)n_prob);
        bpr_rank_kernel<<<grid, 256, shmem, stream>>>(B_max, n_valid_dev, remember_rate, saved, stride, ga);
        LLMREC_LAUNCH_CHECK();
        bpr_reduce_kernel<<<n_prob, BPR_THREADS, 0, stream>>>(B_max, n_valid_dev, remember_rate, decay, bsz, out, saved, stride, ga);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

int llmrec_bpr_prune_fwd_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev,
                             double remember_rate, float decay, float batch_size_flag,
                             float* out2, float* saved, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(B_max >= 0 && d > 0 && out2 && saved, "bpr_fwd: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_fwd: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_max == 0 || (Eu && Ei && users && pos && neg && ldu >= d && ldi >= d), "bpr_fwd: null pointer or ld < d");
    BprTables t = {};
    t.Eu[0] = Eu; t.Ei[0] = Ei; t.ldu[0] = ldu; t.ldi[0] = ldi;
    return launch_bpr_fwd(t, 1, d, users, pos, neg, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out2, saved,
                          BprGather{}, true, true, nullptr, (hipStream_t)stream_);
}

int llmrec_bpr_prune_fwd_sharded_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_local, double remember_rate, float decay, float batch_size_flag,
                                     const float* global_m, int32_t global_B, int32_t my_offset, int32_t scores_only,
                                     float* out2, float* saved, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(B_local >= 0 && d > 0 && out2 && saved, "bpr_fwd_sharded: bad argument");
    if (B_local > LLMREC_BPR_MAX_B || global_B > 3 * LLMREC_BPR_MAX_B) { set_error("bpr_fwd_sharded: batch too large"); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_local == 0 || (Eu && Ei && users && pos && neg && ldu >= d && ldi >= d), "bpr_fwd_sharded: null pointer or ld < d");
    LLMREC_CHECK_ARG(scores_only || (global_m && global_B >= B_local && my_offset >= 0 && my_offset + B_local <= global_B),
                     "bpr_fwd_sharded: pass 2 needs the gathered scores and a valid offset");
    BprTables t = {};
    t.Eu[0] = Eu; t.Ei[0] = Ei; t.ldu[0] = ldu; t.ldi[0] = ldi;
    // pass 1 writes the per-sample scratch (m at saved[B_local + 4 ...)); pass 2 only selects
    BprGather ga = {};
    if (!scores_only) { ga.g = global_m; ga.n_ranks = 1; ga.stride = 0; ga.cap = global_B; ga.n_prob = 1; ga.my_offset = my_offset; ga.has_tail = 0; }
    return launch_bpr_fwd(t, 1, d, users, pos, neg, B_local, nullptr, remember_rate, decay, batch_size_flag, out2, saved,
                          ga, scores_only != 0, scores_only == 0, nullptr, (hipStream_t)stream_);
}

int64_t llmrec_bpr_prune_wide_workspace_bytes(int64_t global_B) {
    if (global_B < 0 || global_B > LLMREC_BPR_WIDE_MAX_B) return -1;
    return align_up(4 * (SEL_WS_EQ + ceil_div(global_B > 0 ? global_B : 1, SEL_CHUNK)), 256);
}

int llmrec_bpr_prune_fwd_wide_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                  const int64_t* users, const int64_t* pos, const int64_t* neg,
                                  int32_t B_local, double remember_rate, float decay, float batch_size_flag,
                                  const float* global_m, int32_t global_B, int32_t my_offset, int32_t scores_only,
                                  float* out2, float* saved, const int32_t* n_valid_dev,
                                  void* workspace, int64_t workspace_bytes, llmrec_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LLMREC_CHECK_ARG(B_local >= 0 && d > 0 && out2 && saved, "bpr_fwd_wide: bad argument");
    if (B_local > LLMREC_BPR_WIDE_MAX_B || global_B > LLMREC_BPR_WIDE_MAX_B) {
        set_error("bpr_fwd_wide: batch of %d (global %d) > %d", B_local, global_B, LLMREC_BPR_WIDE_MAX_B);
        return LLMREC_EUNSUPPORTED;
    }
    LLMREC_CHECK_ARG(B_local == 0 || (Eu && Ei && users && pos && neg && ldu >= d && ldi >= d), "bpr_fwd_wide: null pointer or ld < d");
    const bool local = !global_m;
    if (!scores_only) {
        if (local) LLMREC_CHECK_ARG(my_offset == 0 && (global_B == 0 || global_B == B_local),
                                    "bpr_fwd_wide: a local batch (no gathered scores) has offset 0 and no other global size");
        else LLMREC_CHECK_ARG(global_B >= B_local && my_offset >= 0 && my_offset + (int64_t)B_local <= global_B,
                              "bpr_fwd_wide: pass 2 needs a valid offset into the gathered scores");
    }
    BprTables t = {};
    t.Eu[0] = Eu; t.Ei[0] = Ei; t.ldu[0] = ldu; t.ldi[0] = ldi;
    if (scores_only)                                                   // pass 1 of the sharded form: the per-sample scratch only
        return launch_bpr_fwd(t, 1, d, users, pos, neg, B_local, n_valid_dev, remember_rate, decay, batch_size_flag, out2, saved,
                              BprGather{}, true, false, nullptr, stream);
    const int slots = local ? B_local : global_B;
    const int64_t need = llmrec_bpr_prune_wide_workspace_bytes(slots);
    if (!workspace || workspace_bytes < need) {
        set_error("bpr_fwd_wide: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    if (local) {
        const int rc = launch_bpr_fwd(t, 1, d, users, pos, neg, B_local, n_valid_dev, remember_rate, decay, batch_size_flag, out2, saved,
                                      BprGather{}, true, false, nullptr, stream);
        if (rc != LLMREC_OK) return rc;
    }
    BprGather ga = {};
    if (!local) { ga.g = global_m; ga.n_ranks = 1; ga.stride = 0; ga.cap = global_B; ga.n_prob = 1; ga.my_offset = my_offset; ga.has_tail = 0; }
    SelArgs a = {};
    a.list = global_m; a.slots = slots; a.B_max = B_local; a.n_valid_dev = n_valid_dev; a.remember_rate = remember_rate; a.saved = saved;
    a.my_offset = my_offset; a.ws = (uint32_t*)workspace;
    const unsigned chunks = (unsigned)ceil_div(slots > 0 ? slots : 1, SEL_CHUNK);
    // a list length the host knows (no device batch count) settles k here: k <= 0 or k >= Bg needs no threshold
    const bool host_len = !local || !n_valid_dev;
    const int k_host = (int)(remember_rate * (double)slots);
    if (!(host_len && (k_host <= 0 || k_host >= slots))) {
        bpr_sel_init_kernel<<<1, SEL_THREADS, 0, stream>>>(a.ws, 0);
        LLMREC_LAUNCH_CHECK();
        for (int p = 0; p < SEL_PASSES; ++p) {
            bpr_sel_hist_kernel<<<chunks, SEL_THREADS, 0, stream>>>(a, p);
            LLMREC_LAUNCH_CHECK();
        }
        bpr_sel_count_kernel<<<chunks, SEL_THREADS, 0, stream>>>(a);
        LLMREC_LAUNCH_CHECK();
    }
    bpr_sel_write_kernel<<<chunks, SEL_THREADS, 0, stream>>>(a);
    LLMREC_LAUNCH_CHECK();
    bpr_reduce_kernel<<<1, BPR_THREADS, 0, stream>>>(B_local, n_valid_dev, remember_rate, decay, batch_size_flag, out2, saved,
                                                    LLMREC_BPR_SAVED_FLOATS(B_local), ga);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

static int fill_tables(BprTables& t, int n, const llmrec_bpr_problem_t* p, int d, bool need_grads) {
    for (int i = 0; i < n; ++i) {
        if (!p[i].Eu || !p[i].Ei || p[i].ldu < d || p[i].ldi < d) return 1;
        if (need_grads && (!p[i].dEu || !p[i].dEi || p[i].lddu < d || p[i].lddi < d)) return 1;
        t.Eu[i] = p[i].Eu; t.Ei[i] = p[i].Ei; t.ldu[i] = p[i].ldu; t.ldi[i] = p[i].ldi;
        t.dEu[i] = p[i].dEu; t.dEi[i] = p[i].dEi; t.lddu[i] = p[i].lddu; t.lddi[i] = p[i].lddi;
        t.g_mf[i] = p[i].g_mf; t.g_emb[i] = p[i].g_emb;
    }
    return 0;
}

int llmrec_bpr_multi_fwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                             float batch_size_flag, float* out, float* saved, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && out && saved,
                     "bpr_multi_fwd: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_fwd: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_max == 0 || (users && pos && neg), "bpr_multi_fwd: null index pointer");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, false), "bpr_multi_fwd: bad problem table");
    return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved,
                          BprGather{}, true, true, nullptr, (hipStream_t)stream_);
}

int llmrec_bpr_multi_fwd_sharded_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                     float batch_size_flag, int32_t phase, float* gather_block,
                                     const float* gathered, int32_t n_ranks, int64_t rank_stride, int32_t my_rank,
                                     float* out, float* saved, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && out && saved,
                     "bpr_multi_fwd_sharded: bad argument");
    LLMREC_CHECK_ARG(phase == 1 || phase == 2, "bpr_multi_fwd_sharded: phase is 1 (scores + gather block) or 2 (selection)");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_fwd_sharded: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_max == 0 || (users && pos && neg), "bpr_multi_fwd_sharded: null index pointer");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, false), "bpr_multi_fwd_sharded: bad problem table");
    if (phase == 1) {
        LLMREC_CHECK_ARG(gather_block, "bpr_multi_fwd_sharded: phase 1 needs the gather block");
        return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved,
                              BprGather{}, true, false, gather_block, (hipStream_t)stream_);
    }
    LLMREC_CHECK_ARG(gathered && n_ranks >= 1 && my_rank >= 0 && my_rank < n_ranks &&
                     rank_stride >= LLMREC_BPR_GATHER_FLOATS(n_problems, B_max), "bpr_multi_fwd_sharded: bad gathered layout");
    if ((int64_t)n_ranks * B_max > 4 * LLMREC_BPR_MAX_B) {
        set_error("bpr_multi_fwd_sharded: global batch capacity %lld > %d", (long long)n_ranks * B_max, 4 * LLMREC_BPR_MAX_B);
        return LLMREC_EUNSUPPORTED;
    }
    BprGather ga = {};
    ga.g = gathered; ga.n_ranks = n_ranks; ga.stride = rank_stride; ga.cap = B_max; ga.n_prob = n_problems;
    ga.my_offset = my_rank * B_max; ga.has_tail = 1;
    return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved,
                          ga, false, true, nullptr, (hipStream_t)stream_);
}

int llmrec_bpr_scatter_plan(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                            uint64_t* plan, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(B_max >= 0, "bpr_scatter_plan: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_scatter_plan: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(users && pos && neg && plan, "bpr_scatter_plan: null pointer");
    const unsigned blocks = (unsigned)plan_blocks_for(B_max, 256);
    bpr_plan_kernel<<<blocks, 256, sizeof(uint64_t) * 2 * (size_t)B_max, (hipStream_t)stream_>>>(users, pos, neg, B_max, n_valid_dev, plan);   // <= 64 KB of LDS
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_scatter_plan_reach_mark(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                                       uint64_t* plan, int64_t n_users, int64_t n_items, const int32_t* item_rowptr,
                                       const int32_t* item_colidx, uint8_t* flags, llmrec_stream_t stream_) {
    const llmrec_guest_plan_reach_t g = {users, pos, neg, B_max, n_valid_dev, plan, n_users, n_items, item_rowptr, item_colidx, flags};
    PlanReachArgs a;
    int64_t blocks;
    size_t shmem;
    const int rc = guest_prepare(g, 256, "bpr_scatter_plan_reach_mark", a, blocks, shmem);
    if (rc != LLMREC_OK || blocks == 0) return rc;
    bpr_plan_reach_mark_kernel<<<(unsigned)blocks, 256, shmem, (hipStream_t)stream_>>>(a);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

static int launch_bwd_runs(const BprTables& t, int n_prob, int d, const int64_t* users, const int64_t* pos, const int64_t* neg, int B_max,
                           float decay, float bsz, const float* saved, const uint64_t* plan, const float* grads2_dev, hipStream_t stream) {
    dim3 grid((unsigned)(ceil_div(B_max, 16) + ceil_div(2 * (int64_t)B_max, 16)), (unsigned)n_prob);
    bool vec = d % 4 == 0;                                             // float4 rows: every row pointer 16-byte aligned
    for (int i = 0; i < n_prob && vec; ++i)
        vec = t.ldu[i] % 4 == 0 && t.ldi[i] % 4 == 0 && t.lddu[i] % 4 == 0 && t.lddi[i] % 4 == 0 &&
              ((uintptr_t)t.Eu[i] | (uintptr_t)t.Ei[i] | (uintptr_t)t.dEu[i] | (uintptr_t)t.dEi[i]) % 16 == 0;
    const int stride = LLMREC_BPR_SAVED_FLOATS(B_max);
#define RUNS_LAUNCH(V, N) bpr_bwd_runs_kernel<V, N><<<grid, 256, 0, stream>>>(t, n_prob, d, users, pos, neg, B_max, decay, bsz, saved, stride, plan, grads2_dev)
    if (vec) { if (d <= 64) RUNS_LAUNCH(true, 1); else RUNS_LAUNCH(true, 2); }
    else { if (d <= 64) RUNS_LAUNCH(false, 1); else RUNS_LAUNCH(false, 2); }
#undef RUNS_LAUNCH
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_multi_bwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev, float decay, float batch_size_flag,
                             const float* saved, const uint64_t* plan, llmrec_stream_t stream_) {
    (void)n_valid_dev;                                                  // (the plan carries it: slots beyond n_valid are not listed)
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved,
                     "bpr_multi_bwd: bad argument");
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(users && pos && neg && plan, "bpr_multi_bwd: null index pointer or no scatter plan (llmrec_bpr_scatter_plan)");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, true), "bpr_multi_bwd: bad problem table");
    return launch_bwd_runs(t, n_problems, d, users, pos, neg, B_max, decay, batch_size_flag, saved, plan, nullptr, (hipStream_t)stream_);
}

int llmrec_bpr_multi_scores_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                const int64_t* users, const int64_t* pos, const int64_t* neg,
                                int32_t B_max, const int32_t* n_valid_dev, float* saved, int32_t* row_stamp, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved, "bpr_multi_scores: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_scores: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_max == 0 || (users && pos && neg), "bpr_multi_scores: null index pointer");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, false), "bpr_multi_scores: bad problem table");
    StepBegin sb = {};
    sb.row_stamp = row_stamp;
    return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, 0.0, 0.f, 1.f, nullptr, saved, BprGather{}, true, false,
                          nullptr, (hipStream_t)stream_, sb);
}

int llmrec_bpr_multi_scores_step_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, float* saved, int32_t* row_stamp,
                                     float* adamw_state3, float lr, float beta1, float beta2, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved, "bpr_multi_scores_step: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_scores_step: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    LLMREC_CHECK_ARG(B_max > 0 && users && pos && neg, "bpr_multi_scores_step: empty batch capacity or null index pointer (the launch carries the step's counters)");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, false), "bpr_multi_scores_step: bad problem table");
    StepBegin sb = {};
    sb.row_stamp = row_stamp; sb.adamw_state = adamw_state3; sb.lr = lr; sb.b1 = beta1; sb.b2 = beta2;
    return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, 0.0, 0.f, 1.f, nullptr, saved, BprGather{}, true, false,
                          nullptr, (hipStream_t)stream_, sb);
}

int llmrec_bpr_multi_select_bwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                    const int64_t* users, const int64_t* pos, const int64_t* neg,
                                    int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                    float batch_size_flag, float* saved, uint8_t* user_row_flags, uint8_t* item_row_flags,
                                    const int32_t* row_stamp, const uint64_t* plan, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved, "bpr_multi_select_bwd: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_select_bwd: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(users && pos && neg && plan, "bpr_multi_select_bwd: null index pointer or no scatter plan (llmrec_bpr_scatter_plan)");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, true), "bpr_multi_select_bwd: bad problem table");
    dim3 grid((unsigned)ceil_div(B_max, 16) + 1u, (unsigned)n_problems);
    const size_t shmem = sizeof(float) * (size_t)(B_max > 3 * BPR_THREADS ? B_max : 3 * BPR_THREADS);
    bpr_select_kernel<<<grid, 256, shmem, (hipStream_t)stream_>>>(users, pos, neg, B_max, n_valid_dev, remember_rate, saved,
                                                                 LLMREC_BPR_SAVED_FLOATS(B_max), user_row_flags, item_row_flags, row_stamp);
    LLMREC_LAUNCH_CHECK();
    return launch_bwd_runs(t, n_problems, d, users, pos, neg, B_max, decay, batch_size_flag, saved, plan, nullptr, (hipStream_t)stream_);
}

int llmrec_bpr_multi_losses_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                float batch_size_flag, float* out, float* saved, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && B_max >= 0 && out && saved, "bpr_multi_losses: bad argument");
    if (B_max > LLMREC_BPR_MAX_B) { set_error("bpr_multi_losses: B_max %d > %d", B_max, LLMREC_BPR_MAX_B); return LLMREC_EUNSUPPORTED; }
    bpr_reduce_kernel<<<n_problems, BPR_THREADS, 0, (hipStream_t)stream_>>>(B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved,
                                                                           LLMREC_BPR_SAVED_FLOATS(B_max), BprGather{});
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_multi_losses_assemble_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                         float batch_size_flag, float* out, float* saved, const float* w_mf_host,
                                         const float* sumsq_partial, int32_t n_partial, float feat_reg_coef,
                                         float* scal4, double* running_sums3, llmrec_stream_t stream_) {
    const llmrec_guest_losses_t g = {n_problems, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved, w_mf_host, sumsq_partial,
                                     n_partial, feat_reg_coef, scal4, running_sums3};
    LossesArgs a;
    int64_t blocks;
    size_t shmem;
    const int rc = guest_prepare(g, BPR_THREADS, "bpr_multi_losses_assemble", a, blocks, shmem);
    if (rc != LLMREC_OK) return rc;
    bpr_losses_assemble_kernel<<<1, BPR_THREADS, 0, (hipStream_t)stream_>>>(a);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_multi_zero_rows_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                   const int64_t* users, const int64_t* pos, const int64_t* neg,
                                   int32_t B_max, const int32_t* n_valid_dev, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0, "bpr_multi_zero_rows: bad argument");
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(users && pos && neg, "bpr_multi_zero_rows: null index pointer");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, true), "bpr_multi_zero_rows: bad problem table");
    dim3 grid((unsigned)ceil_div(B_max, 16), (unsigned)n_problems);
    bpr_zero_rows_kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(t, d, users, pos, neg, B_max, n_valid_dev);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

// ---- the eight-problem loss segment beyond LLMREC_BPR_MAX_B (FusedStep above FusedStep.WIDE_FROM) ----
static int wide_refused(const char* who, int64_t B_max) {
    if (B_max <= LLMREC_BPR_WIDE_MAX_B) return 0;
    set_error("%s: B_max %lld > %d", who, (long long)B_max, LLMREC_BPR_WIDE_MAX_B);
    return 1;
}

// plan workspace: the 3 B_max keys | the sort's second key buffer | its temporary storage (llmrec_scatter_rows_workspace_bytes' bound)
static int64_t plan_wide_keys_bytes(int64_t B_max) { return align_up(8 * 3 * B_max, 256); }
static int64_t plan_wide_temp_bytes(int64_t B_max) { return align_up(2 * B_max + (32ll << 20), 256); }

int64_t llmrec_bpr_scatter_plan_wide_workspace_bytes(int64_t B_max) {
    if (B_max < 0 || B_max > LLMREC_BPR_WIDE_MAX_B) return -1;
    return 2 * plan_wide_keys_bytes(B_max) + plan_wide_temp_bytes(B_max);
}

int llmrec_bpr_scatter_plan_wide(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                                 uint64_t* plan, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LLMREC_CHECK_ARG(B_max >= 0, "bpr_scatter_plan_wide: bad argument");
    if (wide_refused("bpr_scatter_plan_wide", B_max)) return LLMREC_EUNSUPPORTED;
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(users && pos && neg && plan, "bpr_scatter_plan_wide: null pointer");
    const int64_t need_ws = llmrec_bpr_scatter_plan_wide_workspace_bytes(B_max);
    if (!workspace || workspace_bytes < need_ws) {
        set_error("bpr_scatter_plan_wide: workspace %lld < %lld", (long long)workspace_bytes, (long long)need_ws);
        return LLMREC_EWORKSPACE;
    }
    uint64_t* keys = (uint64_t*)workspace;
    uint64_t* alt = (uint64_t*)((char*)workspace + plan_wide_keys_bytes(B_max));
    void* temp = (char*)workspace + 2 * plan_wide_keys_bytes(B_max);
    const size_t temp_avail = (size_t)plan_wide_temp_bytes(B_max);
    hipcub::DoubleBuffer<uint64_t> ubuf(keys, alt), ibuf(keys + B_max, alt + B_max);
    size_t need_u = 0, need_i = 0;                                      // (both queries before the first launch)
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need_u, ubuf, B_max, 0, 64, stream));
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need_i, ibuf, 2 * B_max, 0, 64, stream));
    if (need_u > temp_avail || need_i > temp_avail) {
        set_error("bpr_scatter_plan_wide: the sort needs %zu B of temporary storage > %zu", need_u > need_i ? need_u : need_i, temp_avail);
        return LLMREC_EWORKSPACE;
    }
    const unsigned blocks = (unsigned)ceil_div(3 * (int64_t)B_max, 256);
    bpr_plan_keys_kernel<<<blocks, 256, 0, stream>>>(users, pos, neg, B_max, n_valid_dev, keys);
    LLMREC_LAUNCH_CHECK();
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(temp, need_u, ubuf, B_max, 0, 64, stream));
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(temp, need_i, ibuf, 2 * B_max, 0, 64, stream));
    bpr_plan_runs_kernel<<<blocks, 256, 0, stream>>>(B_max, ubuf.Current(), ibuf.Current(), plan);   // (which buffer: settled on the host)
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_multi_scores_wide_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, float* saved, int32_t* row_stamp,
                                     float* adamw_state3, float lr, float beta1, float beta2, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved, "bpr_multi_scores_wide: bad argument");
    if (wide_refused("bpr_multi_scores_wide", B_max)) return LLMREC_EUNSUPPORTED;
    LLMREC_CHECK_ARG(B_max > 0 && users && pos && neg, "bpr_multi_scores_wide: empty batch capacity or null index pointer (the launch carries the step's counters)");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, false), "bpr_multi_scores_wide: bad problem table");
    StepBegin sb = {};
    sb.row_stamp = row_stamp; sb.adamw_state = adamw_state3; sb.lr = lr; sb.b1 = beta1; sb.b2 = beta2;
    return launch_bpr_fwd(t, n_problems, d, users, pos, neg, B_max, n_valid_dev, 0.0, 0.f, 1.f, nullptr, saved, BprGather{}, true, false,
                          nullptr, (hipStream_t)stream_, sb);
}

// per problem: hist[4][256] | state | eq[chunks], a whole number of 256-byte lines
static int64_t sel_problem_words(int64_t B_max) { return align_up(4 * (SEL_WS_EQ + ceil_div(B_max > 0 ? B_max : 1, SEL_CHUNK)), 256) / 4; }

int64_t llmrec_bpr_multi_wide_workspace_bytes(int32_t n_problems, int64_t B_max) {
    if (n_problems < 1 || n_problems > LLMREC_BPR_MAX_PROBLEMS || B_max < 0 || B_max > LLMREC_BPR_WIDE_MAX_B) return -1;
    return 4 * n_problems * sel_problem_words(B_max);
}

int llmrec_bpr_multi_select_bwd_wide_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                         const int64_t* users, const int64_t* pos, const int64_t* neg,
                                         int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                         float batch_size_flag, float* saved, uint8_t* user_row_flags, uint8_t* item_row_flags,
                                         const int32_t* row_stamp, const uint64_t* plan,
                                         void* workspace, int64_t workspace_bytes, llmrec_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && problems_host && d > 0 && saved, "bpr_multi_select_bwd_wide: bad argument");
    if (wide_refused("bpr_multi_select_bwd_wide", B_max)) return LLMREC_EUNSUPPORTED;
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(B_max > 0 && users && pos && neg && plan, "bpr_multi_select_bwd_wide: null index pointer or no scatter plan (llmrec_bpr_scatter_plan_wide)");
    BprTables t = {};
    LLMREC_CHECK_ARG(!fill_tables(t, n_problems, problems_host, d, true), "bpr_multi_select_bwd_wide: bad problem table");
    const int64_t need = llmrec_bpr_multi_wide_workspace_bytes(n_problems, B_max);
    if (!workspace || workspace_bytes < need) {
        set_error("bpr_multi_select_bwd_wide: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    SelArgs a = {};
    a.slots = B_max; a.B_max = B_max; a.n_valid_dev = n_valid_dev; a.remember_rate = remember_rate; a.saved = saved;
    a.ws = (uint32_t*)workspace; a.saved_stride = LLMREC_BPR_SAVED_FLOATS(B_max); a.ws_stride = sel_problem_words(B_max);
    a.norm_block = 1; a.users = users; a.pos = pos; a.neg = neg; a.flag_u = user_row_flags; a.flag_i = item_row_flags; a.row_stamp = row_stamp;
    const unsigned chunks = (unsigned)ceil_div(B_max, SEL_CHUNK);
    const dim3 grid(chunks, (unsigned)n_problems);
    // a batch size the host knows (no device count) settles k here: k <= 0 or k >= B needs no threshold
    const int k_host = (int)(remember_rate * (double)B_max);
    if (n_valid_dev || (k_host > 0 && k_host < B_max)) {
        bpr_sel_init_kernel<<<dim3(1, (unsigned)n_problems), SEL_THREADS, 0, stream>>>(a.ws, a.ws_stride);
        LLMREC_LAUNCH_CHECK();
        for (int p = 0; p < SEL_PASSES; ++p) {
            bpr_sel_hist_kernel<<<grid, SEL_THREADS, 0, stream>>>(a, p);
            LLMREC_LAUNCH_CHECK();
        }
        bpr_sel_count_kernel<<<grid, SEL_THREADS, 0, stream>>>(a);
        LLMREC_LAUNCH_CHECK();
    }
    bpr_sel_write_kernel<<<dim3(chunks + 1u, (unsigned)n_problems), SEL_THREADS, 0, stream>>>(a);   // (+ 1: the norm block)
    LLMREC_LAUNCH_CHECK();
    return launch_bwd_runs(t, n_problems, d, users, pos, neg, B_max, decay, batch_size_flag, saved, plan, nullptr, stream);
}

int llmrec_bpr_multi_losses_wide_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                     float batch_size_flag, float* out, float* saved, const float* w_mf_host,
                                     const float* sumsq_partial, int32_t n_partial, float feat_reg_coef,
                                     float* scal4, double* running_sums3, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_problems >= 1 && n_problems <= LLMREC_BPR_MAX_PROBLEMS && B_max >= 0 && out && saved && (w_mf_host || !scal4),
                     "bpr_multi_losses_wide: bad argument");
    LLMREC_CHECK_ARG(n_partial >= 0 && (n_partial == 0 || (sumsq_partial && scal4)), "bpr_multi_losses_wide: partial sums without a buffer");
    if (wide_refused("bpr_multi_losses_wide", B_max)) return LLMREC_EUNSUPPORTED;
    LossW w = {};
    for (int i = 0; i < n_problems && w_mf_host; ++i) w.w[i] = w_mf_host[i];
    const LossesArgs a = {n_problems, B_max, n_valid_dev, remember_rate, decay, batch_size_flag, out, saved, (int)LLMREC_BPR_SAVED_FLOATS(B_max), w,
                          n_partial > 0 ? sumsq_partial : nullptr, n_partial, feat_reg_coef, scal4, scal4 ? running_sums3 : nullptr};
    bpr_losses_assemble_kernel<<<1, BPR_THREADS, 0, (hipStream_t)stream_>>>(a);   // scal4 == NULL: the loss values only
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_bpr_prune_bwd_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev, float decay, float batch_size_flag,
                             const float* saved, const float* grads2,
                             float* dEu, int64_t lddu, float* dEi, int64_t lddi, const uint64_t* plan, llmrec_stream_t stream_) {
    (void)n_valid_dev;
    LLMREC_CHECK_ARG(B_max >= 0 && d > 0 && saved && grads2, "bpr_bwd: bad argument");
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(Eu && Ei && users && pos && neg && dEu && dEi && ldu >= d && ldi >= d && lddu >= d && lddi >= d,
                     "bpr_bwd: null pointer or ld < d");
    LLMREC_CHECK_ARG(plan, "bpr_bwd: no scatter plan (llmrec_bpr_scatter_plan)");
    LLMREC_CHECK_ARG(dEu != dEi, "bpr_bwd: dEu and dEi must be distinct buffers");
    BprTables t = {};
    t.Eu[0] = Eu; t.Ei[0] = Ei; t.ldu[0] = ldu; t.ldi[0] = ldi;
    t.dEu[0] = dEu; t.dEi[0] = dEi; t.lddu[0] = lddu; t.lddi[0] = lddi;
    return launch_bwd_runs(t, 1, d, users, pos, neg, B_max, decay, batch_size_flag, saved, plan, grads2, (hipStream_t)stream_);
}

int llmrec_bpr_prune_bwd_rows_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                  const int64_t* users, const int64_t* pos, const int64_t* neg,
                                  int32_t B_max, const int32_t* n_valid_dev, float decay, float batch_size_flag,
                                  const float* saved, const float* grads2, float* rows3, llmrec_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LLMREC_CHECK_ARG(B_max >= 0 && d > 0 && saved && grads2, "bpr_bwd_rows: bad argument");
    if (B_max == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(Eu && Ei && users && pos && neg && rows3 && ldu >= d && ldi >= d, "bpr_bwd_rows: null pointer or ld < d");
    bpr_bwd_rows_kernel<<<grid_for(B_max, 16), 256, 0, stream>>>(Eu, ldu, Ei, ldi, d, users, pos, neg, B_max, n_valid_dev, decay,
                                                                 batch_size_flag, saved, grads2, rows3);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_sample_bpr(uint64_t seed, uint64_t step, int64_t n_exist_users, const int64_t* exist_users,
                      int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                      int32_t B, int64_t* users, int64_t* pos, int64_t* neg, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(B >= 0 && n_exist_users > 0 && n_items > 0, "sample_bpr: bad sizes");
    if (B == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(exist_users && train_rowptr && train_colidx && users && pos && neg, "sample_bpr: null pointer");
    int half_bits = 1;
    while ((1ull << (2 * half_bits)) < (uint64_t)n_exist_users) ++half_bits;
    sample_bpr_kernel<<<(B + 255) / 256, 256, 0, (hipStream_t)stream_>>>(seed, step, n_exist_users, exist_users, n_items,
                                                                          train_rowptr, train_colidx, B, half_bits, users, pos, neg);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_sample_batch(uint64_t seed, uint64_t* step_dev, int64_t n_exist_users, const int64_t* exist_users,
                        int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                        int32_t B_global, int32_t slice_begin, int32_t B, int32_t n_aug,
                        const int64_t* aug_pos, const int64_t* aug_neg,
                        int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_valid_dev, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(B >= 1 && B_global >= B && slice_begin >= 0 && slice_begin + B <= B_global && n_aug >= 0 && n_aug <= B &&
                     n_exist_users > 0 && n_items > 0, "sample_batch: bad sizes");
    LLMREC_CHECK_ARG(step_dev && exist_users && train_rowptr && train_colidx && users && pos && neg && n_valid_dev,
                     "sample_batch: null pointer");
    LLMREC_CHECK_ARG(n_aug == 0 || (aug_pos && aug_neg), "sample_batch: augmented pairs missing");
    int hb_users = 1, hb_batch = 1;
    while ((1ull << (2 * hb_users)) < (uint64_t)n_exist_users) ++hb_users;
    while ((1ull << (2 * hb_batch)) < (uint64_t)B) ++hb_batch;
    sample_batch_kernel<<<1, SAMPLE_THREADS, 0, (hipStream_t)stream_>>>(seed, (unsigned long long*)step_dev, n_exist_users, exist_users,
                                                                       n_items, train_rowptr, train_colidx, B_global, hb_users,
                                                                       slice_begin, B, n_aug, hb_batch, aug_pos, aug_neg,
                                                                       users, pos, neg, n_valid_dev);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_sample_batch_wide(uint64_t seed, uint64_t* step_dev, int64_t n_exist_users, const int64_t* exist_users,
                             int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                             int32_t B_global, int32_t slice_begin, int32_t B, int32_t n_aug,
                             const int64_t* aug_pos, const int64_t* aug_neg,
                             int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_valid_dev, int32_t* ticket, llmrec_stream_t stream_) {
    const llmrec_guest_sampler_t g = {seed, step_dev, n_exist_users, exist_users, n_items, train_rowptr, train_colidx, B_global, slice_begin, B,
                                      n_aug, aug_pos, aug_neg, users, pos, neg, n_valid_dev, ticket};
    SamplerArgs a;
    int64_t blocks;
    size_t shmem;
    const int rc = guest_prepare(g, SAMPLE_WIDE_THREADS, "sample_batch_wide", a, blocks, shmem);
    if (rc != LLMREC_OK) return rc;
    sample_batch_wide_kernel<<<(unsigned)blocks, SAMPLE_WIDE_THREADS, 0, (hipStream_t)stream_>>>(a);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
