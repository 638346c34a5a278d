// foldin.hip - serving: the embedding of a user who is NOT a row of the training graph, from an item history (llmrec_fold_in_users_f32).
//
// The trained model's user embedding is, term by term, the user's row of the normalised adjacency times an item-side table - except the
// user's own id row. Hold the item side fixed and the same formula embeds a new row. The item-side tables arrive as ONE table
// T [n_items][C d], C = L + 2 + n_attr + 1 slices of d columns in the order  chain I_0 .. I_{L-1} | image | text | attributes | profile,
// so that one gathered item is one contiguous read of C d floats.
//
//   S       = sum over the row's entries of T[entry]                  (all C slices at once; fp32, fixed order - below)
//   g(c)    = row_scale . S[slice c]
//   u_l     = g(l - 1), l = 1 .. L; the last one through the row softmax over d
//   out     = (id_row + u_1 + ... + u_L) . fl(1 / (L + 1))
//             + c_m n(g(image)) + c_m n(g(text)) + c_u n(g(profile)) + sum_k c_a n(g(attribute k)),   n(x) = x / max(||x||, 1e-12)
// the mean and the normalise-and-add in the order and with the operations of fuse_fwd_kernel (rowops.hip).
//
// THE ORDER OF A ROW'S SUM depends on the row's length alone. The row is cut into segments of FI_SEG = 256 entries; a block of four waves
// sums one segment: wave w takes the entries [w q, (w + 1) q) of the segment, q = ceil(segment length / 4), and adds them IN THE ORDER
// GIVEN into one accumulator per column (a lane owns the columns (lane + 64 i) VEC .. + VEC); the four wave sums meet in LDS as
// (w0 + w1) + (w2 + w3). A row of one segment is finished by the same block. A longer row leaves its segment sums in the workspace and
// fi_finish_long_kernel adds them in segment order, 0, 1, 2 ..., and finishes. No atomics; a row's bits do not depend on the other rows
// of the call, on its position, or on the run.
//
// WHICH BLOCK SUMS WHAT needs no host read and no scan: block r < n takes segment 0 of row r; block n + j, j < floor(nnz / 256), takes
// segment k >= 1 of the row r with floor(rowptr[r] / 256) + k - 1 == j, if there is one (the largest r with floor(rowptr[r] / 256) <= j,
// found by binary search; the slots of two rows cannot meet because floor((s + len) / 256) >= floor(s / 256) + ceil(len / 256) - 1).
// The workspace holds one [C d] slot per block. Grids, slots and launch count come from the host arguments: capturable.
//
// An entry < 0 or >= n_items adds nothing (-1 padding; a bad id cannot fault); a repeated entry counts every time. A row whose pointers
// do not satisfy 0 <= rowptr[r] <= rowptr[r + 1] <= nnz is treated as empty.
#include "common.h"

namespace llmrec {

constexpr int FI_SEG = 256;                                        // entries of a row that one block sums
constexpr int FI_MAX_W = 2048;                                     // floats of a gathered row, C d: 4 wave sums of it are 32 KiB of LDS

struct FiArgs {
    int n;
    const int32_t* rowptr;
    const int32_t* colidx;
    int64_t nnz;
    const float* row_scale;
    const float* id_rows;
    int64_t ldid;
    const float* T;
    int64_t ldt, n_items;
    int L, n_attr, d, C, W;
    float mean_scale, c_m, c_u, c_a;
    float* out;
    int64_t ldo;
    float* ws;
};

// (first entry, length) of row r; pointers that are no CSR row give an empty row
__device__ __forceinline__ void fi_row(const FiArgs& a, int r, int64_t& s, int64_t& len) {
    const int64_t b = a.rowptr[r], e = a.rowptr[r + 1];
    const bool ok = b >= 0 && e >= b && e <= a.nnz;
    s = ok ? b : 0;
    len = ok ? e - b : 0;
}

__device__ __forceinline__ int64_t fi_nseg(int64_t len) { return len > FI_SEG ? (len + FI_SEG - 1) / FI_SEG : 1; }

// the row's [C d] sums S (LDS) -> out[r]; one wave, lane owns the columns lane and lane + 64 (d <= 128)
__device__ __forceinline__ void fi_finish(const float* __restrict__ S, const FiArgs& a, int r, int lane) {
#pragma clang fp contract(off)                                     // w . S is rounded before it is added: the order tests/_foldin_ref.py restates
    const int d = a.d;
    const float w = a.row_scale[r];
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < d, in1 = c1 < d;
    float acc0 = 0.f, acc1 = 0.f;
    if (a.id_rows) {
        const float* id = a.id_rows + (int64_t)r * a.ldid;
        acc0 = in0 ? id[c0] : 0.f;
        acc1 = in1 ? id[c1] : 0.f;
    }
    for (int l = 0; l < a.L; ++l) {
        const float* s = S + l * d;
        float x0 = in0 ? w * s[c0] : 0.f, x1 = in1 ? w * s[c1] : 0.f;
        if (l == a.L - 1) {                                        // the last layer's row softmax, as softmax_fwd_kernel
            float mx = fmaxf(in0 ? x0 : -INFINITY, in1 ? x1 : -INFINITY);
            mx = group_max<64>(mx);
            x0 = in0 ? expf(x0 - mx) : 0.f;
            x1 = in1 ? expf(x1 - mx) : 0.f;
            const float inv = 1.0f / group_sum<64>(x0 + x1);
            x0 = x0 * inv;
            x1 = x1 * inv;
        }
        acc0 += x0;
        acc1 += x1;
    }
    acc0 = acc0 * a.mean_scale;
    acc1 = acc1 * a.mean_scale;
    const int n_norm = 3 + a.n_attr;
    for (int t = 0; t < n_norm; ++t) {                             // image, text, profile, attributes: fuse_fwd_kernel's order
        const int slice = t < 2 ? a.L + t : (t == 2 ? a.C - 1 : a.L + t - 1);
        const float rate = t < 2 ? a.c_m : (t == 2 ? a.c_u : a.c_a);
        const float* s = S + slice * d;
        const float x0 = in0 ? w * s[c0] : 0.f, x1 = in1 ? w * s[c1] : 0.f;
        const float ss = group_sum<64>(fmaf(x1, x1, fmaf(x0, x0, 0.f)));
        const float nrm = fmaxf(sqrtf(ss), 1e-12f);                // F.normalize eps
        const float wt = rate / nrm;
        acc0 = fmaf(wt, x0, acc0);
        acc1 = fmaf(wt, x1, acc1);
    }
    float* o = a.out + (int64_t)r * a.ldo;
    if (in0) o[c0] = acc0;
    if (in1) o[c1] = acc1;
}

template <int VEC> struct FiVec;
template <> struct FiVec<4> {
    typedef float4 type;
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ void add(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
};
template <> struct FiVec<1> {
    typedef float type;
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ void add(float& a, const float& b) { a += b; }
};

// one block = one segment of one row (the header comment says which); dynamic LDS: 4 W floats
template <int VEC>
__global__ __launch_bounds__(256) void fi_gather_kernel(FiArgs a) {
    extern __shared__ float4 fi_lds[];
    float* part = reinterpret_cast<float*>(fi_lds);                // [4][W]: the wave sums; [0] then holds the segment's sum
    typedef typename FiVec<VEC>::type VT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int r;
    int64_t k, s, len;
    if ((int64_t)blockIdx.x < a.n) {
        r = (int)blockIdx.x;
        k = 0;
        fi_row(a, r, s, len);
    } else {
        const int64_t j = (int64_t)blockIdx.x - a.n;
        int lo = 0, hi = a.n - 1;                                  // the largest r with floor(rowptr[r] / FI_SEG) <= j (row 0 qualifies)
        while (lo < hi) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            int64_t p = a.rowptr[mid];
            p = p < 0 ? 0 : p;
            if (p / FI_SEG <= j) lo = mid; else hi = mid - 1;
        }
        r = lo;
        fi_row(a, r, s, len);
        k = j - s / FI_SEG + 1;
        if (k < 1) return;                                         // (block-uniform, as every return here)
    }
    const int64_t nseg = fi_nseg(len);
    if (k >= nseg) return;
    const int64_t seg0 = s + k * FI_SEG;
    const int seglen = (int)(len - k * FI_SEG < FI_SEG ? len - k * FI_SEG : FI_SEG);
    const int q = (seglen + 3) >> 2;
    const int64_t e0 = seg0 + (wv * q < seglen ? wv * q : seglen), e1 = seg0 + ((wv + 1) * q < seglen ? (wv + 1) * q : seglen);
    const int WU = a.W / VEC;
    for (int u = lane; u < WU; u += 64) {
        const float* col = a.T + (int64_t)u * VEC;
        VT acc = FiVec<VEC>::zero();
        for (int64_t e = e0; e < e1; e += 4) {                     // four rows in flight, added in the order given
            VT v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t id = e + i < e1 ? (int64_t)a.colidx[e + i] : -1;
                v[i] = id >= 0 && id < a.n_items ? *reinterpret_cast<const VT*>(col + id * a.ldt) : FiVec<VEC>::zero();
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) FiVec<VEC>::add(acc, v[i]);
        }
        *reinterpret_cast<VT*>(part + wv * a.W + u * VEC) = acc;
    }
    __syncthreads();
    float* slot = a.ws ? a.ws + (int64_t)blockIdx.x * a.W : nullptr;
    for (int i = threadIdx.x; i < a.W; i += 256) {
        const float sum = (part[i] + part[a.W + i]) + (part[2 * a.W + i] + part[3 * a.W + i]);
        if (nseg == 1) part[i] = sum;
        else if (slot) slot[i] = sum;
    }
    if (nseg != 1) return;
    __syncthreads();
    if (wv == 0) fi_finish(part, a, r, lane);
}

// one block per row of more than one segment: the segment sums in segment order, then the finish; dynamic LDS: W floats
__global__ __launch_bounds__(256) void fi_finish_long_kernel(FiArgs a) {
    extern __shared__ float4 fi_lds[];
    float* S = reinterpret_cast<float*>(fi_lds);
    const int r = (int)blockIdx.x;
    int64_t s, len;
    fi_row(a, r, s, len);
    const int64_t nseg = fi_nseg(len);
    if (nseg < 2) return;
    const float* first = a.ws + (int64_t)r * a.W;
    const float* rest = a.ws + ((int64_t)a.n + s / FI_SEG) * a.W;   // the slots of segments 1 .. nseg - 1, one after the other
    for (int i = threadIdx.x; i < a.W; i += 256) {
        float acc = first[i];
        for (int64_t k = 1; k < nseg; ++k) acc += rest[(k - 1) * a.W + i];
        S[i] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 64) fi_finish(S, a, r, (int)threadIdx.x);
}

static bool fi_sizes_ok(int64_t n, int64_t nnz, int32_t L, int32_t n_attr, int32_t d) {
    return n >= 0 && n < (1ll << 31) && nnz >= 0 && nnz < (1ll << 31) && L >= 1 && n_attr >= 0 && 3 + n_attr <= LLMREC_MAX_TERMS && d >= 1 &&
           L <= FI_MAX_W;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int64_t llmrec_fold_in_users_workspace_bytes(int32_t n, int64_t nnz, int32_t L, int32_t n_attr, int32_t d) {
    if (!fi_sizes_ok(n, nnz, L, n_attr, d)) return -1;
    if (nnz <= FI_SEG) return 0;                                   // no row can have a second segment
    return ((int64_t)n + nnz / FI_SEG) * (L + 3 + n_attr) * d * 4;
}

int llmrec_fold_in_users_f32(int32_t n, const int32_t* rowptr, const int32_t* colidx, int64_t nnz, const float* row_scale,
                             const float* id_rows, int64_t ldid, const float* T, int64_t ldt, int64_t n_items,
                             int32_t L, int32_t n_attr, int32_t d, float c_m, float c_u, float c_a,
                             float* out, int64_t ldo, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(fi_sizes_ok(n, nnz, L, n_attr, d), "fold_in_users: bad sizes (n, nnz in [0, 2^31), L >= 1, 0 <= n_attr <= %d, d >= 1)",
                     LLMREC_MAX_TERMS - 3);
    LLMREC_CHECK_ARG(n_items > 0 && n_items < (1ll << 31), "fold_in_users: n_items outside (0, 2^31)");
    const int64_t C = (int64_t)L + 3 + n_attr, W = C * d;
    if (d > 128 || W > FI_MAX_W) {
        set_error("fold_in_users: d = %d > 128 or (L + 3 + n_attr) d = %lld > %d", d, (long long)W, FI_MAX_W);
        return LLMREC_EUNSUPPORTED;
    }
    if (n == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(rowptr && row_scale && T && out && ldt >= W && ldo >= d, "fold_in_users: null pointer or ld too small (ldt >= (L + 3 + n_attr) d)");
    LLMREC_CHECK_ARG(colidx || nnz == 0, "fold_in_users: nnz > 0 without colidx");
    LLMREC_CHECK_ARG(!id_rows || ldid >= d, "fold_in_users: id_rows with ld < d");
    const int64_t extra = nnz > FI_SEG ? nnz / FI_SEG : 0;
    const int64_t need = extra ? ((int64_t)n + extra) * W * 4 : 0;
    if (need) {
        LLMREC_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0, "fold_in_users: nnz > %d needs the workspace (16-byte aligned)", FI_SEG);
        if (workspace_bytes < need) {
            set_error("fold_in_users: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
            return LLMREC_EWORKSPACE;
        }
    }
    FiArgs a;
    a.n = n; a.rowptr = rowptr; a.colidx = colidx; a.nnz = nnz; a.row_scale = row_scale; a.id_rows = id_rows; a.ldid = ldid;
    a.T = T; a.ldt = ldt; a.n_items = n_items; a.L = L; a.n_attr = n_attr; a.d = d; a.C = (int)C; a.W = (int)W;
    a.mean_scale = 1.0f / (float)(L + 1); a.c_m = c_m; a.c_u = c_u; a.c_a = c_a; a.out = out; a.ldo = ldo;
    a.ws = need ? (float*)workspace : nullptr;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned grid = (unsigned)((int64_t)n + extra);
    const size_t lds = (size_t)4 * W * sizeof(float);
    if (d % 4 == 0 && ldt % 4 == 0 && (uintptr_t)T % 16 == 0) fi_gather_kernel<4><<<grid, 256, lds, stream>>>(a);
    else fi_gather_kernel<1><<<grid, 256, lds, stream>>>(a);
    LLMREC_LAUNCH_CHECK();
    if (extra) {
        fi_finish_long_kernel<<<(unsigned)n, 256, (size_t)W * sizeof(float), stream>>>(a);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

}  // extern "C"
