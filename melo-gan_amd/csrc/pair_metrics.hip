// Pairwise feature-space metrics of the held-out evaluation (melo_gan_amd/gan/evaluate.py, --feature-metrics): dot products
// between two feature sets A (nA, D) and B (nB, D) on the exact-fp32 matrix pipe, with the reduction the metric needs fused
// into the GEMM's epilogue -- the nA x nB matrix never exists.  One mainloop, two epilogues:
//   KSUM   sum_ij (g_ij / D + 1)^3 in fp64 (the cubic kernel of KID)                                        mg_pair_ksum
//   LIST   the KL smallest of  max(|a_i|^2 + |b_j|^2 - 2 g_ij, 0) - shift_j  per row i                      mg_pair_knn (shift = 0)
//                                                                                                           mg_pair_margin (KL = 1, shift = r2B)
// Contracts, limits and the workspace are in include/melo_gan_hip.h.  No floating-point atomics anywhere: per-workgroup
// partials go to a slab that a second launch folds in a fixed order.
#include "common.h"
#include <math.h>

#define ST ((hipStream_t)stream)

namespace {

constexpr int PT = 64;              // tile edge: 64 rows of A x 64 rows of B per workgroup step
constexpr int PKC = 32;             // depth of one LDS chunk of D
constexpr int PLD = PKC + 4;        // LDS row pitch of an operand chunk (floats): 16-byte aligned rows
constexpr int PDL = PT + 4;         // LDS row pitch of the d2 tile: lane (row r, part p) reads bank 4 r + p
constexpr int PTHREADS = 256;       // 4 waves, a 32x32 quadrant of the tile each
constexpr int PTARGET = 1024;       // workgroups wanted per call (4 per CU)
constexpr int PKMAX = 8;
constexpr int MODE_KSUM = 0, MODE_LIST = 1;

// A row tile's column tiles are dealt to `splits` workgroups of `per` consecutive tiles each.
struct PairPlan { int ntA, ntB, splits, per; };
inline PairPlan pair_plan(long nA, long nB) {
    PairPlan P;
    P.ntA = (int)mg_cdiv(nA, PT);
    P.ntB = (int)mg_cdiv(nB, PT);
    long s = mg_cdiv(PTARGET, P.ntA);
    s = s < 1 ? 1 : (s > P.ntB ? P.ntB : s);
    P.per = (int)mg_cdiv(P.ntB, s);
    P.splits = (int)mg_cdiv(P.ntB, P.per);
    return P;
}
inline int list_len(int k) { return k == 1 ? 1 : PKMAX; }
inline size_t norms_bytes(long nA, long nB) { return (size_t)(((nA + nB) * 4 + 15) & ~15L); }
inline size_t pair_work_bytes(long nA, long nB, int k) {
    const PairPlan P = pair_plan(nA, nB);
    const size_t ks = (size_t)P.ntA * P.splits * sizeof(double);
    const size_t ls = (size_t)nA * P.splits * list_len(k) * sizeof(float);
    return norms_bytes(nA, nB) + (ks > ls ? ks : ls);
}

struct PairArgs {
    const float* A;
    const float* B;
    int nA, nB, D;
    int exclude;            // leave i == j out (A == B)
    const float* na;        // |a_i|^2, |b_j|^2 (row_norms_kernel)
    const float* nb;
    const float* shift;     // LIST: subtracted from column j's d2 (r2B), or nullptr
    double* kslab;          // KSUM: [row tile][split]
    float* lslab;           // LIST: [row][split][KL]
    PairPlan P;
};

// v into the ascending list L (its largest entry falls out).  NaN never enters.
template <int KL>
__device__ __forceinline__ void list_insert(float (&L)[KL], float v) {
    if (v < L[KL - 1]) {
        L[KL - 1] = v;
#pragma unroll
        for (int q = KL - 1; q > 0; --q) {
            const float lo = fminf(L[q - 1], L[q]), hi = fmaxf(L[q - 1], L[q]);
            L[q - 1] = lo;
            L[q] = hi;
        }
    }
}

// One k-chunk of one operand tile, global -> registers -> LDS (PFRAG 16-byte pieces per lane): rows >= n and columns >= D
// become zeros.  The two halves are apart so that the next chunk's loads fly while the current one is multiplied.
constexpr int PFRAG = PT * PKC / 4 / PTHREADS;
__device__ __forceinline__ void fetch_chunk(f32x4 (&v)[PFRAG], const float* __restrict__ src, long row0, int n, int D, int k0) {
#pragma unroll
    for (int q = 0; q < PFRAG; ++q) {
        const int idx = threadIdx.x + PTHREADS * q;
        const int r = idx >> 3, c = (idx & 7) * 4;
        v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row0 + r < n && k0 + c < D) v[q] = *reinterpret_cast<const f32x4*>(src + (row0 + r) * D + k0 + c);
    }
}
__device__ __forceinline__ void store_chunk(float (*dst)[PLD], const f32x4 (&v)[PFRAG]) {
#pragma unroll
    for (int q = 0; q < PFRAG; ++q) {
        const int idx = threadIdx.x + PTHREADS * q;
        *reinterpret_cast<f32x4*>(&dst[idx >> 3][(idx & 7) * 4]) = v[q];
    }
}

// The 32x32 quadrant (rows r0.., columns c0..) of As Bs^T added to acc.  Lane (i = lane & 31, h = lane >> 5) feeds
// k = 8 t + 4 h + {0..3} of the chunk: the chain of one output element runs k = 8t+c, 8t+4+c for c = 0..3, t = 0..3 --
// row_norms_kernel walks the same chain, so that a row's distance to its own copy is exactly 0.
__device__ __forceinline__ void mma_chunk(f32x16& acc, const float (*As)[PLD], const float (*Bs)[PLD], int r0, int c0, int lane) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < PKC / 8; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&As[r0 + i][8 * t + 4 * h]);
        const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[c0 + i][8 * t + 4 * h]);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
    }
}

// |x_r|^2 of 32 rows per wave as the diagonal of the rows' own Gram tile, by the main kernel's MFMA chain.
__global__ __launch_bounds__(64) void row_norms_kernel(const float* __restrict__ X, int n, int D, float* __restrict__ out) {
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * 32;
    const bool live = row0 + i < n;
    const float* xr = X + (live ? row0 + i : 0) * D;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = 0; k < D; k += 8) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live && k + 4 * h < D) v = *reinterpret_cast<const f32x4*>(xr + k + 4 * h);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[c], v[c], acc, 0, 0, 0);
    }
    // element (row, col = i) sits in register reg of lane half h with row = (reg & 3) + 8 (reg >> 2) + 4 h
    if (((i >> 2) & 1) == h && live) {
        const int want = (i & 3) + 4 * (i >> 3);
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) v = r == want ? acc[r] : v;
        out[row0 + i] = v;
    }
}

template <int MODE, int KL>
__global__ __launch_bounds__(PTHREADS) void pair_kernel(const PairArgs p) {
    __shared__ __attribute__((aligned(16))) float As[PT][PLD];
    __shared__ __attribute__((aligned(16))) float Bs[PT][PLD];
    __shared__ float d2[MODE == MODE_LIST ? PT : 1][PDL];
    __shared__ float s_na[MODE == MODE_LIST ? PT : 1];
    __shared__ double s_sum[MODE == MODE_KSUM ? PTHREADS : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rt = blockIdx.x / p.P.splits, split = blockIdx.x % p.P.splits;
    const long i0 = (long)rt * PT;
    const int r0 = 32 * (wave & 1), c0 = 32 * (wave >> 1);
    const int lj = c0 + (lane & 31), h = lane >> 5;
    if constexpr (MODE == MODE_LIST) if (tid < PT) s_na[tid] = i0 + tid < p.nA ? p.na[i0 + tid] : 0.f;

    double ksum = 0.0;
    const double inv_d = 1.0 / (double)p.D;
    float best[KL];
#pragma unroll
    for (int q = 0; q < KL; ++q) best[q] = INFINITY;
    const int sr = tid >> 2, sp = tid & 3;      // LIST: this thread scans columns sp, sp + 4, ... of row sr

    const int ct_end = min((split + 1) * p.P.per, p.P.ntB);
    for (int ct = split * p.P.per; ct < ct_end; ++ct) {
        const long j0 = (long)ct * PT;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        f32x4 ra[PFRAG], rb[PFRAG];
        fetch_chunk(ra, p.A, i0, p.nA, p.D, 0);
        fetch_chunk(rb, p.B, j0, p.nB, p.D, 0);
        for (int k0 = 0; k0 < p.D; k0 += PKC) {
            __syncthreads();                    // the previous chunk (and the previous tile's d2 scan) is done with
            store_chunk(As, ra);
            store_chunk(Bs, rb);
            __syncthreads();
            if (k0 + PKC < p.D) {               // the next chunk's loads fly behind this chunk's multiply-adds
                fetch_chunk(ra, p.A, i0, p.nA, p.D, k0 + PKC);
                fetch_chunk(rb, p.B, j0, p.nB, p.D, k0 + PKC);
            }
            mma_chunk(acc, As, Bs, r0, c0, lane);
        }
        const long gj = j0 + lj;
        const bool col_ok = gj < p.nB;
        if constexpr (MODE == MODE_KSUM) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long gi = i0 + r0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const double v = (double)acc[r] * inv_d + 1.0;
                if (col_ok && gi < p.nA && !(p.exclude && gi == gj)) ksum += v * v * v;
            }
        } else {
            const float nbj = col_ok ? p.nb[gj] : 0.f;
            const float sh = (col_ok && p.shift) ? p.shift[gj] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int li = r0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                float v = fmaxf(s_na[li] + nbj - 2.f * acc[r], 0.f) - sh;
                if (!col_ok || (p.exclude && i0 + li == gj)) v = INFINITY;      // never a zero-filled row's distance
                d2[li][lj] = v;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < PT / 4; ++c) list_insert<KL>(best, d2[sr][sp + 4 * c]);
        }
    }

    if constexpr (MODE == MODE_KSUM) {
        s_sum[tid] = ksum;
        __syncthreads();
        for (int s = PTHREADS / 2; s > 0; s >>= 1) {
            if (tid < s) s_sum[tid] += s_sum[tid + s];
            __syncthreads();
        }
        if (tid == 0) p.kslab[blockIdx.x] = s_sum[0];
    } else {
        __syncthreads();                        // the last scan is over: d2 becomes the four part lists of every row
        float* lists = &d2[0][0];               // [row][part][KL]: 64 * 4 * KL <= 2048 floats
#pragma unroll
        for (int q = 0; q < KL; ++q) lists[(sr * 4 + sp) * KL + q] = best[q];
        __syncthreads();
        if (sp == 0 && i0 + sr < p.nA) {
            for (int o = 1; o < 4; ++o)
#pragma unroll
                for (int q = 0; q < KL; ++q) list_insert<KL>(best, lists[(sr * 4 + o) * KL + q]);
            float* dst = p.lslab + ((i0 + sr) * p.P.splits + split) * KL;
#pragma unroll
            for (int q = 0; q < KL; ++q) dst[q] = best[q];
        }
    }
}

// The fixed-order fold of KSUM: one workgroup, lane t adds entries t, t + 256, ..., then a fixed tree.
__global__ __launch_bounds__(PTHREADS) void ksum_fold_kernel(const double* __restrict__ slab, long n, double* __restrict__ out) {
    __shared__ double s_sum[PTHREADS];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += PTHREADS) s += slab[i];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    for (int st = PTHREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_sum[threadIdx.x] += s_sum[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s_sum[0];
}

// The fold of LIST: one lane per row merges its `splits` lists (entries may be +inf) and writes the k smallest, ascending.
template <int KL>
__global__ __launch_bounds__(PTHREADS) void list_fold_kernel(const float* __restrict__ slab, int nA, int splits, int k,
                                                             float* __restrict__ out) {
    const long i = (long)blockIdx.x * PTHREADS + threadIdx.x;
    if (i >= nA) return;
    float best[KL];
#pragma unroll
    for (int q = 0; q < KL; ++q) best[q] = INFINITY;
    const float* src = slab + i * splits * KL;
    for (int s = 0; s < splits * KL; ++s) list_insert<KL>(best, src[s]);
#pragma unroll
    for (int q = 0; q < KL; ++q)
        if (q < k) out[i * k + q] = best[q];
}

__global__ void scatter_rows_cursor_kernel(const float* __restrict__ src, int width, float* __restrict__ dst, long dst_rows,
                                           const unsigned long long* __restrict__ counter,
                                           const unsigned long long* __restrict__ base, int rows) {
    const unsigned long long pos = (counter[0] - base[0]) * (unsigned long long)rows + blockIdx.x;
    if (pos >= (unsigned long long)dst_rows) return;        // the padded tail of the last batch falls off the end
    const float* s = src + (long)blockIdx.x * width;
    float* d = dst + (long)pos * width;
    for (int c = threadIdx.x; c < width; c += blockDim.x) d[c] = s[c];
}

// ---------------- host ----------------
int check_sets(const char* who, const float* A, long nA, const float* B, long nB, int D, const void* out, const void* work) {
    MG_CHECK_ARG(A && B && out && work, "%s: null A / B / out / work", who);
    MG_CHECK_ARG((((uintptr_t)A | (uintptr_t)B | (uintptr_t)work) & 15) == 0, "%s: A, B and work must be 16-byte aligned", who);
    MG_CHECK_ARG(D >= 4 && D <= 1024 && D % 4 == 0, "%s: D must be a multiple of 4 in 4..1024 (16-byte loads)", who);
    MG_CHECK_ARG(nA >= 1 && nA <= (1L << 20) && nB >= 1 && nB <= (1L << 20), "%s: 1..2^20 rows on each side", who);
    return MG_OK;
}
int check_work(const char* who, long nA, long nB, int k, size_t work_bytes) {
    const size_t need = pair_work_bytes(nA, nB, k);
    if (work_bytes < need) {
        mg_set_error("%s: workspace of %zu bytes, %zu needed (mg_pair_workspace_bytes)", who, work_bytes, need);
        return MG_EWORK;
    }
    return MG_OK;
}
int launch_norms(const float* A, int nA, const float* B, int nB, int D, float* na, float* nb, hipStream_t s) {
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)mg_cdiv(nA, 32)), dim3(64), 0, s, A, nA, D, na);
    MG_CHECK_LAUNCH("pair_row_norms");
    if (nb == na) return MG_OK;             // a set against itself: one vector serves both sides
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)mg_cdiv(nB, 32)), dim3(64), 0, s, B, nB, D, nb);
    MG_CHECK_LAUNCH("pair_row_norms");
    return MG_OK;
}
// mg_pair_knn and mg_pair_margin behind their argument checks
int pair_list(const float* A, int nA, const float* B, int nB, int D, int exclude, int k, const float* shift, float* out, void* work,
              hipStream_t s) {
    PairArgs p = {};
    p.A = A; p.B = B; p.nA = nA; p.nB = nB; p.D = D; p.exclude = exclude; p.shift = shift;
    p.P = pair_plan(nA, nB);
    float* na = static_cast<float*>(work);
    float* nb = (A == B && nA == nB) ? na : na + nA;
    p.na = na; p.nb = nb;
    p.lslab = reinterpret_cast<float*>(static_cast<char*>(work) + norms_bytes(nA, nB));
    const int rc = launch_norms(A, nA, B, nB, D, na, nb, s);
    if (rc != MG_OK) return rc;
    const dim3 grid((unsigned)(p.P.ntA * p.P.splits)), fold((unsigned)mg_cdiv(nA, PTHREADS));
    if (list_len(k) == 1) {
        hipLaunchKernelGGL((pair_kernel<MODE_LIST, 1>), grid, dim3(PTHREADS), 0, s, p);
        MG_CHECK_LAUNCH("pair_list");
        hipLaunchKernelGGL(list_fold_kernel<1>, fold, dim3(PTHREADS), 0, s, (const float*)p.lslab, nA, p.P.splits, k, out);
    } else {
        hipLaunchKernelGGL((pair_kernel<MODE_LIST, PKMAX>), grid, dim3(PTHREADS), 0, s, p);
        MG_CHECK_LAUNCH("pair_list");
        hipLaunchKernelGGL(list_fold_kernel<PKMAX>, fold, dim3(PTHREADS), 0, s, (const float*)p.lslab, nA, p.P.splits, k, out);
    }
    MG_CHECK_LAUNCH("pair_list_fold");
    return MG_OK;
}

}  // namespace

extern "C" {

size_t mg_pair_workspace_bytes(long nA, long nB, int D, int k) {
    if (nA < 1 || nA > (1L << 20) || nB < 1 || nB > (1L << 20) || D < 4 || D > 1024 || D % 4 || k < 1 || k > PKMAX) return 0;
    return pair_work_bytes(nA, nB, k);
}

int mg_pair_ksum(const float* A, long nA, const float* B, long nB, int D, int exclude_diag, double* out, void* work,
                 size_t work_bytes, mg_stream_t stream) {
    int rc = check_sets("mg_pair_ksum", A, nA, B, nB, D, out, work);
    if (rc != MG_OK) return rc;
    MG_CHECK_ARG(((uintptr_t)out & 7) == 0, "mg_pair_ksum: out must be 8-byte aligned");
    MG_CHECK_ARG(!exclude_diag || (A == B && nA == nB), "mg_pair_ksum: exclude_diag needs A == B and nA == nB");
    if ((rc = check_work("mg_pair_ksum", nA, nB, 1, work_bytes)) != MG_OK) return rc;
    PairArgs p = {};
    p.A = A; p.B = B; p.nA = (int)nA; p.nB = (int)nB; p.D = D; p.exclude = exclude_diag ? 1 : 0;
    p.P = pair_plan(nA, nB);
    p.kslab = reinterpret_cast<double*>(static_cast<char*>(work) + norms_bytes(nA, nB));
    const long parts = (long)p.P.ntA * p.P.splits;
    hipLaunchKernelGGL((pair_kernel<MODE_KSUM, 1>), dim3((unsigned)parts), dim3(PTHREADS), 0, ST, p);
    MG_CHECK_LAUNCH("pair_ksum");
    hipLaunchKernelGGL(ksum_fold_kernel, dim3(1), dim3(PTHREADS), 0, ST, (const double*)p.kslab, parts, out);
    MG_CHECK_LAUNCH("pair_ksum_fold");
    return MG_OK;
}

int mg_pair_knn(const float* A, long nA, const float* B, long nB, int D, int exclude_self, int k, float* out, void* work,
                size_t work_bytes, mg_stream_t stream) {
    int rc = check_sets("mg_pair_knn", A, nA, B, nB, D, out, work);
    if (rc != MG_OK) return rc;
    MG_CHECK_ARG(!exclude_self || (A == B && nA == nB), "mg_pair_knn: exclude_self needs A == B and nA == nB");
    MG_CHECK_ARG(k >= 1 && k <= PKMAX, "mg_pair_knn: k must be in 1..%d", PKMAX);
    MG_CHECK_ARG(((uintptr_t)out & 3) == 0, "mg_pair_knn: out must be 4-byte aligned");
    MG_CHECK_ARG(k <= nB - (exclude_self ? 1 : 0), "mg_pair_knn: k = %d neighbours asked of %ld candidates", k,
                 nB - (exclude_self ? 1 : 0));
    if ((rc = check_work("mg_pair_knn", nA, nB, k, work_bytes)) != MG_OK) return rc;
    return pair_list(A, (int)nA, B, (int)nB, D, exclude_self ? 1 : 0, k, nullptr, out, work, ST);
}

int mg_pair_margin(const float* A, long nA, const float* B, long nB, int D, const float* r2B, float* out, void* work,
                   size_t work_bytes, mg_stream_t stream) {
    int rc = check_sets("mg_pair_margin", A, nA, B, nB, D, out, work);
    if (rc != MG_OK) return rc;
    MG_CHECK_ARG(r2B != nullptr, "mg_pair_margin: null r2B");
    MG_CHECK_ARG((((uintptr_t)r2B | (uintptr_t)out) & 3) == 0, "mg_pair_margin: r2B and out must be 4-byte aligned");
    if ((rc = check_work("mg_pair_margin", nA, nB, 1, work_bytes)) != MG_OK) return rc;
    return pair_list(A, (int)nA, B, (int)nB, D, 0, 1, r2B, out, work, ST);
}

int mg_scatter_rows_cursor(const float* src, int rows, int width, float* dst, long dst_rows, const uint64_t* counter,
                           const uint64_t* base, mg_stream_t stream) {
    MG_CHECK_ARG(src && dst && counter && base, "mg_scatter_rows_cursor: null src / dst / counter / base");
    MG_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "mg_scatter_rows_cursor: src and dst must be 4-byte aligned");
    MG_CHECK_ARG(rows >= 1 && rows <= 65535 && width >= 1 && dst_rows >= 1,
                 "mg_scatter_rows_cursor: 1..65535 rows, a positive width and destination");
    hipLaunchKernelGGL(scatter_rows_cursor_kernel, dim3((unsigned)rows), dim3(256), 0, ST, src, width, dst, dst_rows,
                       (const unsigned long long*)counter, (const unsigned long long*)base, rows);
    MG_CHECK_LAUNCH("scatter_rows_cursor");
    return MG_OK;
}

}  // extern "C"
