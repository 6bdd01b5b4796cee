// Exact t-SNE (van der Maaten & Hinton 2008, with scikit-learn's gradient-descent schedule) of a feature set on the device:
// melo_gan_amd/gan/tsne.py and evaluate --tsne.  Two families:
//   mg_tsne_affinities   X (N, D) -> the symmetric joint P (N, N): squared distances by pair_metrics.hip's formula and
//                        multiply-add chain, a per-row solve for the Gaussian precision beta_i at the wanted perplexity with
//                        the row of d2 in LDS, then P = (P_cond + P_cond^T) / 2N written so that P_ij and P_ji hold the same bits
//   mg_tsne_step         one descent iteration = two launches: forces (attraction, repulsion and the normaliser's partials per
//                        row tile x column run, to a slab) and fold + update (Z folded by every workgroup in the same fixed
//                        order, then gradient, gains, momentum update and Y)
// Contracts, limits and the workspace are in include/melo_gan_hip.h.  Sums are formed in fp64 by fixed lane trees; no
// floating-point atomics, no signalling between workgroups: workgroups of one launch write disjoint memory only.
#include "common.h"
#include <math.h>

#define ST ((hipStream_t)stream)

namespace {

constexpr long TS_MAX_N = 16384;        // dense P is 1 GiB there
constexpr int TT = 64;                  // d2 / symmetrise tile edge
constexpr int TKC = 32;                 // depth of one LDS chunk of D
constexpr int TLD = TKC + 4;            // LDS row pitch of an operand chunk (floats): 16-byte aligned rows
constexpr int TTHREADS = 256;
constexpr int FROWS = 16;               // forces: rows per workgroup, 4 per wave (8 per wave: 188 VGPRs, and measured slower)
constexpr int FQ = FROWS / 4;
constexpr int FCOLS = 64;               // forces: one lane per column of a column tile
constexpr int FTARGET = 1024;           // forces: workgroups wanted per launch (4 per CU)
constexpr int MAX_DOUBLINGS = 100;      // the bracket's upper end stays finite in fp32
constexpr int BISECTIONS = 64;

// A row tile's column tiles are dealt to `splits` workgroups of `per` consecutive tiles each (pair_plan's rule).
struct ForcePlan { int ntR, ntC, splits, per; };
inline ForcePlan force_plan(long N) {
    ForcePlan P;
    P.ntR = (int)mg_cdiv(N, FROWS);
    P.ntC = (int)mg_cdiv(N, FCOLS);
    long s = mg_cdiv(FTARGET, P.ntR);
    s = s < 1 ? 1 : (s > P.ntC ? P.ntC : s);
    P.per = (int)mg_cdiv(P.ntC, s);
    P.splits = (int)mg_cdiv(P.ntC, P.per);
    return P;
}
// step workspace: [row][split][4] attraction x, y, repulsion x, y | [workgroup] z | [workgroup] sum p (log p - log w)
inline size_t step_bytes(long N) {
    const ForcePlan P = force_plan(N);
    return ((size_t)N * P.splits * 4 + 2 * (size_t)P.ntR * P.splits) * sizeof(double);
}
inline size_t work_bytes_for(long N) {
    const size_t norms = (size_t)((N * 4 + 15) & ~15L), step = step_bytes(N);
    return norms > step ? norms : step;
}

// ---------------- fixed-order reductions ----------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);       // a butterfly: every lane ends with the same bits
    return v;
}
// The sum of v over the workgroup's 256 lanes, the same bits in every lane.  s: 4 doubles of LDS; two barriers.
__device__ __forceinline__ double block_sum(double v, double* s) {
    v = wave_sum(v);
    __syncthreads();                    // the previous use of s is over
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// ---------------- affinities ----------------
// |x_r|^2 of 32 rows per wave as the diagonal of the rows' own Gram tile, by d2_kernel's MFMA chain (pair_metrics.hip's
// row_norms_kernel with element-wise guarded loads: D need not be a multiple of 4 here).
__global__ __launch_bounds__(64) void ts_norms_kernel(const float* __restrict__ X, int n, int D, float* __restrict__ out) {
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * 32;
    const bool live = row0 + i < n;
    const float* xr = X + (live ? row0 + i : 0) * D;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = 0; k < D; k += 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kk = k + 4 * h + c;
            const float v = (live && kk < D) ? xr[kk] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v, v, acc, 0, 0, 0);
        }
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

__device__ __forceinline__ void ts_load_chunk(float (*dst)[TLD], const float* __restrict__ X, long row0, int n, int D, int k0) {
#pragma unroll
    for (int q = 0; q < TT * TKC / TTHREADS; ++q) {
        const int idx = threadIdx.x + TTHREADS * q;
        const int r = idx >> 5, c = idx & 31;
        dst[r][c] = (row0 + r < n && k0 + c < D) ? X[(row0 + r) * D + k0 + c] : 0.f;
    }
}

// d2_ij = max(|x_i|^2 + |x_j|^2 - 2 x_i . x_j, 0), 0 on the diagonal, one 64x64 tile of the (N, N) output per workgroup:
// pair_kernel's mainloop (a 32x32 quadrant per wave on the exact-fp32 MFMA, the chain of one element running over k in
// ts_norms_kernel's order, so that identical rows are exactly 0 apart).
__global__ __launch_bounds__(TTHREADS) void ts_d2_kernel(const float* __restrict__ X, int N, int D, const float* __restrict__ norms,
                                                         float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float As[TT][TLD];
    __shared__ __attribute__((aligned(16))) float Bs[TT][TLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long i0 = (long)blockIdx.y * TT, j0 = (long)blockIdx.x * TT;
    const int r0 = 32 * (wave & 1), c0 = 32 * (wave >> 1);
    const int li = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < D; k0 += TKC) {
        __syncthreads();                // the previous chunk is done with
        ts_load_chunk(As, X, i0, N, D, k0);
        ts_load_chunk(Bs, X, j0, N, D, k0);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TKC / 8; ++t) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&As[r0 + li][8 * t + 4 * h]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[c0 + li][8 * t + 4 * h]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
        }
    }
    const long gj = j0 + c0 + li;
    if (gj >= N) return;
    const float nj = norms[gj];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long gi = i0 + r0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (gi < N) out[gi * N + gj] = gi == gj ? 0.f : fmaxf(norms[gi] + nj - 2.f * acc[r], 0.f);
    }
}

// One workgroup per row i: the row of d2 comes into LDS less its minimum over j != i, beta_i is bracketed by doubling from 1
// and bisected a fixed number of steps so that the entropy of p_j|i ~ exp(-beta_i d_j), j != i, is log(perplexity), and the
// row is overwritten with p_j|i (0 at j = i).  The sums of one entropy evaluation are fp64.
__global__ __launch_bounds__(TTHREADS) void ts_cond_kernel(float* __restrict__ P, int N, double target, float* __restrict__ beta_out) {
    extern __shared__ float s_d[];
    __shared__ double s_red[4];
    __shared__ float s_min[4];
    const int tid = threadIdx.x, i = blockIdx.x;
    float* row = P + (long)i * N;
    float mn = INFINITY;
    for (int j = tid; j < N; j += TTHREADS) {
        const float v = row[j];
        s_d[j] = v;
        if (j != i) mn = fminf(mn, v);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, 64));
    if ((tid & 63) == 0) s_min[tid >> 6] = mn;
    __syncthreads();
    mn = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    for (int j = tid; j < N; j += TTHREADS) s_d[j] -= mn;        // a lane re-reads its own entries only
    double s0 = 0.0;

    auto entropy = [&](float beta) -> double {
        double a = 0.0, b = 0.0;
        for (int j = tid; j < N; j += TTHREADS) {
            const float d = s_d[j];
            const float p = j == i ? 0.f : expf(-beta * d);
            a += (double)p;
            b += (double)d * (double)p;
        }
        s0 = block_sum(a, s_red);
        const double s1 = block_sum(b, s_red);
        return log(s0) + (double)beta * s1 / s0;
    };

    float lo = 0.f, hi = 1.f;
    for (int it = 0; it < MAX_DOUBLINGS; ++it) {        // every lane holds the same entropy: the branches are uniform
        if (entropy(hi) <= target) break;
        lo = hi;
        hi *= 2.f;
    }
    for (int it = 0; it < BISECTIONS; ++it) {
        const float mid = 0.5f * (lo + hi);
        if (entropy(mid) > target) lo = mid; else hi = mid;
    }
    const float beta = 0.5f * (lo + hi);
    entropy(beta);
    for (int j = tid; j < N; j += TTHREADS) row[j] = j == i ? 0.f : (float)((double)expf(-beta * s_d[j]) / s0);
    if (beta_out && tid == 0) beta_out[i] = beta;
}

// P = (C + C^T) / 2N in place.  The workgroup of tile pair (I <= J) reads both tiles into LDS and writes both: element
// (i, j) and element (j, i) are the same sum of the same two operands in the same order, so they hold the same bits.
__global__ __launch_bounds__(TTHREADS) void ts_symm_kernel(float* __restrict__ P, int N) {
    __shared__ float sa[TT][TT + 1];
    __shared__ float sb[TT][TT + 1];
    const int I = blockIdx.y, J = blockIdx.x;
    if (J < I) return;
    const long i0 = (long)I * TT, j0 = (long)J * TT;
    const int c = threadIdx.x & 63, rq = threadIdx.x >> 6;
    for (int r = rq; r < TT; r += 4) {
        sa[r][c] = (i0 + r < N && j0 + c < N) ? P[(i0 + r) * N + j0 + c] : 0.f;
        sb[r][c] = (j0 + r < N && i0 + c < N) ? P[(j0 + r) * N + i0 + c] : 0.f;
    }
    __syncthreads();
    const float two_n = 2.f * (float)N;
    for (int r = rq; r < TT; r += 4) {
        if (i0 + r < N && j0 + c < N) P[(i0 + r) * N + j0 + c] = (sa[r][c] + sb[c][r]) / two_n;
        if (J != I && j0 + r < N && i0 + c < N) P[(j0 + r) * N + i0 + c] = (sa[c][r] + sb[r][c]) / two_n;
    }
}

// ---------------- one descent iteration ----------------
struct ForceArgs {
    const float* P;
    const float* Y;         // (N, 2)
    int N;
    double* slab;           // [row][split][4]
    double* zslab;          // [workgroup]
    double* klslab;         // [workgroup] (KL instantiation)
    ForcePlan plan;
};

// Launch 1.  A workgroup owns 16 rows (4 per wave) and a run of 64-column tiles; lane l of a wave owns column l of the
// current tile.  Per row it accumulates in fp64, with w = 1 / (1 + |y_i - y_j|^2) and j != i:
//   attr = sum_j p_ij w_ij (y_i - y_j),  rep = sum_j w_ij^2 (y_i - y_j),  z = sum_j w_ij    [KL: sum_j p_ij (log p_ij - log w_ij)]
// then a butterfly over the wave's lanes; attr and rep go to the row's slab entry, z (and the KL sum) of the workgroup's
// rows, added in a fixed order, to the workgroup's own entry.
template <bool KL>
__global__ __launch_bounds__(TTHREADS) void ts_forces_kernel(const ForceArgs a) {
    __shared__ double s_z[4], s_kl[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rt = blockIdx.x / a.plan.splits, split = blockIdx.x % a.plan.splits;
    const int N = a.N;
    const long i0 = (long)rt * FROWS + wave * FQ;
    float yix[FQ], yiy[FQ];
    double ax[FQ], ay[FQ], rx[FQ], ry[FQ], z[FQ], kl[FQ];
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        const long i = i0 + q < N ? i0 + q : 0;
        yix[q] = a.Y[2 * i];
        yiy[q] = a.Y[2 * i + 1];
        ax[q] = ay[q] = rx[q] = ry[q] = z[q] = kl[q] = 0.0;
    }
    const int ct_end = min((split + 1) * a.plan.per, a.plan.ntC);
    for (int ct = split * a.plan.per; ct < ct_end; ++ct) {
        const long j = (long)ct * FCOLS + lane;
        const bool col_ok = j < N;
        const float yjx = col_ok ? a.Y[2 * j] : 0.f, yjy = col_ok ? a.Y[2 * j + 1] : 0.f;
        float p[FQ];
#pragma unroll
        for (int q = 0; q < FQ; ++q) p[q] = (col_ok && i0 + q < N) ? a.P[(i0 + q) * N + j] : 0.f;     // all in flight
#pragma unroll
        for (int q = 0; q < FQ; ++q) {
            const bool ok = col_ok && i0 + q < N && i0 + q != j;
            const float dx = yix[q] - yjx, dy = yiy[q] - yjy;
            const float w = ok ? 1.f / (1.f + (dx * dx + dy * dy)) : 0.f;
            const float pw = p[q] * w, w2 = w * w;
            ax[q] += (double)(pw * dx);
            ay[q] += (double)(pw * dy);
            rx[q] += (double)(w2 * dx);
            ry[q] += (double)(w2 * dy);
            z[q] += (double)w;
            if constexpr (KL)
                if (ok && p[q] > 0.f) kl[q] += (double)p[q] * (log((double)p[q]) - log((double)w));
        }
    }
    double zw = 0.0, klw = 0.0;
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        const double sax = wave_sum(ax[q]), say = wave_sum(ay[q]), srx = wave_sum(rx[q]), sry = wave_sum(ry[q]);
        zw += wave_sum(z[q]);
        if constexpr (KL) klw += wave_sum(kl[q]);
        if (lane == 0 && i0 + q < N) {
            double* dst = a.slab + ((i0 + q) * a.plan.splits + split) * 4;
            dst[0] = sax; dst[1] = say; dst[2] = srx; dst[3] = sry;
        }
    }
    if (lane == 0) { s_z[wave] = zw; s_kl[wave] = klw; }
    __syncthreads();
    if (tid == 0) {
        a.zslab[blockIdx.x] = (s_z[0] + s_z[1]) + (s_z[2] + s_z[3]);
        if constexpr (KL) a.klslab[blockIdx.x] = (s_kl[0] + s_kl[1]) + (s_kl[2] + s_kl[3]);
    }
}

struct UpdateArgs {
    float* Y;
    float* update;
    float* gains;
    float* grad;            // nullable (N, 2)
    double* trace;          // nullable: records of 4 doubles (KL, |grad|_2, Z, sum p (log p - log w))
    unsigned long long* cursor;     // nullable: the record index, advanced by one
    long trace_cap;
    int N;
    float ee, momentum, lr;
    const double* slab;
    const double* zslab;
    const double* klslab;
    int splits, nwg;
};

__device__ __forceinline__ void fold_row(const UpdateArgs& u, long i, double Z, double& gx, double& gy) {
    const double* src = u.slab + i * u.splits * 4;
    double a0 = 0.0, a1 = 0.0, r0 = 0.0, r1 = 0.0;
    for (int s = 0; s < u.splits; ++s) {
        a0 += src[4 * s]; a1 += src[4 * s + 1]; r0 += src[4 * s + 2]; r1 += src[4 * s + 3];
    }
    gx = 4.0 * ((double)u.ee * a0 - r0 / Z);
    gy = 4.0 * ((double)u.ee * a1 - r1 / Z);
}

// Launch 2.  Every workgroup folds the z partials in the same fixed order (lane t adds entries t, t + 256, ..., then the
// lane tree), so Z is identical everywhere without communication; a lane then folds its row's attr / rep partials over the
// runs in order, forms grad = 4 (ee attr - rep / Z) and applies scikit-learn's _gradient_descent update.  With a trace,
// workgroup 0 also folds every row's gradient into |grad|_2 and the KL partials into KL = sum p log p - sum p log w + log Z.
__global__ __launch_bounds__(TTHREADS) void ts_update_kernel(const UpdateArgs u) {
    __shared__ double s_red[4];
    const int tid = threadIdx.x;
    double zs = 0.0;
    for (int k = tid; k < u.nwg; k += TTHREADS) zs += u.zslab[k];
    const double Z = block_sum(zs, s_red);
    const long i = (long)blockIdx.x * TTHREADS + tid;
    if (i < u.N) {
        double gx, gy;
        fold_row(u, i, Z, gx, gy);
        const float g[2] = {(float)gx, (float)gy};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const float up = u.update[2 * i + d];
            float gn = u.gains[2 * i + d];
            gn = up * g[d] < 0.f ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            const float nu = u.momentum * up - u.lr * gn * g[d];
            u.gains[2 * i + d] = gn;
            u.update[2 * i + d] = nu;
            u.Y[2 * i + d] += nu;
            if (u.grad) u.grad[2 * i + d] = g[d];
        }
    }
    if (u.trace && blockIdx.x == 0) {
        double g2 = 0.0, ks = 0.0;
        for (long r = tid; r < u.N; r += TTHREADS) {
            double gx, gy;
            fold_row(u, r, Z, gx, gy);
            g2 += gx * gx + gy * gy;
        }
        for (int k = tid; k < u.nwg; k += TTHREADS) ks += u.klslab[k];
        g2 = block_sum(g2, s_red);
        ks = block_sum(ks, s_red);
        if (tid == 0) {
            const unsigned long long at = u.cursor ? u.cursor[0] : 0ull;
            if (at < (unsigned long long)u.trace_cap) {
                double* rec = u.trace + 4 * at;
                rec[0] = ks + log(Z);
                rec[1] = sqrt(g2);
                rec[2] = Z;
                rec[3] = ks;
            }
            if (u.cursor) u.cursor[0] = at + 1;
        }
    }
}

// ts_cond_kernel's dynamic LDS (the row of d2: up to 64 KiB, beside its few static bytes) needs the opt-in above 64 KiB in
// total; made once per device, as mg_lds_optin does for the tile kernels (whose 160 KiB leave no room for static LDS).
std::atomic<uint64_t> g_cond_lds_done{0};
int cond_lds_optin() {
    int dev = 0;
    MG_HIP(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? 1ull << dev : 0;
    if (g_cond_lds_done.load(std::memory_order_relaxed) & bit) return MG_OK;
    MG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ts_cond_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(TS_MAX_N * sizeof(float))));
    g_cond_lds_done.fetch_or(bit, std::memory_order_relaxed);
    return MG_OK;
}

}  // namespace

extern "C" {

size_t mg_tsne_workspace_bytes(long N) {
    if (N < 4 || N > TS_MAX_N) return 0;
    return work_bytes_for(N);
}

int mg_tsne_affinities(const float* X, long N, int D, float perplexity, float* P, float* beta, void* work, size_t work_bytes,
                       mg_stream_t stream) {
    MG_CHECK_ARG(X && P && work, "mg_tsne_affinities: null X / P / work");
    MG_CHECK_ARG(N >= 4 && N <= TS_MAX_N, "mg_tsne_affinities: N = %ld: 4..%ld rows (dense P)", N, TS_MAX_N);
    MG_CHECK_ARG(D >= 1 && D <= (1 << 20), "mg_tsne_affinities: D = %d: 1..2^20", D);
    MG_CHECK_ARG(perplexity >= 1.f && perplexity < (float)(N - 1), "mg_tsne_affinities: perplexity %g: 1 <= perplexity < N - 1 = %ld",
                 (double)perplexity, N - 1);
    MG_CHECK_ARG((((uintptr_t)X | (uintptr_t)P | (uintptr_t)work | (uintptr_t)beta) & 3) == 0,
                 "mg_tsne_affinities: X, P, beta and work must be 4-byte aligned");
    const size_t need = work_bytes_for(N);
    if (work_bytes < need) {
        mg_set_error("mg_tsne_affinities: workspace of %zu bytes, %zu needed (mg_tsne_workspace_bytes)", work_bytes, need);
        return MG_EWORK;
    }
    const int n = (int)N;
    float* norms = static_cast<float*>(work);
    const unsigned nt = (unsigned)mg_cdiv(N, TT);
    hipLaunchKernelGGL(ts_norms_kernel, dim3((unsigned)mg_cdiv(N, 32)), dim3(64), 0, ST, X, n, D, norms);
    MG_CHECK_LAUNCH("tsne_norms");
    hipLaunchKernelGGL(ts_d2_kernel, dim3(nt, nt), dim3(TTHREADS), 0, ST, X, n, D, (const float*)norms, P);
    MG_CHECK_LAUNCH("tsne_d2");
    const int rc = cond_lds_optin();
    if (rc != MG_OK) return rc;
    hipLaunchKernelGGL(ts_cond_kernel, dim3((unsigned)N), dim3(TTHREADS), (size_t)N * sizeof(float), ST, P, n,
                       log((double)perplexity), beta);
    MG_CHECK_LAUNCH("tsne_cond");
    hipLaunchKernelGGL(ts_symm_kernel, dim3(nt, nt), dim3(TTHREADS), 0, ST, P, n);
    MG_CHECK_LAUNCH("tsne_symm");
    return MG_OK;
}

int mg_tsne_step(const float* P, long N, float* Y, float* update, float* gains, float exaggeration, float momentum, float lr,
                 float* grad, double* trace, uint64_t* trace_cursor, long trace_cap, void* work, size_t work_bytes,
                 mg_stream_t stream) {
    MG_CHECK_ARG(P && Y && update && gains && work, "mg_tsne_step: null P / Y / update / gains / work");
    MG_CHECK_ARG(N >= 4 && N <= TS_MAX_N, "mg_tsne_step: N = %ld: 4..%ld rows (dense P)", N, TS_MAX_N);
    MG_CHECK_ARG((((uintptr_t)P | (uintptr_t)Y | (uintptr_t)update | (uintptr_t)gains | (uintptr_t)grad) & 3) == 0,
                 "mg_tsne_step: P, Y, update, gains and grad must be 4-byte aligned");
    MG_CHECK_ARG((((uintptr_t)work | (uintptr_t)trace | (uintptr_t)trace_cursor) & 7) == 0,
                 "mg_tsne_step: work, trace and trace_cursor must be 8-byte aligned");
    MG_CHECK_ARG(exaggeration > 0.f && momentum >= 0.f && momentum < 1.f && lr > 0.f,
                 "mg_tsne_step: exaggeration and lr must be positive, momentum in [0, 1)");
    MG_CHECK_ARG(!trace_cursor || trace, "mg_tsne_step: a trace cursor without a trace");
    MG_CHECK_ARG(!trace || trace_cap >= 1, "mg_tsne_step: a trace of %ld records", trace_cap);
    const size_t need = work_bytes_for(N);
    if (work_bytes < need) {
        mg_set_error("mg_tsne_step: workspace of %zu bytes, %zu needed (mg_tsne_workspace_bytes)", work_bytes, need);
        return MG_EWORK;
    }
    ForceArgs f = {};
    f.P = P; f.Y = Y; f.N = (int)N; f.plan = force_plan(N);
    const int nwg = f.plan.ntR * f.plan.splits;
    f.slab = static_cast<double*>(work);
    f.zslab = f.slab + (size_t)N * f.plan.splits * 4;
    f.klslab = f.zslab + nwg;
    if (trace) hipLaunchKernelGGL(ts_forces_kernel<true>, dim3((unsigned)nwg), dim3(TTHREADS), 0, ST, f);
    else hipLaunchKernelGGL(ts_forces_kernel<false>, dim3((unsigned)nwg), dim3(TTHREADS), 0, ST, f);
    MG_CHECK_LAUNCH("tsne_forces");
    UpdateArgs u = {};
    u.Y = Y; u.update = update; u.gains = gains; u.grad = grad; u.trace = trace;
    u.cursor = reinterpret_cast<unsigned long long*>(trace_cursor); u.trace_cap = trace_cap;
    u.N = (int)N; u.ee = exaggeration; u.momentum = momentum; u.lr = lr;
    u.slab = f.slab; u.zslab = f.zslab; u.klslab = f.klslab; u.splits = f.plan.splits; u.nwg = nwg;
    hipLaunchKernelGGL(ts_update_kernel, dim3((unsigned)mg_cdiv(N, TTHREADS)), dim3(TTHREADS), 0, ST, u);
    MG_CHECK_LAUNCH("tsne_update");
    return MG_OK;
}

}  // extern "C"
