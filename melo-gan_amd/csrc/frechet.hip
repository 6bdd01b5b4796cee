// Second moments, a symmetric eigensolver and the Frechet distance in fp64 (melo_gan_amd/gan/evaluate.py, --feature-metrics
// --frechet): what the pair kernels cannot give, because it is not a function of pairwise dot products.
//   mg_feat_moments    mean (D) and unbiased covariance (D, D) of n fp32 rows, two passes, the rank-n update on
//                      v_mfma_f64_16x16x4_f64
//   mg_sym_eig         batched cyclic Jacobi (two-sided, round-robin ordering), one workgroup per matrix
//   mg_frechet_pairs   eig of every set -> B = H^T S_b H per pair -> eigenvalues of every B -> distances and spectra
// Contracts, limits and the workspace are in include/melo_gan_hip.h.  No floating-point atomics anywhere: partials go to a
// slab that a second launch folds in a fixed order, and every reduction inside a workgroup is a fixed tree.
#include "common.h"
#include <math.h>

#define ST ((hipStream_t)stream)

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FD_MAX_D = 256;
constexpr long FD_MAX_ROWS = 1L << 20;
constexpr int FD_MAX_BATCH = 4096;          // matrices of one mg_sym_eig call; sets of one mg_frechet_pairs call
constexpr int FD_MAX_PAIRS = 65535;         // grid.z of the batched product
constexpr int MT = 16;                      // tile edge of the covariance and of the product kernels
constexpr int MTHREADS = 256;
constexpr int MEAN_MAX_SPLITS = 256, COV_MAX_SPLITS = 32;
constexpr int EIG_THREADS = 1024;
constexpr int EIG_MAX_SWEEPS = 30;
constexpr double EIG_EPS = 1.1102230246251565e-16;      // 2^-53

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// ---------------- moments ----------------
struct MomentPlan { int msplits, mchunk, csplits, cchunk; };
inline MomentPlan moment_plan(long n) {
    MomentPlan P;
    long s = mg_cdiv(n, 256);
    s = s > MEAN_MAX_SPLITS ? MEAN_MAX_SPLITS : s;
    P.mchunk = (int)mg_cdiv(n, s);
    P.msplits = (int)mg_cdiv(n, P.mchunk);
    s = mg_cdiv(n, 256);
    s = s > COV_MAX_SPLITS ? COV_MAX_SPLITS : s;
    P.cchunk = (int)(mg_cdiv(mg_cdiv(n, s), MT) * MT);      // whole 16-row groups: 4 waves x 4 rows per MFMA
    P.csplits = (int)mg_cdiv(n, P.cchunk);
    return P;
}
inline size_t moment_work_bytes(long n, int D) {
    const MomentPlan P = moment_plan(n);
    return align16((size_t)P.msplits * D * sizeof(double)) + (size_t)P.csplits * D * D * sizeof(double);
}

// column sums of one run of rows: lane c owns column c
__global__ __launch_bounds__(MTHREADS) void mean_partial_kernel(const float* __restrict__ X, long n, int D, int chunk,
                                                                double* __restrict__ part) {
    const int c = threadIdx.x;
    if (c >= D) return;
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    double s = 0.0;
    for (long r = r0; r < r1; ++r) s += (double)X[r * D + c];
    part[(long)blockIdx.x * D + c] = s;
}
__global__ __launch_bounds__(MTHREADS) void mean_fold_kernel(const double* __restrict__ part, int splits, int D, long n,
                                                             double* __restrict__ mean) {
    const int c = threadIdx.x;
    if (c >= D) return;
    double s = 0.0;
    for (int q = 0; q < splits; ++q) s += part[(long)q * D + c];
    mean[c] = s / (double)n;
}

// One 16 x 16 tile (ti <= tj) of sum_r xc_r xc_r^T over one run of rows.  Wave w takes rows 16 g + 4 w + (lane >> 4) of the run:
// lane l feeds A[i = l & 15][k = l >> 4] = xc[row k][i0 + i] and B[k][j = l & 15] = xc[row k][j0 + j]; the result sits at
// col = lane & 15, row = (lane >> 4) + 4 reg.  Rows past the end and columns past D are zero AFTER centring.
__global__ __launch_bounds__(MTHREADS) void cov_partial_kernel(const float* __restrict__ X, long n, int D, int chunk,
                                                               const double* __restrict__ mean, double* __restrict__ part) {
    __shared__ double s_acc[MTHREADS / 64][MT][MT + 1];
    const int nt = (D + MT - 1) / MT;
    const int ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (ti > tj) return;                        // the fold mirrors the upper triangle
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci = ti * MT + (lane & 15), cj = tj * MT + (lane & 15);
    const bool oki = ci < D, okj = cj < D;
    const double mi = oki ? mean[ci] : 0.0, mj = okj ? mean[cj] : 0.0;
    const long r0 = (long)blockIdx.y * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (long g = r0; g < r1; g += MT) {
        const long r = g + 4 * wave + (lane >> 4);
        const bool live = r < r1;
        const double a = (live && oki) ? (double)X[r * D + ci] - mi : 0.0;
        const double b = (live && okj) ? (double)X[r * D + cj] - mj : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s_acc[wave][(lane >> 4) + 4 * q][lane & 15] = acc[q];
    __syncthreads();
    const int row = tid >> 4, col = tid & 15;
    const int gi = ti * MT + row, gj = tj * MT + col;
    if (gi < D && gj < D) {
        double s = s_acc[0][row][col];
#pragma unroll
        for (int w = 1; w < MTHREADS / 64; ++w) s += s_acc[w][row][col];
        part[((long)blockIdx.y * D + gi) * D + gj] = s;
    }
}
__global__ __launch_bounds__(MTHREADS) void cov_fold_kernel(const double* __restrict__ part, int splits, int D, long n,
                                                            double* __restrict__ cov) {
    const int idx = blockIdx.x * MTHREADS + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx % D;
    const int lo = i < j ? i : j, hi = i < j ? j : i;       // both halves from the one upper-triangle partial: exactly symmetric
    double s = 0.0;
    for (int q = 0; q < splits; ++q) s += part[((long)q * D + lo) * D + hi];
    cov[idx] = s / (double)(n - 1);
}

int launch_moments(const float* X, long n, int D, double* mean, double* cov, void* work, hipStream_t s) {
    const MomentPlan P = moment_plan(n);
    double* mpart = static_cast<double*>(work);
    double* cpart = reinterpret_cast<double*>(static_cast<char*>(work) + align16((size_t)P.msplits * D * sizeof(double)));
    hipLaunchKernelGGL(mean_partial_kernel, dim3((unsigned)P.msplits), dim3(MTHREADS), 0, s, X, n, D, P.mchunk, mpart);
    MG_CHECK_LAUNCH("feat_mean_partial");
    hipLaunchKernelGGL(mean_fold_kernel, dim3(1), dim3(MTHREADS), 0, s, (const double*)mpart, P.msplits, D, n, mean);
    MG_CHECK_LAUNCH("feat_mean_fold");
    const int nt = (D + MT - 1) / MT;
    hipLaunchKernelGGL(cov_partial_kernel, dim3((unsigned)(nt * nt), (unsigned)P.csplits), dim3(MTHREADS), 0, s, X, n, D, P.cchunk,
                       (const double*)mean, cpart);
    MG_CHECK_LAUNCH("feat_cov_partial");
    hipLaunchKernelGGL(cov_fold_kernel, dim3((unsigned)mg_cdiv((long)D * D, MTHREADS)), dim3(MTHREADS), 0, s, (const double*)cpart,
                       P.csplits, D, n, cov);
    MG_CHECK_LAUNCH("feat_cov_fold");
    return MG_OK;
}

// ---------------- the eigensolver ----------------
// The working copy is m x m with m = D rounded up to even (D = 1: 2): the extra index is a zero row and column that no
// rotation ever touches, so that every step of the round-robin schedule has m / 2 disjoint pairs.
inline int eig_m(int D) { return D + (D & 1); }
inline size_t eig_work_bytes(int batch, int D) {
    const size_t m = (size_t)eig_m(D);
    return (size_t)batch * 2 * m * m * sizeof(double);
}

// Step `step` (0 .. m - 2) of the round-robin tournament over m players (m even): pair 0 is (m - 1, step), pair i is
// ((step + i) mod (m - 1), (step - i) mod (m - 1)); every index meets every other exactly once per sweep.
__device__ __forceinline__ void eig_pair(int i, int step, int m, int& p, int& q) {
    int a, b;
    if (i == 0) {
        a = m - 1;
        b = step;
    } else {
        a = (step + i) % (m - 1);
        b = (step - i + (m - 1)) % (m - 1);
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// One workgroup diagonalises one matrix in global memory (at D = 256 the matrix and its vectors are 512 KB each: L2, not
// LDS) by J^T A J with J the m / 2 disjoint rotations of a step.  A lane owns whole 2 x 2 blocks (pair a's rows x pair b's
// columns): it reads and writes nothing another lane touches, so a step needs one barrier after the angles and one after the
// update.  The blocks (a, b) and (b, a) run the same instructions on the same numbers: the copy stays exactly symmetric.
__global__ __launch_bounds__(EIG_THREADS) void sym_eig_kernel(const double* __restrict__ A, int D, double* __restrict__ w,
                                                              double* __restrict__ V, int* __restrict__ info,
                                                              double* __restrict__ work) {
    __shared__ double s_red[EIG_THREADS];
    __shared__ double s_c[FD_MAX_D / 2], s_s[FD_MAX_D / 2], s_t[FD_MAX_D / 2];
    __shared__ int s_p[FD_MAX_D / 2], s_q[FD_MAX_D / 2], s_on[FD_MAX_D / 2], s_perm[FD_MAX_D];
    const int tid = threadIdx.x;
    const int m = D + (D & 1), h = m / 2;
    const long mat = blockIdx.x;
    const double* Ain = A + mat * D * D;
    double* Aw = work + mat * 2 * m * m;
    double* Vw = Aw + (long)m * m;

    // the symmetrised, padded copy; V = I; |A|_F for the absolute threshold, scaled by the largest entry so that no square
    // overflows (a lane reads back only what it wrote itself)
    double big = 0.0;
    for (int idx = tid; idx < m * m; idx += EIG_THREADS) {
        const int i = idx / m, j = idx % m;
        const double v = (i < D && j < D) ? 0.5 * Ain[i * D + j] + 0.5 * Ain[j * D + i] : 0.0;
        Aw[idx] = v;
        if (V) Vw[idx] = i == j ? 1.0 : 0.0;
        big = fmax(big, fabs(v));
    }
    s_red[tid] = big;
    __syncthreads();
    for (int st = EIG_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) s_red[tid] = fmax(s_red[tid], s_red[tid + st]);
        __syncthreads();
    }
    big = s_red[0];
    __syncthreads();
    double fro = 0.0;
    if (big > 0.0) {
        for (int idx = tid; idx < m * m; idx += EIG_THREADS) {
            const double v = Aw[idx] / big;
            fro += v * v;
        }
    }
    s_red[tid] = fro;
    __syncthreads();
    for (int st = EIG_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) s_red[tid] += s_red[tid + st];
        __syncthreads();
    }
    const double tol_abs = EIG_EPS * big * sqrt(s_red[0]) / (double)m;
    __syncthreads();

    int sweeps = 0, converged = 0;
    for (int sweep = 0; sweep < EIG_MAX_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int step = 0; step < m - 1; ++step) {
            int on = 0;
            if (tid < h) {
                int p, q;
                eig_pair(tid, step, m, p, q);
                const double app = Aw[(long)p * m + p], aqq = Aw[(long)q * m + q], apq = Aw[(long)p * m + q];
                const double mag = fabs(apq);
                double c = 1.0, s = 0.0, t = 0.0;
                // a pair is left alone when its off-diagonal is negligible against its own diagonal or against the matrix;
                // !(<=) so that a NaN rotates (and the sweep limit ends the solve)
                if (!(mag <= EIG_EPS * (sqrt(fabs(app)) * sqrt(fabs(aqq)))) && !(mag <= tol_abs)) {
                    const double theta = 0.5 * (aqq - app) / apq;
                    const double at = fabs(theta);
                    t = 1.0 / (at + hypot(1.0, at));        // no theta^2: a huge theta gives t = 1 / (2 theta), inf gives 0
                    t = theta < 0.0 ? -t : t;
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    on = 1;
                }
                s_p[tid] = p; s_q[tid] = q; s_c[tid] = c; s_s[tid] = s; s_t[tid] = t; s_on[tid] = on;
            }
            if (!__syncthreads_or(on)) continue;            // nothing to rotate in this step: A and V stand
            rotated = 1;
            for (int it = tid; it < h * h; it += EIG_THREADS) {
                const int a = it / h, b = it % h;
                if (!s_on[a] && !s_on[b]) continue;
                const long pa = s_p[a], qa = s_q[a], pb = s_p[b], qb = s_q[b];
                if (a == b) {
                    const double apq = Aw[pa * m + qa], t = s_t[a];
                    Aw[pa * m + pa] -= t * apq;
                    Aw[qa * m + qa] += t * apq;
                    Aw[pa * m + qa] = 0.0;
                    Aw[qa * m + pa] = 0.0;
                    continue;
                }
                // the block in its canonical orientation: rows of the lower-numbered pair, columns of the higher
                const bool up = a < b;
                const int lo = up ? a : b, hi = up ? b : a;
                const double cl = s_c[lo], sl = s_s[lo], ch = s_c[hi], sh = s_s[hi];
                double* e00 = Aw + pa * m + pb;
                double* e01 = Aw + (up ? pa * m + qb : qa * m + pb);
                double* e10 = Aw + (up ? qa * m + pb : pa * m + qb);
                double* e11 = Aw + qa * m + qb;
                const double m00 = *e00, m01 = *e01, m10 = *e10, m11 = *e11;
                const double t00 = m00 * ch - m01 * sh, t01 = m00 * sh + m01 * ch;
                const double t10 = m10 * ch - m11 * sh, t11 = m10 * sh + m11 * ch;
                *e00 = cl * t00 - sl * t10;
                *e01 = cl * t01 - sl * t11;
                *e10 = sl * t00 + cl * t10;
                *e11 = sl * t01 + cl * t11;
            }
            if (V) {
                for (int it = tid; it < m * h; it += EIG_THREADS) {
                    const int k = it / h, i = it % h;
                    if (!s_on[i]) continue;
                    double* vp = Vw + (long)k * m + s_p[i];
                    double* vq = Vw + (long)k * m + s_q[i];
                    const double x = *vp, y = *vq, c = s_c[i], s = s_s[i];
                    *vp = c * x - s * y;
                    *vq = s * x + c * y;
                }
            }
            __syncthreads();
        }
        ++sweeps;
        if (!rotated) {
            converged = 1;
            break;
        }
    }

    // ascending order by rank (ties by index); the vectors follow their values
    double* s_d = s_red;
    if (tid < D) {
        s_d[tid] = Aw[(long)tid * m + tid];
        s_perm[tid] = tid;                      // a NaN matrix has colliding ranks: every slot still names a column
    }
    __syncthreads();
    if (tid < D) {
        const double d = s_d[tid];
        int rank = 0;
        for (int j = 0; j < D; ++j) rank += (s_d[j] < d || (s_d[j] == d && j < tid)) ? 1 : 0;
        w[mat * D + rank] = d;
        s_perm[rank] = tid;
    }
    if (tid == 0) {
        info[mat * 2 + 0] = sweeps;
        info[mat * 2 + 1] = converged;
    }
    if (V) {
        // c^2 + s^2 is 1 only to rounding, so a column's norm drifts over the thousands of rotations it takes part in -- at
        // D = 256 that drift is ten times what the rotations cost the columns' mutual orthogonality.  Each column is
        // normalised once, here.
        double* s_inv = s_red + FD_MAX_D;
        if (tid < D) {
            double n2 = 0.0;
            for (int k = 0; k < D; ++k) {
                const double v = Vw[(long)k * m + tid];
                n2 += v * v;
            }
            s_inv[tid] = 1.0 / sqrt(n2);
        }
        __syncthreads();
        double* Vo = V + mat * D * D;
        for (int idx = tid; idx < D * D; idx += EIG_THREADS) {
            const int k = idx / D, j = idx % D, c = s_perm[j];
            Vo[idx] = Vw[(long)k * m + c] * s_inv[c];
        }
    }
}

int launch_eig(const double* A, int batch, int D, double* w, double* V, int32_t* info, void* work, hipStream_t s) {
    hipLaunchKernelGGL(sym_eig_kernel, dim3((unsigned)batch), dim3(EIG_THREADS), 0, s, A, D, w, V, (int*)info,
                       static_cast<double*>(work));
    MG_CHECK_LAUNCH("sym_eig");
    return MG_OK;
}

// ---------------- the pairs ----------------
struct PairsWork { double* wS; double* VS; double* T; double* B; double* wP; void* eig; };
inline size_t pairs_fixed_bytes(int S, int P, int D) {
    const size_t d = (size_t)D, dd = d * d;
    return align16(((size_t)S * d + (size_t)S * dd + 2 * (size_t)P * dd + (size_t)P * d) * sizeof(double));
}
inline size_t pairs_work_bytes(int S, int P, int D) { return pairs_fixed_bytes(S, P, D) + eig_work_bytes(S > P ? S : P, D); }
inline PairsWork pairs_carve(void* work, int S, int P, int D) {
    const size_t d = (size_t)D, dd = d * d;
    PairsWork W;
    W.wS = static_cast<double*>(work);
    W.VS = W.wS + (size_t)S * d;
    W.T = W.VS + (size_t)S * dd;
    W.B = W.T + (size_t)P * dd;
    W.wP = W.B + (size_t)P * dd;
    W.eig = static_cast<char*>(work) + pairs_fixed_bytes(S, P, D);
    return W;
}

// One 16 x 16 tile of one pair's product, with H = V_a diag(sqrt(max(w_a, 0))):
//   stage 0   T = S_b H      = (S_b V_a) with column j scaled
//   stage 1   B = H^T T      = (V_a^T T) with row i scaled
// A pair that names a set outside 0 .. S - 1 reads nothing and writes NaN.
__global__ __launch_bounds__(MTHREADS) void pair_product_kernel(const double* __restrict__ covs, const double* __restrict__ VS,
                                                                const double* __restrict__ wS, double* __restrict__ T,
                                                                double* __restrict__ Bm, const int* __restrict__ pairs, int S, int D,
                                                                int stage) {
    __shared__ double As[MT][MT + 1], Bs[MT][MT + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long p = blockIdx.z, dd = (long)D * D;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const int i = blockIdx.y * MT + ty, j = blockIdx.x * MT + tx;
    double* out = (stage == 0 ? T : Bm) + p * dd;
    if (a < 0 || a >= S || b < 0 || b >= S) {
        if (i < D && j < D) out[(long)i * D + j] = nan("");
        return;
    }
    const double* Va = VS + a * dd;
    const double* left = stage == 0 ? covs + b * dd : Va;
    const double* right = stage == 0 ? Va : T + p * dd;
    double acc = 0.0;
    for (int k0 = 0; k0 < D; k0 += MT) {
        // As[row of the tile][k], Bs[k][column of the tile]
        if (stage == 0) {
            const int r = blockIdx.y * MT + ty, k = k0 + tx;
            As[ty][tx] = (r < D && k < D) ? left[(long)r * D + k] : 0.0;
        } else {                                // V_a^T: element (row i, k) is V_a[k][i]; read along V_a's rows
            const int k = k0 + ty, r = blockIdx.y * MT + tx;
            As[tx][ty] = (r < D && k < D) ? left[(long)k * D + r] : 0.0;
        }
        {
            const int k = k0 + ty;
            Bs[ty][tx] = (k < D && j < D) ? right[(long)k * D + j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MT; ++k) acc += As[ty][k] * Bs[k][tx];
        __syncthreads();
    }
    if (i < D && j < D) {
        const double wv = wS[(long)a * D + (stage == 0 ? j : i)];
        out[(long)i * D + j] = acc * sqrt(wv > 0.0 ? wv : 0.0);
    }
}

// a fixed tree over the workgroup's MTHREADS values
__device__ __forceinline__ double block_sum(double v, double* s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int st = MTHREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_red[threadIdx.x] += s_red[threadIdx.x + st];
        __syncthreads();
    }
    return s_red[0];
}
__device__ __forceinline__ double block_max(double v, double* s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int st = MTHREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_red[threadIdx.x] = fmax(s_red[threadIdx.x], s_red[threadIdx.x + st]);
        __syncthreads();
    }
    return s_red[0];
}

// workgroups 0 .. S - 1: the spectrum of set s; S .. S + P - 1: the distance of pair p.  Lane i owns element i (D <= 256).
__global__ __launch_bounds__(MTHREADS) void frechet_finish_kernel(const double* __restrict__ means, const double* __restrict__ covs,
                                                                  const double* __restrict__ wS, const double* __restrict__ wP,
                                                                  const int* __restrict__ pairs, const int* __restrict__ info, int S,
                                                                  int D, double* __restrict__ out, double* __restrict__ spectrum) {
    __shared__ double s_red[MTHREADS];
    const int tid = threadIdx.x;
    const bool live = tid < D;
    if ((int)blockIdx.x < S) {
        const long s = blockIdx.x;
        double wv = live ? wS[s * D + tid] : 0.0;
        wv = wv > 0.0 ? wv : 0.0;
        const double sum = block_sum(wv, s_red), sq = block_sum(wv * wv, s_red), top = block_max(wv, s_red);
        const double pr = sum > 0.0 ? wv / sum : 0.0;
        const double ent = block_sum(pr > 0.0 ? -pr * log(pr) : 0.0, s_red);
        if (tid == 0) {
            const bool ok = info[2 * s + 1] != 0 && sum > 0.0;
            spectrum[3 * s + 0] = ok ? sum * sum / sq : nan("");
            spectrum[3 * s + 1] = ok ? exp(ent) : nan("");
            spectrum[3 * s + 2] = ok ? top / sum : nan("");
        }
        return;
    }
    const long p = (long)blockIdx.x - S, dd = (long)D * D;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= S || b < 0 || b >= S) {
        if (tid < 4) out[4 * p + tid] = nan("");
        return;
    }
    const double dm = live ? means[(long)a * D + tid] - means[(long)b * D + tid] : 0.0;
    const double tr = live ? covs[a * dd + (long)tid * D + tid] + covs[b * dd + (long)tid * D + tid] : 0.0;
    const double wv = live ? wP[p * D + tid] : 0.0;
    const double mean_term = block_sum(dm * dm, s_red), trace = block_sum(tr, s_red);
    const double root = block_sum(wv > 0.0 ? sqrt(wv) : 0.0, s_red);
    if (tid == 0) {
        const bool ok = info[2 * a + 1] != 0 && info[2 * (S + p) + 1] != 0;
        out[4 * p + 0] = ok ? mean_term + trace - 2.0 * root : nan("");
        out[4 * p + 1] = mean_term;
        out[4 * p + 2] = trace;
        out[4 * p + 3] = ok ? root : nan("");
    }
}

int check_work(const char* who, size_t have, size_t need) {
    if (have < need) {
        mg_set_error("%s: workspace of %zu bytes, %zu needed (mg_frechet_workspace_bytes)", who, have, need);
        return MG_EWORK;
    }
    return MG_OK;
}
inline bool moments_ok(long n, int D) { return n >= 2 && n <= FD_MAX_ROWS && D >= 4 && D <= FD_MAX_D && D % 4 == 0; }

}  // namespace

extern "C" {

size_t mg_frechet_workspace_bytes(long n, int D, int S, int P) {
    if (D < 1 || D > FD_MAX_D || n < 0 || S < 0 || S > FD_MAX_BATCH || P < 0 || P > FD_MAX_PAIRS) return 0;
    if (n > 0 && !moments_ok(n, D)) return 0;
    if (n == 0 && S == 0) return 0;
    if (P > 0 && S == 0) return 0;
    size_t need = 0;
    if (n > 0) need = moment_work_bytes(n, D);
    if (S > 0) {
        const size_t e = P > 0 ? pairs_work_bytes(S, P, D) : eig_work_bytes(S, D);
        need = e > need ? e : need;
    }
    return need;
}

int mg_feat_moments(const float* X, long n, int D, double* mean, double* cov, void* work, size_t work_bytes, mg_stream_t stream) {
    MG_CHECK_ARG(X && mean && cov && work, "mg_feat_moments: null X / mean / cov / work");
    MG_CHECK_ARG((((uintptr_t)X | (uintptr_t)work) & 15) == 0, "mg_feat_moments: X and work must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)mean | (uintptr_t)cov) & 7) == 0, "mg_feat_moments: mean and cov must be 8-byte aligned");
    MG_CHECK_ARG(D >= 4 && D <= FD_MAX_D && D % 4 == 0, "mg_feat_moments: D must be a multiple of 4 in 4..%d", FD_MAX_D);
    MG_CHECK_ARG(n >= 2 && n <= FD_MAX_ROWS, "mg_feat_moments: 2..2^20 rows");
    const int rc = check_work("mg_feat_moments", work_bytes, moment_work_bytes(n, D));
    if (rc != MG_OK) return rc;
    return launch_moments(X, n, D, mean, cov, work, ST);
}

int mg_sym_eig(const double* A, int batch, int D, double* w, double* V, int32_t* info, void* work, size_t work_bytes,
               mg_stream_t stream) {
    MG_CHECK_ARG(A && w && info && work, "mg_sym_eig: null A / w / info / work");
    MG_CHECK_ARG((((uintptr_t)A | (uintptr_t)w | (uintptr_t)V | (uintptr_t)work) & 7) == 0,
                 "mg_sym_eig: A, w, V and work must be 8-byte aligned");
    MG_CHECK_ARG(((uintptr_t)info & 3) == 0, "mg_sym_eig: info must be 4-byte aligned");
    MG_CHECK_ARG(D >= 1 && D <= FD_MAX_D, "mg_sym_eig: D must be in 1..%d", FD_MAX_D);
    MG_CHECK_ARG(batch >= 1 && batch <= FD_MAX_BATCH, "mg_sym_eig: 1..%d matrices", FD_MAX_BATCH);
    const int rc = check_work("mg_sym_eig", work_bytes, eig_work_bytes(batch, D));
    if (rc != MG_OK) return rc;
    return launch_eig(A, batch, D, w, V, info, work, ST);
}

int mg_frechet_pairs(const double* means, const double* covs, int S, int D, const int32_t* pairs, int P, double* out,
                     double* spectrum, int32_t* info, void* work, size_t work_bytes, mg_stream_t stream) {
    MG_CHECK_ARG(means && covs && pairs && out && spectrum && info && work,
                 "mg_frechet_pairs: null means / covs / pairs / out / spectrum / info / work");
    MG_CHECK_ARG((((uintptr_t)means | (uintptr_t)covs | (uintptr_t)out | (uintptr_t)spectrum) & 7) == 0,
                 "mg_frechet_pairs: means, covs, out and spectrum must be 8-byte aligned");
    MG_CHECK_ARG((((uintptr_t)pairs | (uintptr_t)info) & 3) == 0, "mg_frechet_pairs: pairs and info must be 4-byte aligned");
    MG_CHECK_ARG(((uintptr_t)work & 15) == 0, "mg_frechet_pairs: work must be 16-byte aligned");
    MG_CHECK_ARG(D >= 1 && D <= FD_MAX_D, "mg_frechet_pairs: D must be in 1..%d", FD_MAX_D);
    MG_CHECK_ARG(S >= 1 && S <= FD_MAX_BATCH, "mg_frechet_pairs: 1..%d sets", FD_MAX_BATCH);
    MG_CHECK_ARG(P >= 1 && P <= FD_MAX_PAIRS, "mg_frechet_pairs: 1..%d pairs", FD_MAX_PAIRS);
    int rc = check_work("mg_frechet_pairs", work_bytes, pairs_work_bytes(S, P, D));
    if (rc != MG_OK) return rc;
    const PairsWork W = pairs_carve(work, S, P, D);
    if ((rc = launch_eig(covs, S, D, W.wS, W.VS, info, W.eig, ST)) != MG_OK) return rc;
    const unsigned nt = (unsigned)((D + MT - 1) / MT);
    for (int stage = 0; stage < 2; ++stage) {
        hipLaunchKernelGGL(pair_product_kernel, dim3(nt, nt, (unsigned)P), dim3(MTHREADS), 0, ST, covs, (const double*)W.VS,
                           (const double*)W.wS, W.T, W.B, (const int*)pairs, S, D, stage);
        MG_CHECK_LAUNCH("frechet_pair_product");
    }
    if ((rc = launch_eig(W.B, P, D, W.wP, nullptr, info + 2 * S, W.eig, ST)) != MG_OK) return rc;
    hipLaunchKernelGGL(frechet_finish_kernel, dim3((unsigned)(S + P)), dim3(MTHREADS), 0, ST, means, covs, (const double*)W.wS,
                       (const double*)W.wP, (const int*)pairs, (const int*)info, S, D, out, spectrum);
    MG_CHECK_LAUNCH("frechet_finish");
    return MG_OK;
}

}  // extern "C"
