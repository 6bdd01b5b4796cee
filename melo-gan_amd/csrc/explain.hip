// Integrated gradients of the frozen emotion classifier, per note (melo_gan_amd/emotion_discriminator/explain.py).  The
// classifier's forward and its input gradient are GanEngine's (_ed_fwd / _ed_bwd); the four kernels here build the rows it
// runs on, seed its backward pass, reduce the path's gradients and rank the notes.  The baseline b is the silent roll, every
// value -1: the padding row of mg_roll_encode.  The layout is in include/melo_gan_hip.h; the host restatements are in
// explain.py.  No atomics: every output word has one writer and a fixed summation order.
#include "common.h"
#include "softmax64.h"

#define ST ((hipStream_t)stream)

constexpr int IG_THREADS = 256;
constexpr int IG_WAVES = IG_THREADS / 64;
constexpr int IG_MAX_K = 32;
constexpr int IG_MAX_T = 4096;
constexpr int IG_RANK_TILE = 1024;      // doubles of `note` held in LDS at a time
constexpr int IG_SUMS = 5;              // total, then the four channel sums

typedef double f64x4 __attribute__((ext_vector_type(4)));

// window of batch row r: R consecutive rows per window, G = B / R windows per batch, the cursor counting batches
// (mg_scatter_rows_cursor's rule with G in the place of the batch).  -1: the row has no window.
__device__ __forceinline__ long ig_window(int r, int B, int R, long W, const unsigned long long* counter,
                                          const unsigned long long* base) {
    const int G = B / R;
    if (r >= G * R) return -1;
    const unsigned long long w = (counter[0] - base[0]) * (unsigned long long)G + (unsigned long long)(r / R);
    return w < (unsigned long long)W ? (long)w : -1;
}

// One workgroup per batch row; a thread per position, one 16-byte load and one 16-byte store each.
__global__ __launch_bounds__(IG_THREADS) void ig_rows_kernel(const f32x4* __restrict__ X, const int* __restrict__ win_len,
                                                             const int* __restrict__ rank, const int* __restrict__ n_del, int D,
                                                             long W, int T, int B, int R, int mode, f32x4* __restrict__ out,
                                                             const unsigned long long* __restrict__ counter,
                                                             const unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    const int r = blockIdx.x;
    const long w = ig_window(r, B, R, W, counter, base);
    f32x4* o = out + (long)r * T;
    if (w < 0) {
        f32x4 v;
        v[0] = v[1] = v[2] = v[3] = -1.0f;
        for (int t = threadIdx.x; t < T; t += IG_THREADS) o[t] = v;
        return;
    }
    const f32x4* x = X + w * T;
    const int j = r % R;
    if (mode == MG_IG_PATH) {
        const double alpha = ((double)j + 0.5) / (double)R;
        for (int t = threadIdx.x; t < T; t += IG_THREADS) {
            const f32x4 a = x[t];
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (float)(-1.0 + alpha * ((double)a[c] - (-1.0)));
            o[t] = v;
        }
        return;
    }
    const int len = win_len[w];
    const bool head = j < D;
    const int n = n_del[head ? j : j - D];
    const int* rk = rank + w * T;
    for (int t = threadIdx.x; t < T; t += IG_THREADS) {
        f32x4 v = x[t];
        const int q = rk[t];
        if (q >= 0 && t < len && (head ? q < n : q >= len - n)) v[0] = v[1] = v[2] = v[3] = -1.0f;
        o[t] = v;
    }
}

// One lane per batch row.
__global__ __launch_bounds__(64) void ig_seed_kernel(const float* __restrict__ logits, const int* __restrict__ target, long W,
                                                     int B, int K, int R, float* __restrict__ dlogits, double* __restrict__ logp,
                                                     const unsigned long long* __restrict__ counter,
                                                     const unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= B) return;
    float* dl = dlogits + (long)r * K;
    const long w = ig_window(r, B, R, W, counter, base);
    if (w < 0) {
        for (int j = 0; j < K; ++j) dl[j] = 0.0f;
        logp[r] = 0.0;
        return;
    }
    const int k = target[w];
    if (k < 0 || k >= K) {      // the targets lie on the device, so the entry point cannot see them
        for (int j = 0; j < K; ++j) dl[j] = __builtin_nanf("");
        logp[r] = __builtin_nan("");
        return;
    }
    const float* z = logits + (long)r * K;
    double p[IG_MAX_K];
    softmax64_row(z, K, p);
    // log p[k] by softmax64_row's own terms: (z[k] - max) - log(1 + the other terms, in class order)
    int pred = 0;
    for (int j = 1; j < K; ++j)
        if (z[j] > z[pred]) pred = j;
    const double m = (double)z[pred];
    double rest = 0.0;
    for (int j = 0; j < K; ++j)
        if (j != pred) rest = rest + exp((double)z[j] - m);
    logp[r] = ((double)z[k] - m) - log(1.0 + rest);
    for (int j = 0; j < K; ++j) dl[j] = (float)((j == k ? 1.0 : 0.0) - p[j]);
}

// v summed over the workgroup in a fixed order: a butterfly over each wave, then the waves in order.  Every thread returns
// the sum.  `part` holds IG_WAVES doubles.
__device__ __forceinline__ double ig_block_sum(double v, double* part) {
#pragma clang fp contract(off)
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    __syncthreads();            // the last call's readers are done
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int q = 1; q < IG_WAVES; ++q) s = s + part[q];
    return s;
}

// One workgroup per window of the batch.  A thread owns the positions t = tid, tid + 256, ..: the window's R gradient rows
// added in row order, one 16-byte load each, times (x - b) / R; its positions' attributions added in position order, then
// ig_block_sum.
__global__ __launch_bounds__(IG_THREADS) void ig_accumulate_kernel(const f32x4* __restrict__ dnotes, const f32x4* __restrict__ X,
                                                                   long W, int T, int B, int R, f64x4* __restrict__ attr,
                                                                   double* __restrict__ note, double* __restrict__ sums,
                                                                   const unsigned long long* __restrict__ counter,
                                                                   const unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    __shared__ double part[IG_WAVES];
    const int g = blockIdx.x;
    const long w = ig_window(g * R, B, R, W, counter, base);
    if (w < 0) return;          // uniform over the workgroup
    const f32x4* x = X + w * T;
    const f32x4* d = dnotes + (long)g * R * T;
    double acc[IG_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < T; t += IG_THREADS) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < R; ++i) {
            const f32x4 gq = d[(long)i * T + t];
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] = s[c] + (double)gq[c];
        }
        const f32x4 a = x[t];
        f64x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double dx = (double)a[c] - (-1.0);
            v[c] = dx == 0.0 ? 0.0 : dx * (s[c] / (double)R);       // a note equal to the baseline: exactly 0
        }
        const double nt = ((v[0] + v[1]) + v[2]) + v[3];
        attr[w * T + t] = v;
        note[w * T + t] = nt;
        acc[0] = acc[0] + nt;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[1 + c] = acc[1 + c] + v[c];
    }
#pragma unroll
    for (int q = 0; q < IG_SUMS; ++q) {
        const double s = ig_block_sum(acc[q], part);
        if (threadIdx.x == 0) sums[w * IG_SUMS + q] = s;
    }
}

// One workgroup per window.  rank[t] = the number of real events u with note[u] > note[t], or equal and u < t: counted over
// tiles of the window's `note` in LDS, every lane reading the same word.  A window with a NaN among its events, or with a
// length outside [0, T], gets -1 everywhere.
__global__ __launch_bounds__(IG_THREADS) void ig_rank_kernel(const double* __restrict__ note, const int* __restrict__ win_len,
                                                             int T, int* __restrict__ rank) {
    __shared__ double tile[IG_RANK_TILE];
    const long w = blockIdx.x;
    const double* v = note + w * T;
    int* rk = rank + w * T;
    int len = win_len[w];
    int bad = len < 0 || len > T;
    if (bad) len = 0;
    for (int t = threadIdx.x; t < len; t += IG_THREADS) bad |= isnan(v[t]) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (bad) len = 0;
    for (int t0 = 0; t0 < T; t0 += IG_THREADS) {        // uniform trip count: every thread reaches the barriers below
        const int t = t0 + threadIdx.x;
        const bool mine = t < len;
        const double me = mine ? v[t] : 0.0;
        int cnt = 0;
        for (int u0 = 0; u0 < len; u0 += IG_RANK_TILE) {
            const int nu = min(IG_RANK_TILE, len - u0);
            __syncthreads();
            for (int i = threadIdx.x; i < nu; i += IG_THREADS) tile[i] = v[u0 + i];
            __syncthreads();
            if (mine)
                for (int i = 0; i < nu; ++i) {
                    const double o = tile[i];
                    cnt += (o > me || (o == me && u0 + i < t)) ? 1 : 0;
                }
        }
        if (t < T) rk[t] = mine ? cnt : -1;
    }
}

extern "C" {

static int ig_check_batch(const char* who, long W, int T, int B, int R) {
    MG_CHECK_ARG(W >= 1 && W <= 0x7FFFFFFFL, "%s: W = %ld: 1..2^31 - 1", who, W);
    MG_CHECK_ARG(T >= 1 && T <= IG_MAX_T, "%s: T = %d: 1..%d", who, T, IG_MAX_T);
    MG_CHECK_ARG(B >= 1 && B <= 65535 && R >= 1 && R <= B, "%s: B = %d, rows_per_window = %d: 1 <= rows_per_window <= B <= 65535",
                 who, B, R);
    return MG_OK;
}

int mg_ig_rows(const float* X, const int32_t* win_len, const int32_t* rank, const int32_t* n_del, int D, long W, int T, int B, int R,
               int mode, float* out, const uint64_t* counter, const uint64_t* base, mg_stream_t stream) {
    MG_CHECK_ARG(X && out && counter && base, "mg_ig_rows: null X / out / counter / base");
    if (ig_check_batch("mg_ig_rows", W, T, B, R) != MG_OK) return MG_EARG;
    MG_CHECK_ARG(mode == MG_IG_PATH || mode == MG_IG_DELETE, "mg_ig_rows: mode = %d: MG_IG_PATH or MG_IG_DELETE", mode);
    if (mode == MG_IG_DELETE) {
        MG_CHECK_ARG(win_len && rank && n_del, "mg_ig_rows: deletion rows need win_len, rank and n_del");
        MG_CHECK_ARG(D >= 1 && R == 2 * D, "mg_ig_rows: rows_per_window = %d with %d deletion counts: 2 per count", R, D);
        MG_CHECK_ARG((((uintptr_t)win_len | (uintptr_t)rank | (uintptr_t)n_del) & 3) == 0,
                     "mg_ig_rows: win_len, rank and n_del must be 4-byte aligned");
    }
    MG_CHECK_ARG((((uintptr_t)X | (uintptr_t)out) & 15) == 0, "mg_ig_rows: X and out must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)counter | (uintptr_t)base) & 7) == 0, "mg_ig_rows: counter and base must be 8-byte aligned");
    hipLaunchKernelGGL(ig_rows_kernel, dim3((unsigned)B), dim3(IG_THREADS), 0, ST, (const f32x4*)X, (const int*)win_len,
                       (const int*)rank, (const int*)n_del, D, W, T, B, R, mode, (f32x4*)out, (const unsigned long long*)counter,
                       (const unsigned long long*)base);
    MG_CHECK_LAUNCH("ig_rows");
    return MG_OK;
}

int mg_ig_seed(const float* logits, const int32_t* target, long W, int B, int n_classes, int R, float* dlogits, double* logp,
               const uint64_t* counter, const uint64_t* base, mg_stream_t stream) {
    MG_CHECK_ARG(logits && target && dlogits && logp && counter && base,
                 "mg_ig_seed: null logits / target / dlogits / logp / counter / base");
    MG_CHECK_ARG(W >= 1 && W <= 0x7FFFFFFFL, "mg_ig_seed: W = %ld: 1..2^31 - 1", W);
    MG_CHECK_ARG(B >= 1 && B <= (1 << 24) && R >= 1 && R <= B, "mg_ig_seed: B = %d, rows_per_window = %d: 1 <= rows_per_window <= B "
                 "<= 2^24", B, R);
    MG_CHECK_ARG(n_classes >= 2 && n_classes <= IG_MAX_K, "mg_ig_seed: %d classes: 2..%d", n_classes, IG_MAX_K);
    MG_CHECK_ARG((((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 3) == 0 &&
                     (((uintptr_t)logp | (uintptr_t)counter | (uintptr_t)base) & 7) == 0,
                 "mg_ig_seed: logits, target and dlogits must be 4-byte, logp, counter and base 8-byte aligned");
    hipLaunchKernelGGL(ig_seed_kernel, dim3((unsigned)mg_cdiv(B, 64)), dim3(64), 0, ST, logits, (const int*)target, W, B, n_classes, R,
                       dlogits, logp, (const unsigned long long*)counter, (const unsigned long long*)base);
    MG_CHECK_LAUNCH("ig_seed");
    return MG_OK;
}

int mg_ig_accumulate(const float* dnotes, const float* X, long W, int T, int B, int R, double* attr, double* note, double* sums,
                     const uint64_t* counter, const uint64_t* base, mg_stream_t stream) {
    MG_CHECK_ARG(dnotes && X && attr && note && sums && counter && base,
                 "mg_ig_accumulate: null dnotes / X / attr / note / sums / counter / base");
    if (ig_check_batch("mg_ig_accumulate", W, T, B, R) != MG_OK) return MG_EARG;
    MG_CHECK_ARG((((uintptr_t)dnotes | (uintptr_t)X) & 15) == 0 && ((uintptr_t)attr & 31) == 0,
                 "mg_ig_accumulate: dnotes and X must be 16-byte, attr 32-byte aligned");
    MG_CHECK_ARG((((uintptr_t)note | (uintptr_t)sums | (uintptr_t)counter | (uintptr_t)base) & 7) == 0,
                 "mg_ig_accumulate: note, sums, counter and base must be 8-byte aligned");
    hipLaunchKernelGGL(ig_accumulate_kernel, dim3((unsigned)(B / R)), dim3(IG_THREADS), 0, ST, (const f32x4*)dnotes, (const f32x4*)X,
                       W, T, B, R, (f64x4*)attr, note, sums, (const unsigned long long*)counter, (const unsigned long long*)base);
    MG_CHECK_LAUNCH("ig_accumulate");
    return MG_OK;
}

int mg_ig_rank(const double* note, const int32_t* win_len, long W, int T, int32_t* rank, mg_stream_t stream) {
    MG_CHECK_ARG(note && win_len && rank, "mg_ig_rank: null note / win_len / rank");
    MG_CHECK_ARG(W >= 1 && W <= 0x7FFFFFFFL, "mg_ig_rank: W = %ld: 1..2^31 - 1", W);
    MG_CHECK_ARG(T >= 1 && T <= IG_MAX_T, "mg_ig_rank: T = %d: 1..%d", T, IG_MAX_T);
    MG_CHECK_ARG(((uintptr_t)note & 7) == 0 && (((uintptr_t)win_len | (uintptr_t)rank) & 3) == 0,
                 "mg_ig_rank: note must be 8-byte, win_len and rank 4-byte aligned");
    hipLaunchKernelGGL(ig_rank_kernel, dim3((unsigned)W), dim3(IG_THREADS), 0, ST, note, (const int*)win_len, T, (int*)rank);
    MG_CHECK_LAUNCH("ig_rank");
    return MG_OK;
}

int mg_ig_rank_tile(void) { return IG_RANK_TILE; }

}  // extern "C"
