// Held-out evaluation of a trained VAE (melo_gan_amd/ae/evaluate.py): the reconstruction, note-level and latent statistics of
// one evaluated batch added to a device-resident accumulator that lives for the whole pass.  The layout and the reference
// lines these answer to are in include/melo_gan_hip.h (mg_vae_eval_acc); the host restatement is melo_gan_amd/ae/metrics.py.
#include "common.h"
#include "note_decode.h"

#define ST ((hipStream_t)stream)

constexpr int VM_THREADS = 256;
// one accumulator block per true class, 8-byte words (include/melo_gan_hip.h): int64 c[16], then the fp64 sums
constexpr int VM_C = 16;
enum { VC_ROWS, VC_VALID, VC_INVALID, VC_BOTH_ON, VC_BOTH_REST, VC_MISSED, VC_EXTRA, VC_PITCH_EQ, VC_PITCH_1, VC_PC_EQ,
       VC_PITCH_ABS, VC_VEL_ABS, VC_USED };
constexpr int VM_NI = VC_USED - 1;      // the counters a lane carries: c[1 .. 11]
enum { VD_SE = 0, VD_AE = 4, VD_DUR = 8, VD_STEP = 9, VM_D = 10 };
constexpr int VM_HEAD = VM_C + VM_D;    // 26: also one row's entry of `work`, in the block's own layout
constexpr int VM_LAT = 5;               // sum mu, mu^2, logvar, exp(logvar), KL -- each [L]
constexpr int VM_MAX_L = 1024;

__host__ __device__ static inline long vae_block_words(int L) { return VM_HEAD + (long)VM_LAT * L; }

// -1/2 (1 + lv - mu^2 - exp lv) in fp64, the operations in the order the expression is written
__device__ __forceinline__ double vae_kl_term(double m, double lv, double elv) {
#pragma clang fp contract(off)
    return -0.5 * (((1.0 + lv) - m * m) - elv);
}

// Launch 1: one workgroup per row.  Lane u takes time positions u, u + 256, ... of x and recon (one 16-byte load each) and
// latent dimensions u, u + 256, ...; it adds its own terms in order, the 256 lanes are reduced by a fixed tree in LDS, and
// the row's partial goes to the row's own entry of `work` and to row_i / row_d.  No atomics.
__global__ __launch_bounds__(VM_THREADS) void vae_rows_kernel(
    const float* __restrict__ x, const float* __restrict__ recon, const float* __restrict__ mu, const float* __restrict__ logvar,
    const int64_t* __restrict__ labels, int T, int L, int K, long long* __restrict__ work, int* __restrict__ row_i,
    double* __restrict__ row_d, long dst_rows, const unsigned long long* __restrict__ counter,
    const unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    __shared__ double s_d[VM_D + 1][VM_THREADS];        // [VM_D]: the row's KL
    __shared__ int s_i[VM_NI][VM_THREADS];
    const int row = (int)blockIdx.x, u = threadIdx.x;
    const int64_t y = labels[row];
    if (y < 0 || y >= K) return;                // a padding row: counts nowhere, writes nothing (uniform over the workgroup)
    const f32x4* xs = reinterpret_cast<const f32x4*>(x + (long)row * T * 4);
    const f32x4* rs = reinterpret_cast<const f32x4*>(recon + (long)row * T * 4);
    int ci[VM_NI];
    double cd[VM_D + 1];
#pragma unroll
    for (int q = 0; q < VM_NI; ++q) ci[q] = 0;
#pragma unroll
    for (int q = 0; q <= VM_D; ++q) cd[q] = 0.0;
    for (int t = u; t < T; t += VM_THREADS) {
        const f32x4 a = xs[t], b = rs[t];
        const NoteEvent ea = note_decode(a), eb = note_decode(b);
        if (!(ea.valid && eb.valid)) {
            ci[VC_INVALID - 1] += 1;
            continue;
        }
        ci[VC_VALID - 1] += 1;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const double d = (double)b[ch] - (double)a[ch];
            cd[VD_SE + ch] += d * d;
            cd[VD_AE + ch] += fabs(d);
        }
        cd[VD_STEP] += fabs(eb.step - ea.step);
        if (ea.sounding && eb.sounding) {
            const int dp = abs(eb.pitch - ea.pitch);
            ci[VC_BOTH_ON - 1] += 1;
            ci[VC_PITCH_EQ - 1] += dp == 0;
            ci[VC_PITCH_1 - 1] += dp <= 1;
            ci[VC_PC_EQ - 1] += dp % 12 == 0;
            ci[VC_PITCH_ABS - 1] += dp;
            ci[VC_VEL_ABS - 1] += abs(eb.vel - ea.vel);
            cd[VD_DUR] += fabs(eb.dur - ea.dur);
        } else if (ea.sounding) {
            ci[VC_MISSED - 1] += 1;
        } else if (eb.sounding) {
            ci[VC_EXTRA - 1] += 1;
        } else {
            ci[VC_BOTH_REST - 1] += 1;
        }
    }
    for (int j = u; j < L; j += VM_THREADS) {
        const double m = (double)mu[(long)row * L + j], lv = (double)logvar[(long)row * L + j];
        cd[VM_D] += vae_kl_term(m, lv, exp(lv));
    }
#pragma unroll
    for (int q = 0; q < VM_NI; ++q) s_i[q][u] = ci[q];
#pragma unroll
    for (int q = 0; q <= VM_D; ++q) s_d[q][u] = cd[q];
    __syncthreads();
    for (int s = VM_THREADS / 2; s > 0; s >>= 1) {      // the fixed tree
        if (u < s) {
#pragma unroll
            for (int q = 0; q < VM_NI; ++q) s_i[q][u] += s_i[q][u + s];
#pragma unroll
            for (int q = 0; q <= VM_D; ++q) s_d[q][u] += s_d[q][u + s];
        }
        __syncthreads();
    }
    if (u < VM_HEAD) {
        long long v = 0;
        if (u == VC_ROWS) v = 1;
        else if (u < VC_USED) v = (long long)s_i[u - 1][0];
        else if (u >= VM_C) v = __double_as_longlong(s_d[u - VM_C][0]);
        work[(long)row * VM_HEAD + u] = v;
    }
    const unsigned long long p = (counter[0] - base[0]) * (unsigned long long)gridDim.x + (unsigned long long)row;
    if (p < (unsigned long long)dst_rows) {             // the padded tail of the last batch falls off the end
        if (u < 8) row_i[(long)p * 8 + u] = s_i[u][0];  // c[1 .. 8]
        if (u < 4) {
            double v;
            if (u == 0) v = ((s_d[VD_SE][0] + s_d[VD_SE + 1][0]) + s_d[VD_SE + 2][0]) + s_d[VD_SE + 3][0];
            else if (u == 1) v = s_d[VM_D][0];
            else v = s_d[u == 2 ? VD_DUR : VD_STEP][0];
            row_d[(long)p * 4 + u] = v;
        }
    }
}

// Launch 2: one lane owns one accumulator word of one class and adds the batch's rows of that class onto it, rows 0 .. B-1 in
// order, one at a time: the result does not depend on how a split is cut into batches.  The head words come from the rows'
// entries of `work`, the latent words straight from mu / logvar.
__global__ __launch_bounds__(VM_THREADS) void vae_fold_kernel(
    const long long* __restrict__ work, const float* __restrict__ mu, const float* __restrict__ logvar,
    const int64_t* __restrict__ labels, int B, int L, long long* __restrict__ acc, unsigned long long* tick) {
#pragma clang fp contract(off)
    const int k = (int)blockIdx.y;
    const long w = (long)blockIdx.x * VM_THREADS + threadIdx.x, words = vae_block_words(L);
    if (w < words) {
        long long* a = acc + (long)k * words + w;
        if (w < VM_C) {
            long long v = *a;
            for (int r = 0; r < B; ++r)
                if (labels[r] == (int64_t)k) v += work[(long)r * VM_HEAD + w];
            *a = v;
        } else if (w < VM_HEAD) {
            double v = __longlong_as_double(*a);
            for (int r = 0; r < B; ++r)
                if (labels[r] == (int64_t)k) v += __longlong_as_double(work[(long)r * VM_HEAD + w]);
            *a = __double_as_longlong(v);
        } else {
            const int s = (int)((w - VM_HEAD) / L), j = (int)((w - VM_HEAD) % L);
            double v = __longlong_as_double(*a);
            for (int r = 0; r < B; ++r) {
                if (labels[r] != (int64_t)k) continue;
                const double m = (double)mu[(long)r * L + j], lv = (double)logvar[(long)r * L + j];
                double term;
                if (s == 0) term = m;
                else if (s == 1) term = m * m;
                else if (s == 2) term = lv;
                else {
                    const double elv = exp(lv);
                    term = s == 3 ? elv : vae_kl_term(m, lv, elv);
                }
                v += term;
            }
            *a = __double_as_longlong(v);
        }
    }
    if (tick && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) tick[0] += 1ull;
}

__global__ void vae_reset_kernel(long long* acc, long words) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) acc[i] = 0;
}

extern "C" {

long mg_vae_eval_acc_words(int n_classes, int L) {
    if (n_classes < 1 || n_classes > 32 || L < 1 || L > VM_MAX_L) return 0;
    return (long)n_classes * vae_block_words(L);
}

size_t mg_vae_eval_acc_workspace_bytes(int B, int L) {
    if (B < 1 || B > 32767 || L < 1 || L > VM_MAX_L) return 0;
    return (size_t)B * VM_HEAD * sizeof(long long);
}

int mg_vae_eval_acc_reset(void* acc, int n_classes, int L, mg_stream_t stream) {
    MG_CHECK_ARG(acc && ((uintptr_t)acc & 7) == 0, "mg_vae_eval_acc_reset: acc must be an 8-byte aligned device pointer");
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32 && L >= 1 && L <= VM_MAX_L, "mg_vae_eval_acc_reset: 1..32 classes, L in 1..1024");
    const long words = (long)n_classes * vae_block_words(L);
    hipLaunchKernelGGL(vae_reset_kernel, dim3((unsigned)mg_cdiv(words, 256)), dim3(256), 0, ST, (long long*)acc, words);
    MG_CHECK_LAUNCH("vae_reset");
    return MG_OK;
}

int mg_vae_eval_acc(const float* x, const float* recon, int B, int T, int C, const float* mu, const float* logvar, int L,
                    const int64_t* labels, int n_classes, void* acc, int32_t* row_i, double* row_d, long dst_rows,
                    const uint64_t* counter, const uint64_t* base, void* work, size_t work_bytes, uint64_t* tick,
                    mg_stream_t stream) {
    MG_CHECK_ARG(x && recon && mu && logvar && labels && acc && row_i && row_d && counter && base && work,
                 "mg_vae_eval_acc: null x / recon / mu / logvar / labels / acc / row_i / row_d / counter / base / work");
    MG_CHECK_ARG(C == 4, "mg_vae_eval_acc: C = %d: only the (T, 4) note-row format decodes into notes", C);
    MG_CHECK_ARG(B >= 1 && B <= 32767 && T >= 1 && T <= (1 << 20), "mg_vae_eval_acc: B must be in 1..32767 and T in 1..2^20");
    MG_CHECK_ARG(L >= 1 && L <= VM_MAX_L, "mg_vae_eval_acc: L = %d: the latent width must be in 1..1024", L);
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32, "mg_vae_eval_acc: 1..32 classes");
    MG_CHECK_ARG(dst_rows >= 1, "mg_vae_eval_acc: dst_rows must be positive");
    MG_CHECK_ARG((((uintptr_t)x | (uintptr_t)recon) & 15) == 0, "mg_vae_eval_acc: x and recon must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)mu | (uintptr_t)logvar | (uintptr_t)row_i) & 3) == 0,
                 "mg_vae_eval_acc: mu, logvar and row_i must be 4-byte aligned");
    MG_CHECK_ARG((((uintptr_t)acc | (uintptr_t)row_d | (uintptr_t)work) & 7) == 0,
                 "mg_vae_eval_acc: acc, row_d and work must be 8-byte aligned");
    const size_t need = (size_t)B * VM_HEAD * sizeof(long long);
    MG_CHECK_ARG(work_bytes >= need, "mg_vae_eval_acc: workspace of %zu bytes, %zu needed (mg_vae_eval_acc_workspace_bytes)",
                 work_bytes, need);
    hipLaunchKernelGGL(vae_rows_kernel, dim3((unsigned)B), dim3(VM_THREADS), 0, ST, x, recon, mu, logvar, labels, T, L, n_classes,
                       (long long*)work, (int*)row_i, row_d, dst_rows, (const unsigned long long*)counter,
                       (const unsigned long long*)base);
    MG_CHECK_LAUNCH("vae_rows");
    hipLaunchKernelGGL(vae_fold_kernel, dim3((unsigned)mg_cdiv(vae_block_words(L), VM_THREADS), (unsigned)n_classes),
                       dim3(VM_THREADS), 0, ST, (const long long*)work, mu, logvar, labels, B, L, (long long*)acc,
                       (unsigned long long*)tick);
    MG_CHECK_LAUNCH("vae_fold");
    return MG_OK;
}

}  // extern "C"
