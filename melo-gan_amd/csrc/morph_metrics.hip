// Two reductions over paths through the generator's conditioning space (melo_gan_amd/gan/morph.py): the squared step
// lengths of every path in some feature space, and the classifier's probabilities along the paths with their per-group sums.
// Rows are path-major: P paths of S1 consecutive rows.  Both run once, after the last chunk, over resident arrays.  The layout
// is in include/melo_gan_hip.h (mg_path_d2, mg_path_probs); the host restatement is melo_gan_amd/gan/morph_metrics.py.
// No atomics: every output word has one writer and a fixed summation order.
#include "common.h"
#include "softmax64.h"

#define ST ((hipStream_t)stream)

constexpr int PM_THREADS = 256;
constexpr int PM_MAX_K = 32;

// One workgroup per (path, step): sum_j (x[next, j] - x[this, j])^2, next = the following step, or step 0 for the last step (the
// endpoint distance).  Every element is widened before the subtraction.  Per-lane sums in element order, a butterfly over
// the wave, a fixed tree over the four waves.
__global__ __launch_bounds__(PM_THREADS) void path_d2_kernel(const float* __restrict__ x, int S1, int D, int vec,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_w[PM_THREADS / 64];
    const long row = blockIdx.x;
    const int s = (int)(row % S1), u = threadIdx.x;
    const float* a = x + row * D;
    const float* b = s < S1 - 1 ? a + D : a - (long)s * D;
    double sum = 0.0;
    if (vec) {
        for (int i = 4 * u; i < D; i += 4 * PM_THREADS) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(a + i), vb = *reinterpret_cast<const f32x4*>(b + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)vb[j] - (double)va[j];
                sum = sum + d * d;
            }
        }
    } else {
        for (int i = u; i < D; i += PM_THREADS) {
            const double d = (double)b[i] - (double)a[i];
            sum = sum + d * d;
        }
    }
    for (int m = 1; m < 64; m <<= 1) sum = sum + __shfl_xor(sum, m, 64);
    if ((u & 63) == 0) s_w[u >> 6] = sum;
    __syncthreads();
    if (u == 0) out[row] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// One lane per row: the fp64 softmax of the row's fp32 logits by mg_cls_eval_acc's rule (softmax64.h).
__global__ __launch_bounds__(PM_THREADS) void path_softmax_kernel(const float* __restrict__ logits, long rows, int K,
                                                                  double* __restrict__ probs) {
#pragma clang fp contract(off)
    const long row = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (row >= rows) return;
    softmax64_row(logits + row * K, K, probs + row * K);
}

// One lane per accumulator word (g, s, k): the sum of probs[p, s, k] over the paths p = 0 .. P-1 of group g, in that order; the
// word k = K counts them.
__global__ __launch_bounds__(PM_THREADS) void path_fold_kernel(const double* __restrict__ probs, const int* __restrict__ group,
                                                               int P, int S1, int K, int G, double* __restrict__ acc) {
#pragma clang fp contract(off)
    const long w = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (w >= (long)G * S1 * (K + 1)) return;
    const int k = (int)(w % (K + 1)), s = (int)((w / (K + 1)) % S1), g = (int)(w / ((long)(K + 1) * S1));
    double v = 0.0;
    for (int p = 0; p < P; ++p)
        if (group[p] == g) v = v + (k < K ? probs[((long)p * S1 + s) * K + k] : 1.0);
    acc[w] = v;
}

extern "C" {

int mg_path_d2(const float* x, int P, int S1, int D, double* out, mg_stream_t stream) {
    MG_CHECK_ARG(x && out, "mg_path_d2: null x / out");
    MG_CHECK_ARG(P >= 1 && S1 >= 1 && D >= 1 && D <= (1 << 30), "mg_path_d2: P = %d, S1 = %d, D = %d: P, S1 >= 1 and D in 1..2^30", P,
                 S1, D);
    MG_CHECK_ARG((long)P * S1 <= 0x7FFFFFFFL, "mg_path_d2: %ld rows: at most 2^31 - 1", (long)P * S1);
    MG_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 7) == 0, "mg_path_d2: x must be 4-byte and out 8-byte aligned");
    const int vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0;
    hipLaunchKernelGGL(path_d2_kernel, dim3((unsigned)((long)P * S1)), dim3(PM_THREADS), 0, ST, x, S1, D, vec, out);
    MG_CHECK_LAUNCH("path_d2");
    return MG_OK;
}

int mg_path_probs(const float* logits, const int32_t* group, int P, int S1, int n_classes, int n_groups, double* probs,
                  double* acc, mg_stream_t stream) {
    MG_CHECK_ARG(logits && group && probs && acc, "mg_path_probs: null logits / group / probs / acc");
    MG_CHECK_ARG(P >= 1 && S1 >= 1 && n_groups >= 1, "mg_path_probs: P = %d, S1 = %d, n_groups = %d: all must be positive", P, S1,
                 n_groups);
    MG_CHECK_ARG(n_classes >= 2 && n_classes <= PM_MAX_K, "mg_path_probs: %d classes: 2..32", n_classes);
    const long rows = (long)P * S1, words = (long)n_groups * S1 * (n_classes + 1);
    MG_CHECK_ARG(rows <= 0x7FFFFFFFL && words <= 0x7FFFFFFFL, "mg_path_probs: %ld rows, %ld accumulator words: at most 2^31 - 1 each",
                 rows, words);
    MG_CHECK_ARG(((uintptr_t)logits & 3) == 0 && ((uintptr_t)group & 3) == 0 && (((uintptr_t)probs | (uintptr_t)acc) & 7) == 0,
                 "mg_path_probs: logits and group must be 4-byte, probs and acc 8-byte aligned");
    hipLaunchKernelGGL(path_softmax_kernel, dim3((unsigned)mg_cdiv(rows, PM_THREADS)), dim3(PM_THREADS), 0, ST, logits, rows,
                       n_classes, probs);
    MG_CHECK_LAUNCH("path_softmax");
    hipLaunchKernelGGL(path_fold_kernel, dim3((unsigned)mg_cdiv(words, PM_THREADS)), dim3(PM_THREADS), 0, ST, (const double*)probs,
                       (const int*)group, P, S1, n_classes, n_groups, acc);
    MG_CHECK_LAUNCH("path_fold");
    return MG_OK;
}

}  // extern "C"
