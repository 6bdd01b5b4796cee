// Held-out evaluation of a trained emotion classifier (melo_gan_amd/emotion_discriminator/evaluate.py): the confusion,
// calibration and temperature statistics of one evaluated batch added to a device-resident accumulator that lives for the
// whole pass, and the exact one-vs-rest Mann-Whitney counts of a finished pass.  The layout is in include/melo_gan_hip.h
// (mg_cls_eval_acc, mg_cls_auroc_pairs); the host restatement is melo_gan_amd/emotion_discriminator/metrics.py.
#include "common.h"

#define ST ((hipStream_t)stream)

constexpr int CM_MAX_K = 16, CM_MAX_BINS = 32, CM_MAX_G = 64;
constexpr int CM_LANES = 64;            // launch 1: one wave per row, lane g owns inverse temperature g
constexpr int CM_FOLD = 256;
constexpr int CM_HEAD_I = 3;            // rows, correct, flipped
constexpr int CM_HEAD_D = 4;            // ce, brier, conf, margin
constexpr int CM_ROW_I = 4, CM_ROW_D = 4;      // the per-row records: (pred, bin, correct, flipped), (ce, conf, p[y], margin)
constexpr int CM_PAIR = 256;            // mg_cls_auroc_pairs: rows of an i-tile and of a j-tile
constexpr long CM_MAX_N = 131072;

struct cls_temps {
    double inv[CM_MAX_G];
};

__host__ __device__ static inline int cls_ints(int K, int nb) { return CM_HEAD_I + K + 2 * nb; }
__host__ __device__ static inline int cls_block_words(int K, int nb, int G) { return cls_ints(K, nb) + CM_HEAD_D + nb + G; }
// one row's entry of `work`: the int32 record in two words, then brier-ordered doubles (ce, brier, conf, margin), then nll[G]
__host__ __device__ static inline int cls_work_words(int G) { return 2 + CM_HEAD_D + G; }

// log sum_k exp(z_k s) - z_y s with the maximum (z_pred s) taken out and its own term, exp(0) = 1, not computed: the other
// terms are added in class order and go through log1p.  s > 0, so the maximum stays where it is.
__device__ __forceinline__ double cls_nll(const double (&z)[CM_MAX_K], int K, int pred, int y, double s, double& rest_out) {
#pragma clang fp contract(off)
    const double m = z[pred] * s;
    double rest = 0.0;
    for (int k = 0; k < K; ++k)
        if (k != pred) rest += exp(z[k] * s - m);
    rest_out = rest;
    return log1p(rest) + (m - z[y] * s);
}

// Launch 1: one wave per row.  Every lane holds the row's K scaled logits; lane g computes the row's NLL at inverse
// temperature g, lane 0 the row's records.  The row's partial goes to the row's own entry of `work`.  No atomics.
__global__ __launch_bounds__(CM_LANES) void cls_rows_kernel(
    const float* __restrict__ logits, const float* __restrict__ clean, const int64_t* __restrict__ labels, int K, int n_bins,
    cls_temps temps, int G, double inv_temperature, long long* __restrict__ work, double* __restrict__ probs,
    int* __restrict__ row_i, double* __restrict__ row_d, long dst_rows, const unsigned long long* __restrict__ counter,
    const unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    const int row = (int)blockIdx.x, u = threadIdx.x;
    const int64_t yl = labels[row];
    if (yl < 0 || yl >= K) return;              // a padding or unlabelled row: counts nowhere, writes nothing
    const int y = (int)yl;
    double z[CM_MAX_K];
    int pred = 0;
    for (int k = 0; k < K; ++k) {
        z[k] = (double)logits[(long)row * K + k] * inv_temperature;
        if (z[k] > z[pred]) pred = k;           // the lowest index on ties
    }
    long long* w = work + (long)row * cls_work_words(G);
    double rest;
    if (u < G) {
        const double nll = cls_nll(z, K, pred, y, temps.inv[u], rest);
        w[2 + CM_HEAD_D + u] = __double_as_longlong(nll);
    }
    if (u != 0) return;
    const double ce = cls_nll(z, K, pred, y, 1.0, rest);
    const double s = 1.0 + rest, m = z[pred];
    double p[CM_MAX_K], brier = 0.0, second = 0.0;
    for (int k = 0; k < K; ++k) {
        p[k] = k == pred ? 1.0 / s : exp(z[k] - m) / s;
        const double d = p[k] - (k == y ? 1.0 : 0.0);
        brier += d * d;
        if (k != pred && p[k] > second) second = p[k];
    }
    const double conf = p[pred], margin = conf - second;
    int bin = (int)floor(conf * (double)n_bins);
    bin = bin > n_bins - 1 ? n_bins - 1 : bin;
    int flipped = 0;
    if (clean) {
        int cp = 0;
        double best = (double)clean[(long)row * K] * inv_temperature;
        for (int k = 1; k < K; ++k) {
            const double c = (double)clean[(long)row * K + k] * inv_temperature;
            if (c > best) best = c, cp = k;
        }
        flipped = cp != pred;
    }
    const int correct = pred == y;
    int* wi = reinterpret_cast<int*>(w);
    wi[0] = pred, wi[1] = bin, wi[2] = correct, wi[3] = flipped;
    w[2] = __double_as_longlong(ce);
    w[3] = __double_as_longlong(brier);
    w[4] = __double_as_longlong(conf);
    w[5] = __double_as_longlong(margin);
    const unsigned long long pos = (counter[0] - base[0]) * (unsigned long long)gridDim.x + (unsigned long long)row;
    if (pos < (unsigned long long)dst_rows) {   // the padded tail of the last batch falls off the end
        for (int k = 0; k < K; ++k) probs[(long)pos * K + k] = p[k];
        int* ri = row_i + (long)pos * CM_ROW_I;
        ri[0] = pred, ri[1] = bin, ri[2] = correct, ri[3] = flipped;
        double* rd = row_d + (long)pos * CM_ROW_D;
        rd[0] = ce, rd[1] = conf, rd[2] = p[y], rd[3] = margin;
    }
}

// Launch 2: one lane owns one accumulator word of one class and adds the batch's rows of that class onto it, rows 0 .. B-1 in
// order, one at a time: the result does not depend on how a split is cut into batches.
__global__ __launch_bounds__(CM_FOLD) void cls_fold_kernel(const long long* __restrict__ work, const int64_t* __restrict__ labels,
                                                           int B, int K, int nb, int G, long long* __restrict__ acc,
                                                           unsigned long long* tick) {
#pragma clang fp contract(off)
    const int k = (int)blockIdx.y, w = (int)(blockIdx.x * CM_FOLD + threadIdx.x);
    const int ni = cls_ints(K, nb), words = cls_block_words(K, nb, G), ww = cls_work_words(G);
    if (w < words) {
        long long* a = acc + (long)k * words + w;
        if (w < ni) {
            long long v = *a;
            for (int r = 0; r < B; ++r) {
                if (labels[r] != (int64_t)k) continue;
                const int* ri = reinterpret_cast<const int*>(work + (long)r * ww);
                int t;
                if (w == 0) t = 1;
                else if (w == 1) t = ri[2];
                else if (w == 2) t = ri[3];
                else if (w < CM_HEAD_I + K) t = ri[0] == w - CM_HEAD_I;
                else if (w < CM_HEAD_I + K + nb) t = ri[1] == w - CM_HEAD_I - K;
                else t = ri[1] == w - CM_HEAD_I - K - nb && ri[2];
                v += t;
            }
            *a = v;
        } else {
            const int d = w - ni;
            double v = __longlong_as_double(*a);
            for (int r = 0; r < B; ++r) {
                if (labels[r] != (int64_t)k) continue;
                const long long* wr = work + (long)r * ww;
                if (d < CM_HEAD_D) v += __longlong_as_double(wr[2 + d]);
                else if (d < CM_HEAD_D + nb) {
                    if (reinterpret_cast<const int*>(wr)[1] == d - CM_HEAD_D) v += __longlong_as_double(wr[4]);
                } else v += __longlong_as_double(wr[2 + CM_HEAD_D + (d - CM_HEAD_D - nb)]);
            }
            *a = __double_as_longlong(v);
        }
    }
    if (tick && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) tick[0] += 1ull;
}

__global__ void cls_zero_kernel(long long* p, long words) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) p[i] = 0;
}

// One-vs-rest Mann-Whitney counts.  Workgroup (bx, by) owns i-tile bx and walks j-tiles by, by + gridDim.y, ... through LDS;
// lane i with a valid label k compares its own p_ik with p_jk of every valid j of another class.  Integer counts only:
// reduced inside the wave by shuffles, across the waves in LDS, then one integer atomicAdd per workgroup and class.
__global__ __launch_bounds__(CM_PAIR) void cls_pairs_kernel(const double* __restrict__ probs, const int64_t* __restrict__ labels,
                                                            long n, int K, unsigned long long* __restrict__ out) {
    __shared__ double s_p[CM_PAIR * CM_MAX_K];
    __shared__ int s_y[CM_PAIR];
    __shared__ unsigned long long s_c[4][CM_MAX_K];
    const int u = threadIdx.x;
    const long i = (long)blockIdx.x * CM_PAIR + u;
    int yi = -1;
    if (i < n) {
        const int64_t l = labels[i];
        if (l >= 0 && l < K) yi = (int)l;
    }
    const double pi = yi >= 0 ? probs[i * K + yi] : 0.0;
    if (u < 4 * CM_MAX_K) s_c[u / CM_MAX_K][u % CM_MAX_K] = 0ull;
    int wins = 0, ties = 0;
    const long tiles = (n + CM_PAIR - 1) / CM_PAIR;
    for (long jt = blockIdx.y; jt < tiles; jt += gridDim.y) {
        const long j0 = jt * CM_PAIR;
        const int rows = (int)(n - j0 < CM_PAIR ? n - j0 : CM_PAIR);
        __syncthreads();                        // the previous tile has been read (and s_c is zero)
        for (int e = u; e < rows * K; e += CM_PAIR) s_p[e] = probs[j0 * K + e];
        if (u < rows) {
            const int64_t l = labels[j0 + u];
            s_y[u] = (l >= 0 && l < K) ? (int)l : -1;
        }
        __syncthreads();
        if (yi >= 0) {
            for (int j = 0; j < rows; ++j) {
                const int yj = s_y[j];
                if (yj < 0 || yj == yi) continue;
                const double pj = s_p[j * K + yi];
                wins += pi > pj;
                ties += pi == pj;
            }
        }
    }
    __syncthreads();
    const int lane = u & 63;
    for (int k = 0; k < K; ++k) {
        // n_pos / n_neg come from the i-tiles alone: the workgroups of the first j-column count them
        int v[4] = {yi == k ? wins : 0, yi == k ? ties : 0, (blockIdx.y == 0 && yi == k) ? 1 : 0,
                    (blockIdx.y == 0 && yi >= 0 && yi != k) ? 1 : 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            for (int s = 32; s > 0; s >>= 1) v[q] += __shfl_down(v[q], s, 64);
            if (lane == 0 && v[q]) atomicAdd(&s_c[q][k], (unsigned long long)v[q]);
        }
    }
    __syncthreads();
    if (u < 4 * K) {
        const int q = u / K, k = u % K;
        if (s_c[q][k]) atomicAdd(&out[q * K + k], s_c[q][k]);
    }
}

extern "C" {

long mg_cls_eval_acc_words(int n_classes, int n_bins, int n_temps) {
    if (n_classes < 2 || n_classes > CM_MAX_K || n_bins < 1 || n_bins > CM_MAX_BINS || n_temps < 1 || n_temps > CM_MAX_G) return 0;
    return (long)n_classes * cls_block_words(n_classes, n_bins, n_temps);
}

size_t mg_cls_eval_acc_workspace_bytes(int B, int n_temps) {
    if (B < 1 || B > 32767 || n_temps < 1 || n_temps > CM_MAX_G) return 0;
    return (size_t)B * cls_work_words(n_temps) * sizeof(long long);
}

int mg_cls_eval_acc(const float* logits, const float* clean_logits, int B, int n_classes, const int64_t* labels, int n_bins,
                    const double* inv_temps, int n_temps, double inv_temperature, void* acc, double* probs, int32_t* row_i,
                    double* row_d, long dst_rows, const uint64_t* counter, const uint64_t* base, void* work, size_t work_bytes,
                    uint64_t* tick, mg_stream_t stream) {
    MG_CHECK_ARG(logits && labels && inv_temps && acc && probs && row_i && row_d && counter && base && work,
                 "mg_cls_eval_acc: null logits / labels / inv_temps / acc / probs / row_i / row_d / counter / base / work");
    MG_CHECK_ARG(B >= 1 && B <= 32767, "mg_cls_eval_acc: B = %d: must be in 1..32767", B);
    MG_CHECK_ARG(n_classes >= 2 && n_classes <= CM_MAX_K, "mg_cls_eval_acc: %d classes: 2..16", n_classes);
    MG_CHECK_ARG(n_bins >= 1 && n_bins <= CM_MAX_BINS, "mg_cls_eval_acc: n_bins = %d: 1..32", n_bins);
    MG_CHECK_ARG(n_temps >= 1 && n_temps <= CM_MAX_G, "mg_cls_eval_acc: %d inverse temperatures: 1..64", n_temps);
    MG_CHECK_ARG(inv_temperature > 0.0 && inv_temperature < 1e300, "mg_cls_eval_acc: inv_temperature must be positive and finite");
    cls_temps temps;
    for (int g = 0; g < CM_MAX_G; ++g) temps.inv[g] = 1.0;
    for (int g = 0; g < n_temps; ++g) {
        MG_CHECK_ARG(inv_temps[g] > 0.0 && inv_temps[g] < 1e300, "mg_cls_eval_acc: inv_temps[%d] must be positive and finite", g);
        temps.inv[g] = inv_temps[g];
    }
    MG_CHECK_ARG(dst_rows >= 1, "mg_cls_eval_acc: dst_rows must be positive");
    MG_CHECK_ARG((((uintptr_t)logits | (uintptr_t)clean_logits | (uintptr_t)row_i) & 3) == 0,
                 "mg_cls_eval_acc: logits, clean_logits and row_i must be 4-byte aligned");
    MG_CHECK_ARG((((uintptr_t)acc | (uintptr_t)probs | (uintptr_t)row_d | (uintptr_t)work | (uintptr_t)labels) & 7) == 0,
                 "mg_cls_eval_acc: labels, acc, probs, row_d and work must be 8-byte aligned");
    const size_t need = (size_t)B * cls_work_words(n_temps) * sizeof(long long);
    MG_CHECK_ARG(work_bytes >= need, "mg_cls_eval_acc: workspace of %zu bytes, %zu needed (mg_cls_eval_acc_workspace_bytes)",
                 work_bytes, need);
    hipLaunchKernelGGL(cls_rows_kernel, dim3((unsigned)B), dim3(CM_LANES), 0, ST, logits, clean_logits, labels, n_classes, n_bins,
                       temps, n_temps, inv_temperature, (long long*)work, probs, (int*)row_i, row_d, dst_rows,
                       (const unsigned long long*)counter, (const unsigned long long*)base);
    MG_CHECK_LAUNCH("cls_rows");
    hipLaunchKernelGGL(cls_fold_kernel, dim3((unsigned)mg_cdiv(cls_block_words(n_classes, n_bins, n_temps), CM_FOLD), (unsigned)n_classes),
                       dim3(CM_FOLD), 0, ST, (const long long*)work, labels, B, n_classes, n_bins, n_temps, (long long*)acc,
                       (unsigned long long*)tick);
    MG_CHECK_LAUNCH("cls_fold");
    return MG_OK;
}

int mg_cls_auroc_pairs(const double* probs, const int64_t* labels, long n, int n_classes, int64_t* out, mg_stream_t stream) {
    MG_CHECK_ARG(probs && labels && out, "mg_cls_auroc_pairs: null probs / labels / out");
    MG_CHECK_ARG(n >= 1 && n <= CM_MAX_N, "mg_cls_auroc_pairs: n = %ld: 1..131072 rows", n);
    MG_CHECK_ARG(n_classes >= 2 && n_classes <= CM_MAX_K, "mg_cls_auroc_pairs: %d classes: 2..16", n_classes);
    MG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)labels | (uintptr_t)out) & 7) == 0,
                 "mg_cls_auroc_pairs: probs, labels and out must be 8-byte aligned");
    hipLaunchKernelGGL(cls_zero_kernel, dim3(1), dim3(64), 0, ST, (long long*)out, (long)4 * n_classes);
    MG_CHECK_LAUNCH("cls_zero");
    const long tiles = mg_cdiv(n, CM_PAIR);
    hipLaunchKernelGGL(cls_pairs_kernel, dim3((unsigned)tiles, (unsigned)(tiles < 64 ? tiles : 64)), dim3(CM_PAIR), 0, ST, probs,
                       labels, n, n_classes, (unsigned long long*)out);
    MG_CHECK_LAUNCH("cls_pairs");
    return MG_OK;
}

}  // extern "C"
