// Held-out evaluation of a trained GAN (melo_gan_amd/gan/evaluate.py): the metrics of one evaluated batch added to a
// device-resident accumulator that lives for the whole pass, and the pass's noise keyed by the split row.  The layouts and
// the reference lines these answer to are in include/melo_gan_hip.h (mg_eval_acc, mg_eval_noise).
#include "common.h"

#define ST ((hipStream_t)stream)

// ---------------- accumulator layout (8-byte words; include/melo_gan_hip.h) ----------------
struct EvalLayout {
    long n, conf_fake, conf_real;                       // int64 section
    long d_sum, cls, nsum, nsq;                         // fp64 section
    long minmax;                                        // fp32 section (word offset; 4 K C floats behind it)
    long words;
};
static inline EvalLayout eval_layout(int K, int C) {
    EvalLayout L;
    L.n = 0;
    L.conf_fake = K;
    L.conf_real = L.conf_fake + (long)K * K;
    L.d_sum = L.conf_real + (long)K * K;
    L.cls = L.d_sum + 2;                                // [side][{ce, p}][K]
    L.nsum = L.cls + 4L * K;                            // [side][K][C]
    L.nsq = L.nsum + 2L * K * C;
    L.minmax = L.nsq + 2L * K * C;                      // floats: min [side][K][C], then max [side][K][C]
    L.words = L.minmax + 2L * K * C;
    return L;
}

// ---------------- launch geometry of the statistics pass ----------------
// A workgroup takes one row and one chunk of its time axis.  Lane t reads 16 bytes: channel quad t % Lq of time position
// t / Lq of the iteration (C = 4: one position per lane; C = 128: 32 lanes per position).
constexpr int EV_THREADS = 256;
constexpr int EV_UNROLL = 4;             // iterations whose loads are issued together
constexpr int EV_TARGET_BLOCKS = 512;    // about two workgroups per CU
struct EvalPlan { int Lq, ppi, iters, nchunks; };
static inline EvalPlan eval_plan(int B, int T, int C) {
    EvalPlan P;
    P.Lq = C / 4;
    P.ppi = EV_THREADS / P.Lq;
    const int total = (int)mg_cdiv(T, P.ppi);
    int want = EV_TARGET_BLOCKS / B;
    want = want < 1 ? 1 : (want > total ? total : want);
    P.iters = (int)mg_cdiv(total, want);
    P.nchunks = (int)mg_cdiv(total, P.iters);
    return P;
}
static inline size_t eval_work_bytes(int B, int T, int C) {
    const EvalPlan P = eval_plan(B, T, C);
    return (size_t)B * P.nchunks * 4 * C * (sizeof(double) + sizeof(float));
}

__device__ __forceinline__ int eval_argmax(const float* z, int K) {      // first index wins, NaN counts as the maximum
    float mx = z[0];
    int am = 0;
    for (int j = 1; j < K; ++j) {
        const float v = z[j];
        if (v > mx || (isnan(v) && !isnan(mx))) { mx = v; am = j; }
    }
    return am;
}

// The per-row metrics of the batch, one workgroup: counts and confusion by integer atomics, the fp64 sums by one owner
// thread each, over the rows in row order -- reruns and replays add bit-identical sums.
__device__ void eval_rows_block(const int64_t* __restrict__ labels, const float* __restrict__ d_real,
                                const float* __restrict__ d_fake, const float* __restrict__ logits_fake,
                                const float* __restrict__ logits_real, int B, int K, long long* __restrict__ acc_i,
                                double* __restrict__ acc_d, const EvalLayout L, unsigned long long* tick) {
    __shared__ int s_t[EV_THREADS];
    __shared__ double s_v[6][EV_THREADS];      // ce fake, p fake, ce real, p real, d_real, d_fake
    const int u = threadIdx.x;
    // owner threads: u < 4 K: value u / K of class u % K; u = 4 K, 4 K + 1: the critic sums
    double own = 0.0;
    for (int r0 = 0; r0 < B; r0 += EV_THREADS) {
        const int r = r0 + u;
        int t = -1;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (r < B) {
            const int64_t y = labels[r];
            t = (y >= 0 && y < K) ? (int)y : -1;
            if (t >= 0) {
                atomicAdd((unsigned long long*)&acc_i[L.n + t], 1ull);
                for (int side = 0; side < 2; ++side) {
                    const float* lg = side ? logits_real : logits_fake;
                    if (!lg) continue;
                    const float* z = lg + (long)r * K;
                    const int am = eval_argmax(z, K);
                    atomicAdd((unsigned long long*)&acc_i[(side ? L.conf_real : L.conf_fake) + (long)t * K + am], 1ull);
                    // mg_softmax_ce's max-subtracted log-sum-exp, evaluated in fp64
                    float mx = z[0];
                    for (int j = 1; j < K; ++j) mx = fmaxf(mx, z[j]);
                    double se = 0.0;
                    for (int j = 0; j < K; ++j) se += exp((double)z[j] - (double)mx);
                    const double zt = (double)z[t] - (double)mx;
                    v[2 * side] = log(se) - zt;
                    v[2 * side + 1] = exp(zt) / se;
                }
                if (d_real) { v[4] = (double)d_real[r]; v[5] = (double)d_fake[r]; }
            }
        }
        s_t[u] = t;
#pragma unroll
        for (int q = 0; q < 6; ++q) s_v[q][u] = v[q];
        __syncthreads();
        const int n = min(EV_THREADS, B - r0);
        if (u < 4 * K) {
            const int k = u % K, q = u / K;
            for (int i = 0; i < n; ++i)
                if (s_t[i] == k) own += s_v[q][i];
        } else if (u < 4 * K + 2) {
            const int q = 4 + (u - 4 * K);
            for (int i = 0; i < n; ++i)
                if (s_t[i] >= 0) own += s_v[q][i];
        }
        __syncthreads();
    }
    if (u < 4 * K) {
        const int k = u % K, q = u / K;            // q: 0 ce fake, 1 p fake, 2 ce real, 3 p real
        if ((q < 2 && logits_fake) || (q >= 2 && logits_real)) acc_d[L.cls + (long)q * K + k] += own;
    } else if (u < 4 * K + 2) {
        if (d_real) acc_d[L.d_sum + (u - 4 * K)] += own;
    }
    if (u == 0 && tick) tick[0] += 1ull;
}

// Pass 1.  blockIdx.y < B: the note statistics of (row blockIdx.y, time chunk blockIdx.x) of both sides, reduced over the
// workgroup by a fixed tree and written to this workgroup's slab entry (every entry is written, padding rows with the
// identities).  blockIdx.y == B: the per-row metrics (one workgroup).
__global__ __launch_bounds__(EV_THREADS) void eval_stats_kernel(
    const float* __restrict__ real, const float* __restrict__ fake, const int64_t* __restrict__ labels, int B, int T, int C,
    int K, const EvalPlan P, double* __restrict__ slab_d, float* __restrict__ slab_f, const float* __restrict__ d_real,
    const float* __restrict__ d_fake, const float* __restrict__ logits_fake, const float* __restrict__ logits_real,
    long long* __restrict__ acc_i, double* __restrict__ acc_d, const EvalLayout L, unsigned long long* tick) {
    if ((int)blockIdx.y == B) {
        if (blockIdx.x == 0) eval_rows_block(labels, d_real, d_fake, logits_fake, logits_real, B, K, acc_i, acc_d, L, tick);
        return;
    }
    __shared__ double sh_d[16][EV_THREADS];      // [side * 8 + {sum, sumsq} * 4 + j]
    __shared__ float sh_f[16][EV_THREADS];       // [side * 8 + {min, max} * 4 + j]
    const int b = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int cg = t % P.Lq, pl = t / P.Lq;
    const bool active = pl < P.ppi;
    const int64_t y = labels[b];
    const bool counted = y >= 0 && y < K;
    double sd[16];
    float sf[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        sd[q] = 0.0;
        sf[q] = (q & 4) ? -INFINITY : INFINITY;
    }
    if (counted && active) {
        const float* base[2] = {real + (long)b * T * C + 4 * cg, fake + (long)b * T * C + 4 * cg};
        const int pos0 = chunk * P.iters * P.ppi + pl;
        for (int it0 = 0; it0 < P.iters; it0 += EV_UNROLL) {
            f32x4 x[EV_UNROLL][2];
            bool ok[EV_UNROLL];
#pragma unroll
            for (int i = 0; i < EV_UNROLL; ++i) {
                const int pos = pos0 + (it0 + i) * P.ppi;
                ok[i] = it0 + i < P.iters && pos < T;
                const long off = (long)(ok[i] ? pos : 0) * C;      // position 0 always exists
                x[i][0] = *reinterpret_cast<const f32x4*>(base[0] + off);
                x[i][1] = *reinterpret_cast<const f32x4*>(base[1] + off);
            }
#pragma unroll
            for (int i = 0; i < EV_UNROLL; ++i) {
                if (!ok[i]) continue;
#pragma unroll
                for (int side = 0; side < 2; ++side)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = x[i][side][j];
                        const double dv = (double)v;
                        sd[side * 8 + j] += dv;
                        sd[side * 8 + 4 + j] += dv * dv;
                        sf[side * 8 + j] = fminf(sf[side * 8 + j], v);
                        sf[side * 8 + 4 + j] = fmaxf(sf[side * 8 + 4 + j], v);
                    }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        sh_d[q][t] = sd[q];
        sh_f[q][t] = sf[q];
    }
    __syncthreads();
    int p2 = 1;
    while (p2 < P.ppi) p2 <<= 1;
    for (int s = p2 >> 1; s > 0; s >>= 1) {
        if (active && pl < s && pl + s < P.ppi) {
            const int o = (pl + s) * P.Lq + cg;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                sh_d[q][t] += sh_d[q][o];
                sh_f[q][t] = (q & 4) ? fmaxf(sh_f[q][t], sh_f[q][o]) : fminf(sh_f[q][t], sh_f[q][o]);
            }
        }
        __syncthreads();
    }
    if (t < P.Lq) {      // pl == 0: channel quad t
        const long blk = (long)b * gridDim.x + chunk;
        double* od = slab_d + blk * 4 * C;       // [side][{sum, sumsq}][C]
        float* of = slab_f + blk * 4 * C;        // [side][{min, max}][C]
#pragma unroll
        for (int side = 0; side < 2; ++side)
#pragma unroll
            for (int kind = 0; kind < 2; ++kind)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    od[(side * 2 + kind) * C + 4 * t + j] = sh_d[side * 8 + kind * 4 + j][t];
                    of[(side * 2 + kind) * C + 4 * t + j] = sh_f[side * 8 + kind * 4 + j][t];
                }
    }
}

// Pass 2, the fixed-order fold.  Workgroup (column block, class k): lane (col, q) adds the slab entries q, q + 32, ... of
// the rows labelled k for column col of [side][C], the 32 q-lanes are reduced by a fixed tree, and the owner lane adds the
// result to the accumulator.
constexpr int FOLD_COLS = 32, FOLD_Q = 32;
__global__ __launch_bounds__(FOLD_COLS * FOLD_Q) void eval_fold_kernel(
    const double* __restrict__ slab_d, const float* __restrict__ slab_f, const int64_t* __restrict__ labels, int B, int C,
    int K, int nchunks, double* __restrict__ acc_d, float* __restrict__ acc_f, const EvalLayout L) {
    __shared__ double sh_s[FOLD_Q][FOLD_COLS], sh_q[FOLD_Q][FOLD_COLS];
    __shared__ float sh_mn[FOLD_Q][FOLD_COLS], sh_mx[FOLD_Q][FOLD_COLS];
    const int col = threadIdx.x % FOLD_COLS, q = threadIdx.x / FOLD_COLS;
    const int j = blockIdx.x * FOLD_COLS + col, k = blockIdx.y;
    const bool live = j < 2 * C;
    const int side = live ? j / C : 0, c = live ? j % C : 0;
    double s = 0.0, sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    const long nblk = (long)B * nchunks;
    if (live)
        for (long blk = q; blk < nblk; blk += FOLD_Q) {
            if (labels[blk / nchunks] != (int64_t)k) continue;
            const double* pd = slab_d + blk * 4 * C + (long)side * 2 * C + c;
            const float* pf = slab_f + blk * 4 * C + (long)side * 2 * C + c;
            s += pd[0];
            sq += pd[C];
            mn = fminf(mn, pf[0]);
            mx = fmaxf(mx, pf[C]);
        }
    sh_s[q][col] = s; sh_q[q][col] = sq; sh_mn[q][col] = mn; sh_mx[q][col] = mx;
    __syncthreads();
    for (int st = FOLD_Q / 2; st > 0; st >>= 1) {
        if (q < st) {
            sh_s[q][col] += sh_s[q + st][col];
            sh_q[q][col] += sh_q[q + st][col];
            sh_mn[q][col] = fminf(sh_mn[q][col], sh_mn[q + st][col]);
            sh_mx[q][col] = fmaxf(sh_mx[q][col], sh_mx[q + st][col]);
        }
        __syncthreads();
    }
    if (q == 0 && live) {
        const long o = ((long)side * K + k) * C + c;
        acc_d[L.nsum + o] += sh_s[0][col];
        acc_d[L.nsq + o] += sh_q[0][col];
        float* fmin_ = acc_f + 2 * L.minmax;
        float* fmax_ = fmin_ + 2L * K * C;
        fmin_[o] = fminf(fmin_[o], sh_mn[0][col]);
        fmax_[o] = fmaxf(fmax_[o], sh_mx[0][col]);
    }
}

__global__ void eval_reset_kernel(long long* acc, const EvalLayout L, int K, int C) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L.minmax) acc[i] = 0;
    const long nf = 2L * K * C;
    float* f = reinterpret_cast<float*>(acc + L.minmax);
    if (i < nf) {
        f[i] = INFINITY;
        f[nf + i] = -INFINITY;
    }
}

// Evaluation noise: one workgroup per batch row, Philox counter (element block, EVAL_TAG, split row lo, split row hi).
constexpr unsigned EVAL_TAG = 0x4556414Cu;      // apart from mg_rng_fill (< 0x40000000), mg_stage_augment (0x415547xx), mg_gen_inputs (0x47454Exx)
__global__ __launch_bounds__(64) void eval_noise_kernel(float* __restrict__ noise, int rows, int noise_dim,
                                                        const unsigned long long* __restrict__ counter,
                                                        const unsigned long long* __restrict__ base, unsigned long long n,
                                                        unsigned long long seed) {
    const int r = blockIdx.x;
    const unsigned long long i = (counter[0] - base[0]) * (unsigned long long)rows + (unsigned long long)r;
    const bool pad = i >= n;
    for (int qb = threadIdx.x; qb < (noise_dim + 3) >> 2; qb += blockDim.x) {
        unsigned c[4] = {(unsigned)qb, EVAL_TAG, (unsigned)i, (unsigned)(i >> 32)};
        philox4(c, (unsigned)seed, (unsigned)(seed >> 32));
        float v[4];
        box_muller4(c, v);       // csrc/common.h
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * qb + j;
            if (col < noise_dim) noise[(long)r * noise_dim + col] = pad ? 0.f : v[j];
        }
    }
}

extern "C" {

long mg_eval_acc_words(int n_classes, int C) {
    if (n_classes < 1 || n_classes > 32 || C < 4 || C > 1024 || C % 4) return 0;
    return eval_layout(n_classes, C).words;
}

size_t mg_eval_acc_workspace_bytes(int B, int T, int C) {
    if (B < 1 || B > 65534 || T < 1 || C < 4 || C > 1024 || C % 4) return 0;
    return eval_work_bytes(B, T, C);
}

int mg_eval_acc_reset(void* acc, int n_classes, int C, mg_stream_t stream) {
    MG_CHECK_ARG(acc && ((uintptr_t)acc & 7) == 0, "mg_eval_acc_reset: acc must be an 8-byte aligned device pointer");
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32 && C >= 4 && C <= 1024 && C % 4 == 0,
                 "mg_eval_acc_reset: 1..32 classes, C a multiple of 4 in 4..1024");
    const EvalLayout L = eval_layout(n_classes, C);
    hipLaunchKernelGGL(eval_reset_kernel, dim3((unsigned)mg_cdiv(L.words, 256)), dim3(256), 0, ST, (long long*)acc, L, n_classes, C);
    MG_CHECK_LAUNCH("eval_reset");
    return MG_OK;
}

int mg_eval_acc(const float* real, const float* fake, int B, int T, int C, const int64_t* emot_idx, const float* d_real,
                const float* d_fake, const float* logits_fake, const float* logits_real, int n_classes, void* acc, void* work,
                size_t work_bytes, uint64_t* tick, mg_stream_t stream) {
    MG_CHECK_ARG(real && fake && emot_idx && acc && work, "mg_eval_acc: null real / fake / emot_idx / acc / work");
    MG_CHECK_ARG(B >= 1 && B <= 65534 && T >= 1, "mg_eval_acc: B must be in 1..65534 and T positive");
    MG_CHECK_ARG(C >= 4 && C <= 1024 && C % 4 == 0, "mg_eval_acc: C must be a multiple of 4 in 4..1024 (16-byte loads)");
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32, "mg_eval_acc: 1..32 classes");
    MG_CHECK_ARG((d_real == nullptr) == (d_fake == nullptr), "mg_eval_acc: d_real and d_fake go together");
    MG_CHECK_ARG((((uintptr_t)real | (uintptr_t)fake) & 15) == 0, "mg_eval_acc: real and fake must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)acc | (uintptr_t)work) & 7) == 0, "mg_eval_acc: acc and work must be 8-byte aligned");
    MG_CHECK_ARG((long)B * T * C < (1L << 40), "mg_eval_acc: batch too large");
    const EvalPlan P = eval_plan(B, T, C);
    const size_t need = eval_work_bytes(B, T, C);
    if (work_bytes < need) {
        mg_set_error("mg_eval_acc: workspace of %zu bytes, %zu needed (mg_eval_acc_workspace_bytes)", work_bytes, need);
        return MG_EWORK;
    }
    const EvalLayout L = eval_layout(n_classes, C);
    double* slab_d = static_cast<double*>(work);
    float* slab_f = reinterpret_cast<float*>(slab_d + (size_t)B * P.nchunks * 4 * C);
    hipLaunchKernelGGL(eval_stats_kernel, dim3((unsigned)P.nchunks, (unsigned)B + 1), dim3(EV_THREADS), 0, ST, real, fake,
                       emot_idx, B, T, C, n_classes, P, slab_d, slab_f, d_real, d_fake, logits_fake, logits_real,
                       (long long*)acc, (double*)acc, L, (unsigned long long*)tick);
    MG_CHECK_LAUNCH("eval_stats");
    hipLaunchKernelGGL(eval_fold_kernel, dim3((unsigned)mg_cdiv(2 * C, FOLD_COLS), (unsigned)n_classes), dim3(FOLD_COLS * FOLD_Q),
                       0, ST, (const double*)slab_d, (const float*)slab_f, emot_idx, B, C, n_classes, P.nchunks, (double*)acc,
                       (float*)acc, L);
    MG_CHECK_LAUNCH("eval_fold");
    return MG_OK;
}

int mg_eval_noise(float* noise, int rows, int noise_dim, const uint64_t* counter, const uint64_t* base, long n, uint64_t seed,
                  mg_stream_t stream) {
    MG_CHECK_ARG(noise && counter && base && rows > 0 && rows <= 65535 && noise_dim > 0 && n > 0,
                 "mg_eval_noise: need noise, counter and base, 1..65535 rows, a positive noise_dim and split length");
    hipLaunchKernelGGL(eval_noise_kernel, dim3((unsigned)rows), dim3(64), 0, ST, noise, rows, noise_dim,
                       (const unsigned long long*)counter, (const unsigned long long*)base, (unsigned long long)n,
                       (unsigned long long)seed);
    MG_CHECK_LAUNCH("eval_noise");
    return MG_OK;
}

}  // extern "C"
