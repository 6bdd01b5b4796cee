// The latent-mode emotion classifier's training step (MLPClassifier, reference src/emotion_discriminator/ed_model.py:72-95;
// the step of train_ed.py:51-82) as TWO launches on v_mfma_f32_16x16x4_f32 (exact fp32), include/melo_gan_hip.h:
//   A  mlp_rows_kernel    per-row half: a workgroup owns 16 rows; forward through every layer with the activations in LDS,
//                         cross-entropy, data gradients back to hidden layer 0.  The weights stream from L2 once per 16 rows
//                         (row_chain_kernel streams them once per ROW).
//   B  mlp_params_kernel  per-parameter half: a wave owns a 16 x 16 tile of one layer's weight (and, in the first tile column,
//                         16 bias elements), reduces it over the rows in row order and applies AdamW from registers.
// The kernel boundary is the one all-to-all seam (rows -> parameters): no workgroup waits for another inside a launch, no
// atomics, so reruns and graph replays give identical bits.
//
// MFMA operand maps (16x16x4, f32): lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and receives
// D[4 * (l >> 4) + reg][l & 15].  A 16-wide reduction chunk is fed as four MFMAs whose k-th slot holds element 4 * (l >> 4) + q
// of the chunk (q = 0..3: the MFMA), so that the LDS side is ONE 16-byte read per lane per chunk; any assignment of the
// chunk's elements to slots is valid as long as A and B agree.
#include "common.h"

namespace {

constexpr int MLP_ROWS = 16;          // rows of a block = the MFMA tile height
constexpr int MLP_THREADS = 512;
constexpr int MLP_WAVES = MLP_THREADS / 64;
constexpr int MLP_MAX_DIM = 512;
constexpr int MLP_MAX_CLASSES = 32;
constexpr int MLP_LAYERS = MG_MLP_MAX_HIDDEN + 1;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct MlpStage {
    const float* split_x; const int64_t* split_y; long src_rows; const int64_t* order; long order_len;
    const unsigned long long* base; int rule;
};

// four consecutive elements k..k+3 of row o of a (out, in) matrix; 0 outside it.  vec: rows are 16-byte aligned pieces.
__device__ __forceinline__ float4 ld_w4(const float* __restrict__ w, int o, int k, int out, int in, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < out && k < in) {
        const float* p = w + (long)o * in + k;
        if (vec) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (k + 1 < in) v.y = p[1];
            if (k + 2 < in) v.z = p[2];
            if (k + 3 < in) v.w = p[3];
        }
    }
    return v;
}

// acc[reg] = sum_k act[4 * (lane >> 4) + reg][k] * w[o0 + (lane & 15)][k]: one 16-column tile of act (16, in) x w^T.
// act: LDS, row stride S, zero up to the next multiple of 16 columns past `in`.
__device__ __forceinline__ f32x4 tile_fwd(const float* act, int S, const float* __restrict__ w, int o0, int out, int in, bool vec,
                                          int lane) {
    const int r = lane & 15, g = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int kpad = (in + 15) & ~15;
    const float* arow = act + r * S + 4 * g;
    for (int k0 = 0; k0 < kpad; k0 += 32) {
        const bool two = k0 + 16 < kpad;
        const float4 w0 = ld_w4(w, o0 + r, k0 + 4 * g, out, in, vec);
        const float4 w1 = two ? ld_w4(w, o0 + r, k0 + 16 + 4 * g, out, in, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a0 = *reinterpret_cast<const float4*>(arow + k0);
        const float4 a1 = two ? *reinterpret_cast<const float4*>(arow + k0 + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc0 = mfma4(a0.x, w0.x, acc0);
        acc1 = mfma4(a1.x, w1.x, acc1);
        acc0 = mfma4(a0.y, w0.y, acc0);
        acc1 = mfma4(a1.y, w1.y, acc1);
        acc0 = mfma4(a0.z, w0.z, acc0);
        acc1 = mfma4(a1.z, w1.z, acc1);
        acc0 = mfma4(a0.w, w0.w, acc0);
        acc1 = mfma4(a1.w, w1.w, acc1);
    }
    return acc0 + acc1;
}

// acc[reg] = sum_o d[4 * (lane >> 4) + reg][o] * w[o][j0 + (lane & 15)]: one 16-column tile of d (16, out) x w.
__device__ __forceinline__ f32x4 tile_bwd(const float* d, int S, const float* __restrict__ w, int j0, int out, int in, int lane) {
    const int r = lane & 15, g = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int opad = (out + 15) & ~15;
    const float* drow = d + r * S + 4 * g;
    const int j = j0 + r;
    const bool jok = j < in;
    for (int o0 = 0; o0 < opad; o0 += 16) {
        float wv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = o0 + 4 * g + q;
            wv[q] = jok && o < out ? w[(long)o * in + j] : 0.f;
        }
        const float4 a = *reinterpret_cast<const float4*>(drow + o0);
        acc0 = mfma4(a.x, wv[0], acc0);
        acc1 = mfma4(a.y, wv[1], acc1);
        acc0 = mfma4(a.z, wv[2], acc0);
        acc1 = mfma4(a.w, wv[3], acc1);
    }
    return acc0 + acc1;
}

__device__ __forceinline__ float drop_mask(long e, unsigned stream_id, unsigned long long step, unsigned long long seed, float p,
                                           float sc) {
    const long q = e >> 2;
    unsigned c[4] = {(unsigned)q, (unsigned)(q >> 32) ^ (stream_id << 28), (unsigned)step, (unsigned)(step >> 32)};
    philox4(c, (unsigned)seed, (unsigned)(seed >> 32));
    return u01(c[e & 3]) >= p ? sc : 0.f;
}

// ---- launch A -----------------------------------------------------------------------------------------------------------
// LDS (dynamic): two (16, S) activation planes that the layers ping-pong between, the block's source rows and logits.
__global__ __launch_bounds__(MLP_THREADS) void mlp_rows_kernel(const mg_mlp_cls N, int rows, float* __restrict__ x,
                                                               int64_t* __restrict__ y, const MlpStage sg, int train, int draw,
                                                               float p_drop, unsigned long long seed,
                                                               const unsigned long long* __restrict__ step_ctr, double* tick_state,
                                                               double beta1, double beta2, float* __restrict__ logits,
                                                               float* __restrict__ loss_rows, float* __restrict__ dlogits, int S) {
    // all of it dynamic: the 160 KiB opt-in (mg_lds_optin) is refused for a kernel that also holds static LDS
    extern __shared__ __align__(16) float smem[];
    float* cur = smem;
    float* nxt = smem + MLP_ROWS * S;
    long* srow = reinterpret_cast<long*>(smem + 2 * MLP_ROWS * S);                         // 16-byte aligned: S % 4 == 0
    float (*lg)[MLP_MAX_CLASSES + 1] = reinterpret_cast<float (*)[MLP_MAX_CLASSES + 1]>(srow + MLP_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int L = N.n_hidden, C = N.n_classes;
    const unsigned long long step = step_ctr ? step_ctr[0] : 0ull;

    if (tick_state && blockIdx.x == 0 && tid == 0) {
        if (tick_state[0] == 0.0) { tick_state[1] = 1.0; tick_state[2] = 1.0; }
        tick_state[0] += 1.0;
        tick_state[1] *= beta1;
        tick_state[2] *= beta2;
    }

    // the block's rows: from x / y, or staged from the split by the device cursor (and then written to x / y)
    if (sg.split_x) {
        if (tid < MLP_ROWS) {
            const int r = row0 + tid;
            long sr = 0;
            if (r < rows) {
                long pos;
                if (sg.rule == MG_STAGE_LAST) {
                    pos = sg.order_len - rows + r;
                } else {
                    const unsigned long long k = step - sg.base[0];
                    pos = (long)((k * (unsigned long long)rows + (unsigned long long)r) % (unsigned long long)sg.order_len);
                }
                sr = sg.order ? sg.order[pos] : pos;
                sr = sr < 0 ? 0 : (sr >= sg.src_rows ? sg.src_rows - 1 : sr);
                y[r] = sg.split_y[sr];
            }
            srow[tid] = sr;
        }
        __syncthreads();
    }
    {
        const int in = N.in_dim, kp = (in + 15) & ~15;
        for (int i = tid; i < MLP_ROWS * kp; i += MLP_THREADS) {
            const int rl = i / kp, k = i - rl * kp, r = row0 + rl;
            float v = 0.f;
            if (r < rows && k < in) {
                if (sg.split_x) {
                    v = sg.split_x[srow[rl] * in + k];
                    x[(long)r * in + k] = v;
                } else {
                    v = x[(long)r * in + k];
                }
            }
            cur[rl * S + k] = v;
        }
    }
    __syncthreads();

    // forward: hidden layers, then the head
    const int c16 = lane & 15, g4 = 4 * (lane >> 4);
    const float sc = 1.f / (1.f - p_drop);
    for (int l = 0; l <= L; ++l) {
        const int in = l == 0 ? N.in_dim : N.width[l - 1];
        const int out = l == L ? C : N.width[l];
        const float* w = N.w[l];
        const bool vec = (in & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
        const int ntiles = (out + 15) >> 4;
        for (int t = wave; t < ntiles; t += MLP_WAVES) {
            f32x4 acc = tile_fwd(cur, S, w, 16 * t, out, in, vec, lane);
            const int col = 16 * t + c16;
            const bool cok = col < out;
            const float bias = cok ? N.b[l][col] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = g4 + i, r = row0 + rl;
                const bool ok = cok && r < rows;
                const float zv = acc[i] + bias;
                if (l == L) {
                    if (cok) lg[rl][col] = zv;
                    if (ok) logits[(long)r * C + col] = zv;
                    continue;
                }
                const long e = (long)r * out + col;
                float av = mg_gelu(zv);
                if (train) {
                    float mk = 0.f;
                    if (ok) {
                        if (draw) {
                            mk = drop_mask(e, l < 2 ? (unsigned)l : (unsigned)l + 2u, step, seed, p_drop, sc);
                            N.mask[l][e] = mk;
                        } else {
                            mk = N.mask[l][e];
                        }
                    }
                    av *= mk;
                }
                if (ok) {
                    if (N.z[l]) N.z[l][e] = zv;
                    if (N.a[l]) N.a[l][e] = av;
                }
                nxt[rl * S + col] = ok ? av : 0.f;
            }
        }
        __syncthreads();
        float* t_ = cur; cur = nxt; nxt = t_;
    }

    // cross-entropy (mg_softmax_ce's arithmetic per row); d logits into `cur`, zero up to the next multiple of 16 columns
    if (tid < MLP_ROWS) {
        const int r = row0 + tid;
        const int cp = (C + 15) & ~15;
        if (r < rows) {
            const float* zr = lg[tid];
            float mx = zr[0];
            for (int j = 1; j < C; ++j) mx = fmaxf(mx, zr[j]);
            float se = 0.f;
            for (int j = 0; j < C; ++j) se += expf(zr[j] - mx);
            const float lse = mx + logf(se);
            const int64_t yy = y[r];
            const bool bad = yy < 0 || yy >= C;
            loss_rows[r] = bad ? __builtin_nanf("") : lse - zr[bad ? 0 : yy];
            if (train) {
                for (int j = 0; j < C; ++j) {
                    const float d = bad ? __builtin_nanf("") : (expf(zr[j] - lse) - (j == yy ? 1.f : 0.f)) / (float)rows;
                    dlogits[(long)r * C + j] = d;
                    cur[tid * S + j] = d;
                }
                for (int j = C; j < cp; ++j) cur[tid * S + j] = 0.f;
            }
        } else if (train) {
            for (int j = 0; j < cp; ++j) cur[tid * S + j] = 0.f;
        }
    }
    if (!train) return;
    __syncthreads();

    // backward: dz[l] = (dz[l + 1] x w[l + 1]) * GELU'(z[l]) * mask[l], l = L - 1 .. 0 (dz[L] = d logits)
    for (int l = L - 1; l >= 0; --l) {
        const int wd = N.width[l];
        const int out = l + 1 == L ? C : N.width[l + 1];
        const int ntiles = (wd + 15) >> 4;
        for (int t = wave; t < ntiles; t += MLP_WAVES) {
            f32x4 acc = tile_bwd(cur, S, N.w[l + 1], 16 * t, out, wd, lane);
            const int col = 16 * t + c16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = g4 + i, r = row0 + rl;
                const bool ok = col < wd && r < rows;
                const long e = ok ? (long)r * wd + col : 0;
                float v = 0.f;
                if (ok) {
                    v = acc[i] * mg_gelu_grad(N.z[l][e]);
                    v *= N.mask[l][e];
                    N.dz[l][e] = v;
                }
                if (l > 0) nxt[rl * S + col] = v;
            }
        }
        if (l > 0) __syncthreads();
        float* t_ = cur; cur = nxt; nxt = t_;
    }
}

// ---- launch B -----------------------------------------------------------------------------------------------------------
struct MlpUpd {
    int n_layers, rows;
    int out[MLP_LAYERS], in[MLP_LAYERS], tiles_i[MLP_LAYERS], tile_end[MLP_LAYERS];
    const float* dz[MLP_LAYERS];
    const float* ap[MLP_LAYERS];
    long w_off[MLP_LAYERS], b_off[MLP_LAYERS];
};
struct MlpAdam { float* p; float* m; float* v; const double* state; float lr, beta1, beta2, eps, wd; };

// adam_apply_kernel's update (small_kernels.hip) of one element, its gradient in a register
__device__ __forceinline__ void adam_elem(const MlpAdam& A, long i, float gi, float step_size, float bc2_sqrt) {
    float pi = A.p[i];
    if (A.wd != 0.f) pi *= (1.f - A.lr * A.wd);  // decoupled (AdamW)
    const float m0 = A.m[i], v0 = A.v[i];
    const float mi = m0 + (gi - m0) * (1.f - A.beta1);
    const float vi = v0 * A.beta2 + (1.f - A.beta2) * gi * gi;
    A.m[i] = mi;
    A.v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + A.eps;
    A.p[i] = pi - step_size * (mi / denom);
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int UPD_WAVES = 4;

__global__ __launch_bounds__(64 * UPD_WAVES) void mlp_params_kernel(const MlpUpd U, float* __restrict__ g, const MlpAdam A, int apply,
                                                                     const float* __restrict__ loss_rows, float* __restrict__ loss,
                                                                     const float* __restrict__ logits, int C,
                                                                     const int64_t* __restrict__ y, float* __restrict__ metrics,
                                                                     unsigned long long* rng_step) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * UPD_WAVES + wave;
    const int rows = U.rows;
    if (t < U.tile_end[U.n_layers - 1]) {
        int l = 0;
        while (t >= U.tile_end[l]) ++l;
        const int tl = t - (l ? U.tile_end[l - 1] : 0);
        const int to = tl / U.tiles_i[l], ti = tl - to * U.tiles_i[l];
        const int out = U.out[l], in = U.in[l];
        const int c = lane & 15, gq = lane >> 4;
        const int oa = 16 * to + c, ib = 16 * ti + c;      // this lane's A column (an output) and B column (an input)
        const bool oa_ok = oa < out, ib_ok = ib < in;
        const float* __restrict__ dz = U.dz[l] + (oa_ok ? oa : 0);
        const float* __restrict__ ap = U.ap[l] + (ib_ok ? ib : 0);
        const bool with_bias = ti == 0;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
        // rows in row order, four per MFMA; eight in flight
        for (int r0 = 0; r0 < rows; r0 += 8) {
            const int ra = r0 + gq, rb = r0 + 4 + gq;
            const float a0 = oa_ok && ra < rows ? dz[(long)ra * out] : 0.f;
            const float b0 = ib_ok && ra < rows ? ap[(long)ra * in] : 0.f;
            const float a1 = oa_ok && rb < rows ? dz[(long)rb * out] : 0.f;
            const float b1 = ib_ok && rb < rows ? ap[(long)rb * in] : 0.f;
            acc0 = mfma4(a0, b0, acc0);
            acc1 = mfma4(a1, b1, acc1);
            if (with_bias) {
                accb = mfma4(a0, 1.f, accb);
                accb = mfma4(a1, 1.f, accb);
            }
        }
        const f32x4 acc = acc0 + acc1;
        float step_size = 0.f, bc2_sqrt = 1.f;
        if (apply) {
            step_size = (float)((double)A.lr / (1.0 - A.state[1]));
            bc2_sqrt = (float)sqrt(1.0 - A.state[2]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 16 * to + 4 * gq + i;
            if (o < out && ib_ok) {
                const long e = U.w_off[l] + (long)o * in + ib;
                g[e] = acc[i];
                if (apply) adam_elem(A, e, acc[i], step_size, bc2_sqrt);
            }
            if (with_bias && c == 0 && o < out) {
                const long e = U.b_off[l] + o;
                g[e] = accb[i];
                if (apply) adam_elem(A, e, accb[i], step_size, bc2_sqrt);
            }
        }
    }
    if (blockIdx.x == 0 && wave == 0) {
        float ls = 0.f;
        if (lane == 0) {
            for (int r = 0; r < rows; ++r) ls += loss_rows[r];
            ls /= (float)rows;
            loss[0] = ls;
            if (rng_step) rng_step[0] += 1;       // the Philox step counter of the draws this update consumed
        }
        if (metrics) {                             // ed_metrics_acc_kernel's sums (small_kernels.hip)
            ls = __shfl(ls, 0, 64);
            float hits = 0.f;
            for (int r = lane; r < rows; r += 64) {
                const float* z = logits + (long)r * C;
                float mx = z[0];
                int am = 0;
                for (int j = 1; j < C; ++j) {
                    const float v = z[j];
                    if (v > mx || (isnan(v) && !isnan(mx))) { mx = v; am = j; }
                }
                hits += (long)am == y[r] ? 1.f : 0.f;
            }
            hits = wave_sum64(hits);
            if (lane == 0) {
                metrics[0] = __fadd_rn(metrics[0], __fmul_rn(ls, (float)rows));
                metrics[1] = __fadd_rn(metrics[1], hits);
            }
        }
    }
}

int check_net(const mg_mlp_cls* net, int rows, const char* who) {
    MG_CHECK_ARG(net, "%s: null net", who);
    MG_CHECK_ARG(net->n_hidden >= 1 && net->n_hidden <= MG_MLP_MAX_HIDDEN, "%s: n_hidden must be in 1..%d, got %d", who,
                 MG_MLP_MAX_HIDDEN, net->n_hidden);
    MG_CHECK_ARG(net->in_dim >= 1 && net->in_dim <= MLP_MAX_DIM, "%s: in_dim must be in 1..%d, got %d", who, MLP_MAX_DIM, net->in_dim);
    for (int l = 0; l < net->n_hidden; ++l)
        MG_CHECK_ARG(net->width[l] >= 1 && net->width[l] <= MLP_MAX_DIM, "%s: width[%d] must be in 1..%d, got %d", who, l, MLP_MAX_DIM,
                     net->width[l]);
    MG_CHECK_ARG(net->n_classes >= 2 && net->n_classes <= MLP_MAX_CLASSES, "%s: n_classes must be in 2..%d, got %d", who,
                 MLP_MAX_CLASSES, net->n_classes);
    MG_CHECK_ARG(rows >= 1 && rows <= (1 << 24), "%s: rows must be in 1..2^24, got %d", who, rows);
    return MG_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" {

int mg_mlp_cls_fwd_bwd(const mg_mlp_cls* net, int rows, float* x, int64_t* y, const float* split_x, const int64_t* split_y,
                       long src_rows, const int64_t* order, long order_len, const uint64_t* base, int rule, int train, int draw,
                       float p_drop, uint64_t seed, const uint64_t* step_counter, double* tick_state, float beta1, float beta2,
                       float* logits, float* loss_rows, float* dlogits, mg_stream_t stream) {
    if (int rc = check_net(net, rows, "mg_mlp_cls_fwd_bwd")) return rc;
    const int L = net->n_hidden;
    MG_CHECK_ARG(x && y && logits && loss_rows, "mg_mlp_cls_fwd_bwd: null x / y / logits / loss_rows");
    for (int l = 0; l <= L; ++l) MG_CHECK_ARG(net->w[l] && net->b[l], "mg_mlp_cls_fwd_bwd: null weight / bias of layer %d", l);
    if (train) {
        MG_CHECK_ARG(dlogits, "mg_mlp_cls_fwd_bwd: training needs dlogits");
        for (int l = 0; l < L; ++l)
            MG_CHECK_ARG(net->z[l] && net->a[l] && net->dz[l] && net->mask[l], "mg_mlp_cls_fwd_bwd: training needs z / a / dz / mask of "
                         "hidden layer %d", l);
        if (draw) {
            MG_CHECK_ARG(step_counter, "mg_mlp_cls_fwd_bwd: drawing the masks needs the step counter");
            MG_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "mg_mlp_cls_fwd_bwd: bad dropout probability");
        }
    } else {
        MG_CHECK_ARG(!draw && !tick_state, "mg_mlp_cls_fwd_bwd: eval mode draws no masks and ticks no optimiser");
    }
    MlpStage sg{};
    if (split_x) {
        MG_CHECK_ARG(split_y, "mg_mlp_cls_fwd_bwd: split_x and split_y go together");
        MG_CHECK_ARG(src_rows > 0, "mg_mlp_cls_fwd_bwd: src_rows must be positive");
        MG_CHECK_ARG(order_len > 0 && (order || order_len <= src_rows), "mg_mlp_cls_fwd_bwd: order_len must be positive (and within "
                     "the split when there is no order)");
        MG_CHECK_ARG(rule == MG_STAGE_BATCH || rule == MG_STAGE_LAST, "mg_mlp_cls_fwd_bwd: unknown position rule %d", rule);
        if (rule == MG_STAGE_BATCH) MG_CHECK_ARG(step_counter && base, "mg_mlp_cls_fwd_bwd: the batch rule needs counter and base");
        else MG_CHECK_ARG(rows <= order_len, "mg_mlp_cls_fwd_bwd: the last-rows rule needs rows <= order_len");
        sg = MlpStage{split_x, split_y, src_rows, order, order_len, (const unsigned long long*)base, rule};
    }
    int mx = net->in_dim > net->n_classes ? net->in_dim : net->n_classes;
    for (int l = 0; l < L; ++l) mx = net->width[l] > mx ? net->width[l] : mx;
    const int S = ((mx + 15) & ~15) + 4;          // + 4: rows start 4 banks apart (16-byte reads of 16 rows x 4 k-groups)
    const size_t lds = (size_t)2 * MLP_ROWS * S * sizeof(float) + MLP_ROWS * sizeof(long) + MLP_ROWS * (MLP_MAX_CLASSES + 1) * sizeof(float);
    static std::atomic<uint64_t> optin{0};
    if (int rc = mg_lds_optin(reinterpret_cast<const void*>(&mlp_rows_kernel), optin)) return rc;
    hipLaunchKernelGGL(mlp_rows_kernel, dim3((unsigned)mg_cdiv(rows, MLP_ROWS)), dim3(MLP_THREADS), lds, ST, *net, rows, x, y, sg,
                       train ? 1 : 0, draw ? 1 : 0, p_drop, (unsigned long long)seed, (const unsigned long long*)step_counter,
                       tick_state, (double)beta1, (double)beta2, logits, loss_rows, dlogits, S);
    MG_CHECK_LAUNCH("mlp_cls_fwd_bwd");
    return MG_OK;
}

int mg_mlp_cls_wgrad_update(const mg_mlp_cls* net, int rows, const float* x, const float* dlogits, const long* w_off,
                            const long* b_off, long n_flat, float* g, float* p, float* m, float* v, int apply, float lr,
                            float beta1, float beta2, float eps, float weight_decay, const double* state,
                            const float* loss_rows, float* loss, const float* logits, const int64_t* y, float* metrics,
                            uint64_t* rng_step, mg_stream_t stream) {
    if (int rc = check_net(net, rows, "mg_mlp_cls_wgrad_update")) return rc;
    const int L = net->n_hidden;
    MG_CHECK_ARG(x && dlogits && w_off && b_off && g && loss_rows && loss, "mg_mlp_cls_wgrad_update: null x / dlogits / offsets / g / "
                 "loss_rows / loss");
    MG_CHECK_ARG(!metrics || (logits && y), "mg_mlp_cls_wgrad_update: metrics need logits and y");
    if (apply) MG_CHECK_ARG(p && m && v && state, "mg_mlp_cls_wgrad_update: the update needs p / m / v / state");
    else MG_CHECK_ARG(!rng_step, "mg_mlp_cls_wgrad_update: the step counter advances with the update only");
    MlpUpd U{};
    U.n_layers = L + 1;
    U.rows = rows;
    long lo[2 * MLP_LAYERS], hi[2 * MLP_LAYERS];
    int tiles = 0;
    for (int l = 0; l <= L; ++l) {
        U.out[l] = l == L ? net->n_classes : net->width[l];
        U.in[l] = l == 0 ? net->in_dim : net->width[l - 1];
        U.dz[l] = l == L ? dlogits : net->dz[l];
        U.ap[l] = l == 0 ? x : net->a[l - 1];
        MG_CHECK_ARG(U.dz[l] && U.ap[l], "mg_mlp_cls_wgrad_update: null dz / a of layer %d", l);
        U.w_off[l] = w_off[l];
        U.b_off[l] = b_off[l];
        lo[2 * l] = w_off[l]; hi[2 * l] = w_off[l] + (long)U.out[l] * U.in[l];
        lo[2 * l + 1] = b_off[l]; hi[2 * l + 1] = b_off[l] + U.out[l];
        U.tiles_i[l] = (U.in[l] + 15) >> 4;
        tiles += ((U.out[l] + 15) >> 4) * U.tiles_i[l];
        U.tile_end[l] = tiles;
    }
    for (int i = 0; i < 2 * (L + 1); ++i) {
        MG_CHECK_ARG(lo[i] >= 0 && hi[i] <= n_flat, "mg_mlp_cls_wgrad_update: tensor %d lies outside the flat buffer", i);
        for (int j = 0; j < i; ++j)
            MG_CHECK_ARG(hi[j] <= lo[i] || hi[i] <= lo[j], "mg_mlp_cls_wgrad_update: tensors %d and %d overlap in the flat buffer", j, i);
    }
    const MlpAdam A{p, m, v, state, lr, beta1, beta2, eps, weight_decay};
    hipLaunchKernelGGL(mlp_params_kernel, dim3((unsigned)mg_cdiv(tiles, UPD_WAVES)), dim3(64 * UPD_WAVES), 0, ST, U, g, A, apply ? 1 : 0,
                       loss_rows, loss, logits, net->n_classes, y, metrics, (unsigned long long*)rng_step);
    MG_CHECK_LAUNCH("mlp_cls_wgrad_update");
    return MG_OK;
}

}  // extern "C"
