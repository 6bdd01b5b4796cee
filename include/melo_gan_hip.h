/*
 * melo_gan_hip.h -- C-ABI of libmelogan_hip.so (gfx950 / MI355X).
 *
 * The reference (kaushik87599/Melo-GAN) has no FFI: its hot path is a set of
 * torch.nn modules (ATen ops).  Each entry point below replaces the ATen op(s)
 * that the cited reference lines dispatch; the host side (melo-gan_amd/) calls
 * them through ctypes with raw device pointers owned by PyTorch's allocator.
 *
 * Conventions
 *   - All tensors are fp32, CHANNELS-LAST: activations (B, T, C) contiguous in C
 *     (the layout of the reference's `notes` tensors; the reference permutes to
 *     (B, C, T) for torch's Conv1d -- src/gan/models.py:159, ed_model.py:65 --
 *     this library never does).
 *   - Weights keep the reference's state_dict layouts: Conv1d (Cout, Cin, K),
 *     ConvTranspose1d (Cin, Cout, K), Linear (out, in).
 *   - Every function enqueues on `stream` (a hipStream_t) and returns without
 *     synchronising.  No allocation, no retained pointers.
 *   - Return 0 on success; <0 on error: -1 bad argument/shape, -2 unsupported
 *     configuration, -3 workspace too small, -4 HIP runtime error.  The message is
 *     available from mg_last_error() (thread-local).
 */
#ifndef MELO_GAN_HIP_H
#define MELO_GAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mg_stream_t; /* hipStream_t */

/* activation ids (epilogue `act`, and `gact` = which derivative to apply) */
enum { MG_ACT_NONE = 0, MG_ACT_RELU = 1, MG_ACT_LRELU = 2, MG_ACT_GELU = 3, MG_ACT_TANH = 4 };

/* Fused epilogue of the window-GEMM kernels.  For an output element v=acc:
 *   v += bias[n];  v = v*scale[n] + shift[n];  zout[idx] = v;  v = act(v);
 *   v *= act'(gref[idx]) (gact);  v *= emul[idx];  v *= gscale[n];
 *   y = accumulate ? y + v : v
 * Null pointers skip the corresponding stage.  gref semantics per gact:
 *   RELU  : gref is the forward OUTPUT a (mask a>0)
 *   LRELU : gref is the forward output a (a>0 ? 1 : 0.2)
 *   GELU  : gref is the forward PRE-activation z (exact erf form)
 *   TANH  : gref is the forward output a (1 - a*a)
 */
typedef struct mg_epilogue {
    const float* bias;
    const float* scale;
    const float* shift;
    float* zout;
    int act;
    const float* gref;
    int gact;
    const float* emul;
    const float* gscale;
    int accumulate;
} mg_epilogue;

int mg_version(void);
const char* mg_last_error(void);

/* ---- window GEMM: Conv1d / ConvTranspose1d / Linear, forward and data-gradient ----
 *
 * mg_conv1d_gather: y[b,t,n] = EPI( sum_{k,c} x[b, t*stride + k - (K-1)/2, c] * W(n,c,kw) )
 *   kw = flip ? K-1-k : k ;  W(n,c,k) = w[n*w_sn + c*w_sc + k].
 *   Tout = (Tin + 2*((K-1)/2) - K)/stride + 1.   stride in {1,2}, K in {1,3,5}.
 *   Replaces: nn.Conv1d forward (src/gan/models.py:141-145, ed_model.py:28, src/ae/model.py:11-19)
 *             with w_sn=Cin*K, w_sc=K;  nn.Linear forward (K=1,T=1; w_sn=in, w_sc=1);
 *             ConvTranspose1d data-gradient (stride 2; w_sn=Cout*K, w_sc=K);
 *             Conv1d stride-1 data-gradient (flip=1; w_sn=K, w_sc=Cin*K);
 *             Linear data-gradient (K=1; w_sn=1, w_sc=in).
 *   x batch stride xbs, y batch stride ybs (elements; 0 => dense).
 *   work/work_bytes: optional scratch (mg_conv_workspace_bytes(B, Tout, N)); when given and the output
 *   tiling alone would leave most CUs idle, the channel reduction is split over workgroups into partial
 *   slabs that a second kernel sums in fixed order before the epilogue.  NULL => never split.
 *   lds_pad: 0..120 KiB of extra LDS per workgroup, i.e. fewer resident workgroups per CU (ignored where it would take
 *   the launch past 160 KiB, and by the thin route).  For a branch that runs on a side stream beside the step's critical
 *   path (the frozen emotion discriminator): its 1024-workgroup convolutions otherwise fill every CU's registers and the
 *   critical path's small dependent kernels wait for their workgroups to retire.  0: the default occupancy.
 */
size_t mg_conv_workspace_bytes(int B, int Tout, int N);
int mg_conv1d_gather(const float* x, const float* w, float* y,
                     int B, int Tin, int Cin, int N, int K, int stride, int flip,
                     int w_sn, int w_sc, long xbs, long ybs,
                     const mg_epilogue* epi, void* work, size_t work_bytes, long lds_pad, mg_stream_t stream);

/* mg_conv1d_scatter2: stride-2, K=5, padding 2, output_padding 1 transposed convolution
 *   y[b,t,n] = EPI( sum_{k,c : t+2-k even} x[b,(t+2-k)/2,c] * W(n,c,k) ),  t < Tout,
 *   Tout = 2*Tin (ConvTranspose1d forward) or 2*Tin-1 (data-gradient of a stride-2 Conv1d whose
 *   input length was odd).
 *   Replaces: nn.ConvTranspose1d forward (src/gan/models.py:56-62, src/ae/model.py:66-74)
 *             with w_sn=K, w_sc=Cout*K;  Conv1d stride-2 data-gradient (src/gan/models.py:141-145
 *             backward; w_sn=K... i.e. n=Cin: w_sn=K, w_sc=Cin*K).
 */
int mg_conv1d_scatter2(const float* x, const float* w, float* y,
                       int B, int Tin, int Cin, int N, int Tout,
                       int w_sn, int w_sc, long xbs, long ybs,
                       const mg_epilogue* epi, void* work, size_t work_bytes, mg_stream_t stream);

/* ---- the stride-2, 5-tap window GEMMs on 16x16x4 MFMA tiles (csrc/conv16_mfma.hip) ----
 * The same arithmetic as mg_conv1d_gather(stride 2, K 5) [transposed = 0: nn.Conv1d(k5,s2,p2) forward,
 * src/gan/models.py:141-145, src/ae/model.py:11-19; nn.ConvTranspose1d data-gradient] and mg_conv1d_scatter2
 * [transposed = 1: nn.ConvTranspose1d(k5,s2,p2,op1) forward, src/gan/models.py:56-62; Conv1d stride-2 data-gradient,
 * Tout = 2*Tin or 2*Tin-1] in 64x32 / 32x32 output tiles with the whole channel reduction inside each workgroup: no
 * split-K workspace, no second launch, bitwise run-to-run reproducible.  Weights in the WQ layout
 *     wq[((c/4)*5 + k)*N + n][c%4] = W(n, c, k)        (N output columns, c reduction channel, Cin % 16 == 0, N % 32 == 0)
 * which mg_wq_relayout derives from a reference-layout tensor (W(n,c,k) = w[n*w_sn + c*w_sc + k]) and mg_adam_flat's table
 * keeps current after every optimiser step.  mg_conv16_supported tells whether a shape is covered (else use the calls above). */
int mg_wq_relayout(const float* w, float* wq, int N, int Cc, int K, int w_sn, int w_sc, mg_stream_t stream);
int mg_conv16_supported(int B, int Tin, int Cin, int N, int transposed, int Tout);
int mg_conv16_plan(int B, int Tin, int N, int transposed, int* batch_rows_per_tile, int* part_rows, int* tile_rows);
int mg_conv16_poolable(int B, int Tin, int Cin, int N);
/* ONE launch, with any of these riders (extra = NULL, or a zeroed field: none):
 *   part:   per-column partial statistics of the values v the launch stores, so that the train-mode BatchNorm that follows
 *           needs no reduction pass of its own: for every (tile, wave row) p and column n
 *             part[p][0][n] = sum_rows v[row, n],   [1][n] = sum_rows (v - mean_p)^2 about that wave's OWN mean,   [2][n] = rows summed
 *           (combined by the parallel-variance rule in fp64: nothing is formed as E[x^2] - mean^2).
 *           part: 3 * part_rows * N floats; part_rows and the batch rows a tile spans from mg_conv16_plan (a caller that stacks
 *           several BatchNorm groups along the batch needs the group size to be a multiple of batch_rows_per_tile).
 *           mg_bn_train_fwd_parts finishes the statistics (fixed order, fp64), moves the running ones and applies, all in ONE
 *           launch: the semantics of mg_bn_train_fwd (nn.BatchNorm1d training forward, src/gan/models.py:57-61).  The
 *           statistics of an accumulating launch (epi->accumulate) are not defined: refused.
 *   pool:   the temporal mean of what the launch stores -- AdaptiveAvgPool1d(1) behind the critic's last convolution
 *           (src/gan/models.py:148): pool[b][n] = pool_scale * sum_t y[b][t][n].  Gather form only; mg_conv16_poolable says
 *           whether a shape qualifies (every sample's time axis is one wave's rows of a tile: Tout = 32, or 16 with 32-row
 *           tiles).  The mean of an accumulating launch is not defined: refused.
 *   y_perm: the permuted output order y[b*ybs + n*Tout + tout] -- the (B, N*Tout) order behind the reference's
 *           `view(B, 256, L)` (src/gan/models.py:70), so the data-gradient of the first deconvolution lands in decoder.pre.2's
 *           output order with no transpose launch (zout / gref / emul keep the dense (b, tout, n) index);
 *   mix_*:  the gradient penalty's interpolate (src/gan/utils.py:76-79): for batch rows b < mix_rows ALSO
 *             mix_out[i] = mix_alpha[b] * mix_real[i] + (1 - mix_alpha[b]) * y[i]   at the element's y index i. */
typedef struct mg_conv16_extra {
    float* part;
    float* pool;
    float pool_scale;
    int y_perm;
    const float* mix_real;
    const float* mix_alpha;
    float* mix_out;
    int mix_rows;
    /* bnb_*: the launch's output y is the gradient that reaches a train-mode BatchNorm + ReLU / LeakyReLU layer from above
     * (src/gan/models.py:57-61 backwards); with that layer's forward tensors a, z (laid out like y) and saved statistics it also
     * leaves bnb_part[p][0][n] = sum_rows g, [1][n] = sum_rows g * x_hat (g = y * act'(a), x_hat = (z - mean) * invstd; p, rows
     * as for `part`: 2 * part_rows * N DOUBLES, accumulated in fp64 like the reduction pass they replace), so the BatchNorm's
     * backward is ONE launch, mg_bn_train_bwd_parts */
    const float* bnb_a;
    const float* bnb_z;
    const float* bnb_mean;
    const float* bnb_invstd;
    double* bnb_part;
    int bnb_act;
} mg_conv16_extra;
int mg_conv16(const float* x, const float* wq, float* y, int B, int Tin, int Cin, int N, int transposed, int Tout,
              long xbs, long ybs, const mg_epilogue* epi, const mg_conv16_extra* extra /* may be NULL */, mg_stream_t stream);
/* mg_bn_train_bwd behind a conv16 launch that left the two column sums (bnb_part, part_rows rows of 2 x C doubles): the sums
 * are added in row order and the gradient applied -- one launch. */
int mg_bn_train_bwd_parts(const double* part, int part_rows, const float* da, const float* a, const float* z, float* dz, long R,
                          int C, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                          float* dgamma, float* dbeta, int act, mg_stream_t stream);
int mg_bn_train_fwd_parts(const float* part, int part_rows_per_group, int groups, const float* z, float* a, long R, int C,
                          const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                          float eps, float* save_mean, float* save_invstd, int act, mg_stream_t stream);

/* ---- row chains (csrc/row_chain.hip): a sample's small layer stack as ONE launch -- one workgroup walks one row through
 *      an op list with the activations in LDS vector slots (MG_CHAIN_SLOTS slots of MG_CHAIN_MAX_VEC floats).  Used for the
 *      numeric encoder (LayerNorm + 3 Linear, src/gan/feature_encoder.py:16-45) forward and data-gradient, the emotion
 *      classifier's tail (ed_model.py:61,86-95,147-165: project, MLP, head, cross-entropy and their data-gradients) and the
 *      critic's tail (src/gan/models.py:149-169: fc, scoring head and their data-gradients).  Row r of every global operand
 *      is at ptr + r * ld.  Ops (fields not named are ignored):
 *   LOAD       slot b [n1, n1+n0) (+= if i0) p0 row (r % i1 if i1 > 0)
 *   COPY       slot b [n1, n1+n0) = slot a [i1, i1+n0)
 *   STORE      q0 row <- slot a [0,n0)
 *   MEAN_T     slot b [0,n0) = mean over t < i0 of p0[(r*i0 + t)*ld0 + c]  (AdaptiveAvgPool1d(1) of a (rows, i0, ld0) tensor); q0 rows <- it
 *   LAYERNORM  slot b = LN(slot a [0,n0<=64)) * p0 + p1, eps f0; q0 rows <- xhat, q1 rows <- output (optional)
 *   LIN_FWD    slot b [0,n1) = act(slot a [0,n0) W^T + p1) * p2 row;  W(n,k) = p0[n*ld0 + k];  q0 rows <- pre-activation,
 *              q1 rows <- output (optional)                                              (nn.Linear forward + act + dropout mask)
 *   LIN_DGRAD  slot b [0,n1) = (slot a [0,n0) W) * act'(p1 row) * p2 row;  W(o,i) = p0[o*ld0 + i];  q1 rows <- output
 *   SOFTMAX_CE slot a = logits [0,n0<=32), t0 = int64 targets: q0[r] = -log softmax[target];  slot b = f0 * (softmax - onehot)
 *              (F.cross_entropy forward + backward per row; an out-of-range target poisons the row with NaN)
 *   DHEAD      critic head on slot a = f [0,n0): q0[r] = f . w[0,n0) + emb row (r % i1) . w[n0, n0+n1) + p1[0], w = p0, emb = p2;
 *              slot b = p3[r] * w[0,n0) * lrelu'(f);  q1 rows <- p3[r] * w[n0, n0+n1)       (src/gan/models.py:160-169 + backward)
 */
#define MG_CHAIN_MAX_OPS 16
#define MG_CHAIN_SLOTS 6
#define MG_CHAIN_MAX_VEC 512
enum { MG_CH_LOAD = 1, MG_CH_STORE = 2, MG_CH_LAYERNORM = 3, MG_CH_LIN_FWD = 4, MG_CH_LIN_DGRAD = 5, MG_CH_SOFTMAX_CE = 6,
       MG_CH_DHEAD = 7, MG_CH_MEAN_T = 8, MG_CH_COPY = 9 };
typedef struct mg_chain_op {
    int kind;
    int a, b;
    int n0, n1;
    int act;
    int i0, i1;
    float f0;
    const float* p0; long ld0;
    const float* p1; long ld1;
    const float* p2; long ld2;
    const float* p3; long ld3;
    float* q0; long lq0;
    float* q1; long lq1;
    const int64_t* t0;
} mg_chain_op;
int mg_row_chain(const mg_chain_op* ops, int n_ops, int rows, mg_stream_t stream);
/* out[0] = scale * mean(src[0..n)) (one block): the loss scalar behind a chain's per-row cross-entropy terms */
int mg_mean_scaled(const float* src, float* out, int n, float scale, mg_stream_t stream);
/* dst[0] = the device's constant-rate clock (wall_clock64, 100 MHz) when the node runs: a time stamp inside a captured graph
 * (measurement only: tools/step_stamps.py) */
int mg_stamp(unsigned long long* dst, mg_stream_t stream);

/* ---- skinny GEMM for nn.Linear forward / data-gradient with few rows (M = batch) ----
 *   y[M,N] = EPI( x[M,K] @ W^T ),  W(n,c) = w[n*w_sn + c*w_sc], one of the strides must be 1:
 *   nn.Linear forward (src/gan/models.py:24-26,47-49,151; feature_encoder.py:23,38; ed_model.py:61,78,90):
 *       w (out,in): w_sn = in, w_sc = 1;   data-gradient dx = dy @ w: w_sn = 1, w_sc = in(=N).
 *   Deep K is split over workgroups into partial slabs in `work` (mg_linear_workspace_bytes, may be 0). */
size_t mg_linear_workspace_bytes(int M, int N, int K);
/* perm_L > 1: the OUTPUT COLUMNS PERMUTED: column n' of y is weight row (n' % C) * perm_L + n' / C, C = N / perm_L (bias,
 * scale, gscale follow the weight row; zout / gref / emul the stored order): y comes out as the channels-last (M, perm_L, C)
 * tensor the reference reaches by `view(B, 256, L)` + permute(0, 2, 1) on the way into the first ConvTranspose1d
 * (src/gan/models.py:70-73) -- no transpose launch.  perm_L = 0: the reference's column order. */
int mg_linear(const float* x, const float* w, float* y, int M, int K, int N, int w_sn, int w_sc,
              const mg_epilogue* epi, int perm_L, void* work, size_t work_bytes, mg_stream_t stream);
/* Host only: what mg_linear launches for these arguments (the same decision function).  Returns 0: the 64x64-tile window
 * GEMM conv_wgemm_kernel<1,1,false,true,TM,TN> (the permuted forward with many rows and columns; MG_LINEAR_SKINNY_ONLY=1
 * disables that route), 1: linear_skinny_kernel<*kcontig, *vec>, followed by linear_finish_kernel when *ksplit > 1;
 * negative: an argument error.  x_aligned / w_aligned: whether the pointer is 16-byte aligned. */
int mg_linear_route(int M, int K, int N, int w_sn, int w_sc, int perm_L, int x_aligned, int w_aligned,
                    int* kcontig, int* vec, int* ksplit);

/* ---- stride-1 three-tap Conv1d (padding 1) by minimal filtering F(2,3) along time (csrc/conv_wino.hip) ----
 * Same result as mg_conv1d_gather(K = 3, stride = 1) up to rounding (the operands are transformed: a few ulp), with 2/3 of
 * its matrix-pipe work: four channel GEMMs per PAIR of outputs instead of six.  For the frozen emotion discriminator's
 * conv1-3 and their input gradients (src/emotion_discriminator/ed_model.py:24-46 inside src/gan/train_gan.py:228-236).
 *   mg_wino3_weights: wt[Cin/4][4][N][4] = the filter transform of g_k = W(n, c, flip ? 2-k : k), W(n,c,k) = w[n*w_sn + c*w_sc + k]
 *                     (forward: w (N,Cin,3), w_sn = 3 Cin, w_sc = 3; data gradient of a Conv1d whose weight is (Cout,Cin,3):
 *                     N = Cin, "Cin" = Cout, w_sn = 3, w_sc = 3 Cin_conv, flip = 1).  Cin % 4 == 0.
 *   mg_conv1d_wino3:  y[b,t,n] = EPI( sum_{k,c} x[b, t+k-1, c] * g_k(n,c) ), x (B,T,Cin) and y (B,T,N) dense, 16-byte aligned;
 *                     T even, Cin % 16 == 0, N % 64 == 0 (mg_conv1d_wino3_supported).  lds_pad: as for mg_conv1d_gather. */
int mg_conv1d_wino3_supported(int B, int T, int Cin, int N);
int mg_wino3_weights(const float* w, float* wt, int N, int Cin, long w_sn, long w_sc, int flip, mg_stream_t stream);
int mg_conv1d_wino3(const float* x, const float* wt, float* y, int B, int T, int Cin, int N, const mg_epilogue* epi,
                    long lds_pad, mg_stream_t stream);
/* mg_wino3_weights for several filters in ONE launch (a network in training transforms all its layers' weights, forward and
 * data-gradient images, at the top of every step: emotion_discriminator/engine.py) */
#define MG_MAX_WINO_WJOBS 8
typedef struct mg_wino3_wjob {
    const float* w;
    float* wt;
    int N, Cin;
    long w_sn, w_sc;
    int flip;
} mg_wino3_wjob;
int mg_wino3_weights_multi(const mg_wino3_wjob* jobs, int n_jobs, mg_stream_t stream);

/* Which instantiation of conv_wgemm_kernel<S,K,TR2,TM,TN> a call launches: TM*10+TN (22: 128x128 tile,
 * 12: 64x128, 11: 64x64).  m_rows = B*Tout (gather) or B*Tin (scatter2).  Lets a profiler label
 * launches by kernel symbol. */
int mg_conv_tile_config(long m_rows, int N, int scatter2);
/* Host only: the split of the channel reduction a window-GEMM call plans (the planner mg_conv1d_gather / mg_conv1d_scatter2
 * launch with; MG_SPLITK_TARGET read per call).  Tm = the rows the time tiling covers (Tout for gather, Tin for scatter2),
 * work_bytes = the workspace the call would be given (0: none).  *ksplit = blockIdx.z slabs (> 1: conv_finish_kernel sums
 * them and runs the epilogue), *cps = channel chunks (16 channels; 64 for K = 1) per slab.  Calls that route to the thin
 * kernels (mg_conv_thin_route) do not use this plan. */
int mg_conv_plan(int B, int Tm, int Tout, int N, int Cin, int K, int stride, int scatter2, size_t work_bytes,
                 int* ksplit, int* cps);
/* Host only: which conv_finish_kernel<VEC> a split launch is followed by (the launch's own predicate): 1 = the 16-byte one,
 * 0 = the scalar one.  ybs = the batch stride of y in elements; tensors_aligned = the workspace, y and every elementwise
 * epilogue tensor given (zout, gref, emul) start on a 16-byte boundary. */
int mg_conv_finish_vec(int N, long ybs, int tensors_aligned);

/* The layers with a <= 8 channel reduction or output side (NOTE_DIM = 4, reference config/gan_config.yaml:43-44: critic
 * conv.0 src/gan/models.py:129, generator deconv.6 src/gan/models.py:67-70, emotion discriminator conv0
 * src/emotion_discriminator/ed_model.py:24, the VAE's first / last layer) do not run on the MFMA tile kernels:
 * mg_conv1d_gather / mg_conv1d_scatter2 route them to VALU kernels (csrc/conv_thin.hip).  This reports the route a call
 * takes: 0 = MFMA tile kernel, 1 = thin_in_kernel, 2 / 3 = thin_out_kernel<TR2, 4 / 8>.  MG_CONV_THIN=0 disables it. */
int mg_conv_thin_route(const float* x, long xbs, int Cin, int N, int K, int stride, int transposed);

/* ---- bf16-storage / fp32-accumulate variant of the frozen emotion-discriminator branch (SECONDARY configuration) ----
 * The branch (src/gan/train_gan.py:228-236: ED(generated) -> cross-entropy -> gradient w.r.t. the generated notes;
 * src/emotion_discriminator/ed_model.py:24-69) has no trained parameters in the GAN step, so it can store activations and
 * its folded weights in bf16 without touching optimiser state.  Products accumulate in fp32 (v_mfma_f32_32x32x16_bf16),
 * epilogue arithmetic is fp32.  Never the default; bench.py reports it as a separate line.
 *
 * mg_epilogue_bf16: v = acc; v = v*scale[n] + shift[n]; zout[di] = bf16(v); v = act(v); v *= act'(gact, gref[di]);
 *                   v *= gscale[n]; y = accumulate ? y + v : v (accumulate: fp32 y only).  zout / gref are bf16 tensors.
 * mg_wb_relayout:   wb[k][n][c] = bf16(w[n*w_sn + c*w_sc + (flip ? K-1-k : k)])  -- the weight image of the kernel below
 *                   (forward: w_sn = Cin*K, w_sc = K; stride-1 data gradient: flip = 1, w_sn = K, w_sc = Cin*K).
 * mg_conv1d_s1_bf16: y[b,t,n] = EPI( sum_{k,c} x[b, t + k - (K-1)/2, c] * wb[k][n][c] ), K in {3,5}; x is bf16 or (x_f32)
 *                   fp32 converted on the way into LDS; y is bf16 or (y_f32) fp32.  Needs T % 128 == 0, Cin % 32 == 0,
 *                   N % 64 == 0 (mg_conv1d_s1_bf16_supported), dense 16-byte aligned tensors (x, wb, y, zout, gref: a
 *                   misaligned one is refused before the launch).
 * mg_meanT_fwd_bf16 / mg_meanT_bwd_bf16: the temporal mean (ed_model.py:65) over a bf16 activation and its backward
 *                   fused with act'(gref) * gscale, writing a bf16 gradient (C % 8 == 0, dz / gref 16-byte aligned). */
typedef struct mg_epilogue_bf16 {
    const float* scale;
    const float* shift;
    void* zout;
    int act;
    const void* gref;
    int gact;
    const float* gscale;
    int accumulate;
} mg_epilogue_bf16;
int mg_wb_relayout(const float* w, void* wb, int N, int Cc, int K, int w_sn, int w_sc, int flip, mg_stream_t stream);
int mg_conv1d_s1_bf16_supported(int B, int T, int Cin, int N, int K);
int mg_conv1d_s1_bf16(const void* x, int x_f32, const void* wb, void* y, int y_f32, int B, int T, int Cin, int N, int K,
                      const mg_epilogue_bf16* epi, mg_stream_t stream);
int mg_meanT_fwd_bf16(const void* a, float* h, int B, int T, int C, mg_stream_t stream);
int mg_meanT_bwd_bf16(const float* dh, void* dz, const void* gref, int gact, const float* gscale, int B, int T, int C,
                      mg_stream_t stream);

/* ---- weight gradient ----
 * out[a][b][k] = sum over segments, batches, u of  S[bt,u,a] * L[bt, u*stride + k - (K-1)/2, b]
 *   S: (nb, Ts, A) "small" tensor, L: (nb, Tl, Bc) "large" tensor (zero outside [0,Tl)).
 *   Conv1d   wgrad: S=dy (A=Cout), L=x  (Bc=Cin)  -> (Cout,Cin,K)
 *   ConvT1d  wgrad: S=x  (A=Cin),  L=dy (Bc=Cout) -> (Cin,Cout,K)
 *   Linear   wgrad: Ts=Tl=1,K=1: S=dy (A=out), L=x (Bc=in) -> (out,in)
 * Up to two (S,L,nb) segments are summed (segment 1 may have nb1=0).
 * Fused bias gradient (optional): bias_from = 1 -> bias_out[a] = sum of S over segment 0's rows (Conv1d / Linear
 * bias); bias_from = 2 -> bias_out[b] = sum of L over segment 0's rows (ConvTranspose1d bias); 0/NULL -> none.
 * `work` must hold mg_wgrad_workspace_bytes(...) bytes.  Deterministic (no atomics).
 */
size_t mg_wgrad_workspace_bytes(int A, int Bc, int K, int nb_total, int Ts);
int mg_wgrad(const float* s0, const float* l0, int nb0,
             const float* s1, const float* l1, int nb1,
             float* out, float* bias_out, int bias_from, int Ts, int Tl, int A, int Bc, int K, int stride,
             void* work, size_t work_bytes, mg_stream_t stream);

/* Several independent weight gradients of ONE (K, stride) in one launch (+ one reduce launch if any of them is split):
 * the small layers' gradients are each a few workgroups at the launch floor.  Each job has the meaning of one
 * mg_wgrad call; `work` must hold the SUM over jobs of mg_wgrad_workspace_bytes(A, Bc, K, nb0 + nb1, Ts), each rounded
 * up to 256 bytes.  Outputs of different jobs must not overlap. */
#define MG_MAX_WGRAD_JOBS 8
typedef struct mg_wgrad_job {
    const float* s0; const float* l0; int nb0;
    const float* s1; const float* l1; int nb1;
    float* out; float* bias_out; int bias_from;
    int Ts, Tl, A, Bc;
} mg_wgrad_job;
int mg_wgrad_multi(const mg_wgrad_job* jobs, int n_jobs, int K, int stride, void* work, size_t work_bytes,
                   mg_stream_t stream);

/* ---- per-channel column reductions over rows of a (R, C) matrix ----
 * sum[c] = sum_r x[r,c] (and sumsq if sumsq != NULL).  Used for bias gradients and BN statistics.
 * `work`: mg_colsum_workspace_bytes(C). */
size_t mg_colsum_workspace_bytes(int C);
int mg_colsum(const float* x, long R, int C, float* sum, float* sumsq,
              void* work, size_t work_bytes, mg_stream_t stream);

/* ---- BatchNorm1d, training mode, fused with ReLU (src/gan/models.py:57-61, src/ae/model.py:12-21) ----
 * z: (R, C) pre-BN (R = B*T).  Computes batch mean / biased var, a = relu((z-mean)*invstd*gamma+beta),
 * saves mean/invstd, updates running_mean/var (momentum 0.1, unbiased var) -- also under no_grad.
 * act: any MG_ACT_* (the generator uses RELU, the emotion discriminator's pre-training GELU).
 * `groups` independent batches of R rows each, stacked along the rows of z / a (the generator forward of the critic step and
 * of the generator step run as one 2B-row pass: src/gan/train_gan.py:186-189 and :216-219 use the same generator weights):
 * batch statistics per group (save_mean / save_invstd: (groups, C)), running statistics updated group after group -- what
 * consecutive forward calls do.  groups = 1: one plain forward.  `work`: mg_bn_workspace_bytes(C, groups). */
size_t mg_bn_workspace_bytes(int C, int groups);
int mg_bn_train_fwd(const float* z, float* a, long R, int C, int groups, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* save_mean, float* save_invstd, int act,
                    void* work, size_t work_bytes, mg_stream_t stream);
/* backward: da (grad wrt a), a (forward output: the ReLU / LeakyReLU mask, tanh'), z.  Produces dz, dgamma, dbeta.
 * beta: only read for act = MG_ACT_GELU, whose derivative is taken at the BN output (recomputed from z); else may be NULL.
 * `work`: mg_bn_workspace_bytes(C, 1). */
int mg_bn_train_bwd(const float* da, const float* a, const float* z, float* dz, long R, int C,
                    const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                    float* dgamma, float* dbeta, int act,
                    void* work, size_t work_bytes, mg_stream_t stream);
/* eval mode: a = act((z-running_mean)/sqrt(running_var+eps)*gamma+beta) */
int mg_bn_eval_fwd(const float* z, float* a, long R, int C, const float* gamma, const float* beta,
                   const float* running_mean, const float* running_var, float eps, int act,
                   mg_stream_t stream);
/* fold eval-mode BN + conv bias into per-channel scale/shift (ed_model.py:37, eval mode) */
int mg_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               const float* conv_bias, float eps, float* scale, float* shift, int C, mg_stream_t stream);

/* ---- mean over time (AdaptiveAvgPool1d(1); src/gan/models.py:148, ed_model.py:60) ---- */
int mg_meanT_fwd(const float* a, float* h, int B, int T, int C, mg_stream_t stream);
/* dz[b,t,c] = dh[b,c]/T * act'(gref[b,t,c]) * gscale[c]   (gref/gscale may be NULL).
 * mean_out != NULL: a scalar mean rides in the same launch (one extra block): mean_out[0] = mean_scale * mean(mean_src[0..mean_n))
 * -- the generator's adversarial loss -mean(D(fake)), src/gan/train_gan.py:224. */
int mg_meanT_bwd(const float* dh, float* dz, int B, int T, int C, const float* gref, int gact, const float* gscale,
                 const float* mean_src, float* mean_out, int mean_n, float mean_scale, mg_stream_t stream);

/* ---- LayerNorm over the last dim (src/gan/feature_encoder.py:19), D <= 64 ---- */
int mg_layernorm_fwd(const float* x, float* y, float* xhat, int B, int D,
                     const float* gamma, const float* beta, float eps, mg_stream_t stream);
int mg_layernorm_bwd_params(const float* dy, const float* xhat, float* dgamma, float* dbeta,
                            int B, int D, mg_stream_t stream);

/* ---- critic head (src/gan/models.py:157,165-169): s[b] = <[f[b], emb[b % Be]], w> + bias ---- */
int mg_dhead_fwd(const float* f, const float* emb, const float* w, const float* bias, float* s,
                 int B, int Be, int F, int E, mg_stream_t stream);
/* dU[b,j] = ds[b]*w[j]*lrelu'(f[b,j]); demb[be,j] (+)= sum over b%Be==be of ds[b]*w[F+j] (if demb) */
int mg_dhead_bwd(const float* ds, const float* f, const float* w, float* dU, float* demb,
                 int B, int Be, int F, int E, int nb_emb, mg_stream_t stream);
/* mg_dhead_fwd and mg_dhead_bwd in one launch: ds is a constant of the step, so the backward does not wait for s. */
int mg_dhead_fwd_bwd(const float* ds, const float* f, const float* emb, const float* w, const float* bias, float* s,
                     float* dU, float* demb, int B, int Be, int F, int E, int nb_emb, mg_stream_t stream);
/* dw[j<F] = sum_{b<nb} ds[b] f[b,j] + sum_{b<ng} gf[b,j];  dw[F+j] = sum_{b<nb} ds[b] emb[b%Be,j];
 * dbias = sum_{b<nb} ds[b].
 * loss_out != NULL: the critic's loss scalars (src/gan/train_gan.py:196-199, logging only) ride in the same launch (one extra
 * block), from the scores s (2 * nb_loss: real rows, then fake) and the per-sample gradient norms of mg_gp_penalty:
 *   gp_out[0] = mean((norms-1)^2) ;  loss_out = {mean fake - mean real + lambda_gp * gp_out[0], mean real, mean fake} */
int mg_dhead_wgrad(const float* ds, const float* f, const float* emb, const float* gf, float* dw, float* dbias,
                   int nb, int ng, int Be, int F, int E, const float* s, const float* norms, float lambda_gp,
                   float* loss_out, float* gp_out, int nb_loss, mg_stream_t stream);

/* ---- WGAN-GP pieces (src/gan/utils.py:75-90) ---- */
/* xhat[b,:] = alpha[b]*real[b,:] + (1-alpha[b])*fake[b,:]   (n = T*C elements per sample) */
int mg_gp_interp(const float* real, const float* fake, const float* alpha, float* xhat,
                 int B, long n, mg_stream_t stream);
/* norms[b] = ||g[b,:]||_2 ; gp = mean((norm-1)^2) ; gbar[b,:] = coef*(2/B)*(norm-1)/norm * g[b,:]
 * gp may be NULL: the mean is then left to mg_dhead_wgrad's loss rider (one launch fewer) */
int mg_gp_penalty(const float* g, float* gbar, float* norms, float* gp, float coef,
                  int B, long n, mg_stream_t stream);

/* ---- losses ---- */
/* cross entropy over C<=32 classes: loss = mean_b(-log softmax[b,y_b]); dlogits = coef*(softmax-onehot)/B */
int mg_softmax_ce(const float* logits, const int64_t* target, float* loss, float* dlogits,
                  float coef, int B, int C, mg_stream_t stream);

/* ---- elementwise helpers ---- */
int mg_axpby(const float* x, float* y, float a, float b, long n, mg_stream_t stream); /* y = a*x + b*y */
/* dst[r, doff + j] = src[r, soff + j] for j < ncols (row-major 2-D copy; accumulate adds) */
int mg_copy_cols(const float* src, int sld, int soff, float* dst, int dld, int doff,
                 int rows, int ncols, int accumulate, mg_stream_t stream);
/* (B, C, L) <-> (B, L, C): out[b, l, c] = in[b, c, l]  (src/gan/models.py:70 view + :73 permute); with gref (laid
 * out like `out`) the result is multiplied by act'(gref): the activation backward of the layer behind the view. */
int mg_transpose_bcl_blc(const float* in, float* out, int B, int C, int L, const float* gref, int gact,
                         mg_stream_t stream);
/* y = x * act'(gref) * emul   (standalone epilogue pieces for tiny tensors) */
int mg_act_bwd(const float* dy, const float* gref, int gact, const float* emul, float* dx, long n,
               mg_stream_t stream);

/* ---- batch staging (the device side of the DataLoader collate + .to(device) of src/gan/train_gan.py:80,172-178):
 *      for every job, dst row r <- src row (idx ? idx[r] : r) for r < n_rows, ALL jobs in one launch.  Rows are
 *      row_bytes long (a multiple of 4; 16-byte aligned rows take the 16-byte path); dst rows are dst_pitch bytes
 *      apart (0: dense), so a job can also fill a column block of a wider matrix.  idx is a
 *      device array of n_rows int64 indices, clamped into [0, src_rows) on the device (an out-of-range index never
 *      reads outside the source). */
/* ---- spectral normalisation of a weight (torch.nn.utils.spectral_norm, dim 0, n_power_iterations 1, eps 1e-12) ----
 * The reference wraps the emotion discriminator's Conv1d / Linear layers in it when `use_spectral_norm` is set
 * (src/emotion_discriminator/ed_model.py:29-32,79-82; FeatureEncoder(use_sn): src/gan/feature_encoder.py:24-31).
 * weight_mat = w_orig as (rows = out, cols = everything else).  One launch serves several layers.
 *   mg_spectral_norm_fwd: power_iterations = 1 (training forward): v = normalize(W^T u), u = normalize(W v), in place;
 *                         then (also with 0 = eval) sigma = u . (W v) and w_eff = w_orig / sigma.
 *   mg_spectral_norm_bwd: dw (the gradient w.r.t. w_eff, in place) <- (dw - <dw, w_eff> u v^T) / sigma = the gradient w.r.t.
 *                         w_orig (u, v constants, as autograd sees them). */
#define MG_MAX_SN_JOBS 8
typedef struct mg_sn_job {
    const float* w_orig;
    float* w_eff;
    float* u;       /* (rows) */
    float* v;       /* (cols) */
    float* sigma;   /* (1) */
    float* dw;      /* bwd only */
    int rows, cols;
} mg_sn_job;
int mg_spectral_norm_fwd(const mg_sn_job* jobs, int n_jobs, int power_iterations, float eps, mg_stream_t stream);
int mg_spectral_norm_bwd(const mg_sn_job* jobs, int n_jobs, mg_stream_t stream);

#define MG_MAX_STAGE_JOBS 8
typedef struct mg_stage_job {
    const void* src;
    void* dst;
    const int64_t* idx; /* NULL: straight copy of the first n_rows rows */
    long row_bytes;
    long src_rows;
    long dst_pitch;     /* bytes between destination rows; 0 = row_bytes */
    long rows;          /* rows of THIS job (<= n_rows); 0 = n_rows */
} mg_stage_job;
int mg_stage_rows(const mg_stage_job* jobs, int n_jobs, int n_rows, mg_stream_t stream);
/* The same with the source rows picked on the DEVICE: row r of every job comes from position
 *   p = ((counter[0] - base[0]) * n_rows + r) mod order_len   of the epoch's order (order[p]; NULL = the identity),
 * i.e. batch number (counter - base) of an HBM-resident split's shuffled order (the DataLoader's sampler,
 * src/gan/train_gan.py:80) -- so that a captured training step stages its own batch on every replay, with no host launch
 * between steps.  counter is advanced by another launch of the step (the Philox step counter doubles as batch counter);
 * the host writes `order` and `base` once per epoch.  Jobs carry no idx / rows of their own. */
int mg_stage_rows_cursor(const mg_stage_job* jobs, int n_jobs, int n_rows, const int64_t* order, long order_len,
                         const uint64_t* counter, const uint64_t* base, mg_stream_t stream);

/* ---- the classifier's / VAE's training data plane: stage a batch AND augment it in one pass ----
 * mg_stage_augment does mg_stage_rows_cursor's work for one notes array (src_rows, T, note_dim) fp32 and, when labels is not
 * NULL, its int64 label array, and applies one augmentation program to the notes on the way through registers (no second
 * pass, no intermediate buffer).  Row r of the batch comes from order[p] (order NULL: p), with p by `rule`:
 *   MG_STAGE_BATCH  p = ((counter[0] - base[0]) * n_rows + r) mod order_len    batch number (counter - base) of n_rows
 *   MG_STAGE_LAST   p = order_len - n_rows + r                                 the fixed last n_rows positions (the trailing
 *                                                                              partial batch; counter / base may be NULL)
 * Capturable: a replay stages the batch the counter then names.
 *   MG_AUG_ED (src/emotion_discriminator/ed_dataset.py:299-314, in its order): noise_std > 0: columns 1, 2, 3 of every time
 *     row += noise_std * N(0,1); dropout_prob > 0: a time row is kept with probability 1 - p, else ALL its columns become 0;
 *     pitch_shift_prob > 0: per sample, with that probability, column 0 of every row += +1 or -1 (equal odds; dropped rows too).
 *   MG_AUG_AE (src/ae/dataset.py:11-38,89-104): five per-sample gates with odds 0.3 / 0.3 / 0.2 / 0.3 / 0.2, in order: columns
 *     1, 2 *= 1 + U(-tempo_jitter, tempo_jitter) (one factor per sample: 1 + (2u - 1) * tempo_jitter in fp32, the product and
 *     the sum each rounded on its own); column 0 += randint(-pitch_shift, pitch_shift)
 *     (inclusive); time rows dropped with probability note_dropout; column 3 += N(0, velocity_jitter); column 1 +=
 *     N(0, timing_jitter) then max(., 0) -- the last two also on dropped rows.  (The reference's nan_to_num is a no-op on
 *     finite input and is not restated.)
 *   A parameter of 0 switches its step off; with all of them 0 the output is a plain copy, bit for bit.
 * Random numbers: Philox4x32-10, key = seed, counter = (t, 0x41554700 | need, serial lo, serial hi) with
 *   serial = (serial_base ? serial_base[0] : 0) + p   -- the trainer sets serial_base = epoch index * split size, so serial
 *   counts the samples staged since the start of training;  t = time row (0 for per-sample draws);
 *   need 0, 1: per-sample gates and draws; 2: a time row's keep/drop uniform (word 0); 3: a time row's four N(0,1);
 *   4: mg_weighted_order (t = i, serial = epoch).
 *   A sample's draws depend on (seed, serial, t) only: not on n_rows, r, the rest of the batch, or eager / replayed launch.
 *   mg_rng_fill's counter word 1 is below 0x40000000 and mg_gen_inputs' is 0x47454E00 | {0, 1}: the streams are disjoint under
 *   one seed. */
enum { MG_AUG_ED = 0, MG_AUG_AE = 1 };
enum { MG_STAGE_BATCH = 0, MG_STAGE_LAST = 1 };
typedef struct mg_augment {
    int program;                                     /* MG_AUG_ED / MG_AUG_AE */
    float noise_std, dropout_prob, pitch_shift_prob; /* ED */
    float tempo_jitter, note_dropout, velocity_jitter, timing_jitter; /* AE */
    int pitch_shift;                                 /* AE, semitones >= 0 */
    uint64_t seed;
} mg_augment;
int mg_stage_augment(const float* notes, const int64_t* labels, long src_rows, int T, int note_dim, float* notes_out,
                     int64_t* labels_out, int n_rows, const int64_t* order, long order_len, const uint64_t* counter,
                     const uint64_t* base, const uint64_t* serial_base, int rule, const mg_augment* aug, mg_stream_t stream);
/* torch.utils.data.WeightedRandomSampler(weights, num_samples = m, replacement = True) (ed_dataset.py:505-549) on the device:
 * order[i], i < m, = the first row whose inclusive fp64 prefix sum cdf[row] exceeds u * cdf[n - 1] (binary search, clamped to
 * n - 1), u a 53-bit uniform from the Philox block keyed by (seed, epoch, i) -- the `order` mg_stage_augment reads. */
int mg_weighted_order(const double* cdf, long n, int64_t* order, long m, uint64_t seed, uint64_t epoch, mg_stream_t stream);
/* The running sums of an epoch's metrics (src/emotion_discriminator/train_ed.py:75-82) after one batch, capturable:
 *   acc[0] += loss[0] * rows ;  acc[1] += #{r : argmax(logits[r, :]) == labels[r]}      (fp32, rounded like the torch ops
 *   they replace; first-index argmax, NaN counts as the maximum, as torch.argmax). */
int mg_ed_metrics_acc(const float* logits, const int64_t* labels, const float* loss, int rows, int n_classes, float* acc,
                      mg_stream_t stream);

/* ---- per-step random inputs (replaces torch.randn / torch.rand / nn.Dropout's bernoulli draws:
 *      src/gan/train_gan.py:188,218; src/gan/utils.py:76; src/gan/feature_encoder.py:34) in ONE launch:
 *      normal[n_normal] ~ N(0,1), uniform[n_uniform] ~ U(0,1), mask{0,1} = keep-mask * 1/(1-p_drop).
 *      A uniform is (k + 0.5) 2^-24 for the top 24 bits k of its Philox word, clamped to 1 - 2^-24: range [2^-25, 1 - 2^-24],
 *      never 0 and never 1.  A mask element is kept when its uniform >= p_drop.
 *      Philox4x32-10 keyed by `seed`; *step_counter (device, uint64) is read and then advanced on device,
 *      so a captured hipGraph draws fresh numbers at every replay.  Any tensor pointer may be NULL.
 *      Counter = (q, (q >> 32) ^ (jid << 28), step lo, step hi): q the block of elements 4q .. 4q + 3 (one word each for a
 *      uniform or a mask, Box-Muller on the word pairs (0, 1) and (2, 3) for the normals), jid the tensor's place among the
 *      non-NULL ones in the order normal, uniform, mask0, mask1.  tests/draw_ref.py restates every layout on the host.
 *      Riders (each NULL: absent):
 *        adam_state:  *step_counter is NOT advanced here; instead the Adam state of the optimiser whose update will consume the
 *                     draws is advanced (it is not read by this launch).  Pair it with mg_adam_flat(state_ticked = 1), which
 *                     applies the update without advancing its state and advances *rng_step instead: two launches per sub-step
 *                     instead of four.  Without adam_state a second launch of this call advances *step_counter.
 *        adam_state2: one draw serving TWO updates (critic and generator step fused into one graph): both states are advanced.
 *                     Needs adam_state, and must differ from it.
 *        jobs:        mg_stage_rows_cursor (counter = step_counter; n_jobs, n_rows, order, order_len, base and the per-job rules
 *                     as there) in the SAME launch: the staging rides as extra block planes.  Both only read the step counter
 *                     and a fused step needs both first -- one launch and one dependent-launch gap fewer.  Needs both states
 *                     and at least one tensor to draw. */
int mg_rng_fill(float* normal, long n_normal, float* uniform, long n_uniform, float* mask0, long n_mask0,
                float* mask1, long n_mask1, float p_drop, uint64_t seed, uint64_t* step_counter,
                double* adam_state, double* adam_state2, float beta1, float beta2, const mg_stage_job* jobs,
                int n_jobs, int n_rows, const int64_t* order, long order_len, const uint64_t* base,
                mg_stream_t stream);

/* ---- sampling from a trained generator (melo_gan_amd.gan.generate; the reference's generation route, app.py:53-65,97-110) ----
 * mg_gen_inputs: the generator's three inputs for `rows` samples in ONE launch (replaces app.py's torch.randn noise, its
 *   base-vector + 0.15 * torch.randn_like jitter and torch.zeros latent): for row r with key (emotion[r], sample[r])
 *     noise[r, 0:noise_dim]   ~ N(0,1)
 *     numeric[r, 0:num_dim]   = table[emotion[r], :] + jitter * N(0,1)     (table: n_emotions x num_dim, device)
 *     latent[r, 0:latent_dim] = 0                                         (latent may be NULL when latent_dim is 0)
 *   Philox4x32-10 keyed by `seed`, counter = (element block, input, emotion, sample): a sample's inputs do not depend on the
 *   other rows, their number or their order.  A row whose emotion lies outside [0, n_emotions) is padding: zeros. */
int mg_gen_inputs(const int32_t* emotion, const int32_t* sample, int rows, float* noise, int noise_dim, float* numeric,
                  int num_dim, const float* table, int n_emotions, float jitter, float* latent, int latent_dim, uint64_t seed,
                  mg_stream_t stream);
/* mg_emotion_score: the frozen classifier's verdict on `rows` generated samples (torch.softmax(logits, 1) indexed by the
 * target and torch.argmax(logits, 1) of the G-step's emotion loss inputs, src/gan/train_gan.py:230-240):
 *   p_target[r] = softmax(logits[r, :])[target[r]]  (fp32, row maximum subtracted first)   pred[r] = first argmax
 *   acc[3c + {0, 1, 2}] += {rows with target c, of them with pred == c, sum of their p_target}   (fp64, n_classes <= 32)
 * Rows whose target lies outside [0, n_classes) are padding: p_target 0, not counted.  One block: reruns add identical sums. */
int mg_emotion_score(const float* logits, int rows, int n_classes, const int32_t* target, float* p_target, int32_t* pred,
                     double* acc, mg_stream_t stream);

/* ---- blends and transitions between emotions (melo_gan_amd.gan.morph; csrc/small_kernels.hip, csrc/morph_metrics.hip) ----
 * mg_gen_inputs_mix: mg_gen_inputs' three outputs for rows that mix.  Row r carries weights[r, 0:n_emotions] (fp32), two keys
 *   key_a[r] = (emotion, sample) and key_b[r] = (emotion, sample) (int32 pairs) and t[r] (fp32 in [0, 1]):
 *     base[c]  = sum_e weights[r, e] * table[e, c]    fp32, class order, every product and sum rounded on its own: a
 *                                                     one-hot row gives table[e] exactly
 *     draw(k)  = what mg_gen_inputs draws for the key k = (emotion, sample): the same Philox counter words, key and
 *                Box-Muller; (za, va) = the noise and the jitter normals of key_a, (zb, vb) those of key_b
 *     t == 0 or key_a == key_b:  noise = za, numeric = base + jitter * va   (key_b is not drawn)
 *     t == 1:                    noise = zb, numeric = base + jitter * vb
 *     otherwise, spherically:    theta = acos(clamp(za.zb / (|za| |zb|), -1, 1)),  ca = sin((1 - t) theta) / sin(theta),
 *                                cb = sin(t theta) / sin(theta)   (sin(theta) < 2^-20 or not a number: ca = 1 - t, cb = t),
 *                                all in fp64 from fp64 sums of the widened draws (per-lane partials in element order, a fixed
 *                                butterfly over the 64 lanes), ca and cb rounded to fp32;
 *                                noise = ca * za + cb * zb,  numeric = base + jitter * (ca * va + cb * vb), the mixes with
 *                                every product and sum rounded on its own.  The jitter takes the noise's coefficients.
 *   `base + jitter * v` is ONE fused multiply-add, as mg_gen_inputs evaluates it: an exact row with one-hot weights equals
 *   mg_gen_inputs' row for that key bit for bit.  latent = 0.  A row whose key_a emotion lies outside [0, n_emotions) is
 *   padding: zeros (its weights are not read).  One 64-lane block per row, no atomics; a row depends on its own descriptors
 *   and the seed alone.  n_emotions 1..32. */
int mg_gen_inputs_mix(const float* weights, const int32_t* key_a, const int32_t* key_b, const float* t, int rows, float* noise,
                      int noise_dim, float* numeric, int num_dim, const float* table, int n_emotions, float jitter, float* latent,
                      int latent_dim, uint64_t seed, mg_stream_t stream);
/* Reductions over paths: x and logits hold P paths of S1 consecutive rows each (path-major).
 * mg_path_d2: out[p, s] (fp64, (P, S1)) = sum_j (x[p, s + 1, j] - x[p, s, j])^2 for s < S1 - 1, and out[p, S1 - 1] the same sum
 *   between step S1 - 1 and step 0 (the endpoint distance; 0 when S1 = 1).  x (P * S1, D) fp32; every element is widened to
 *   fp64 before the subtraction; identical rows give exactly 0.  One 256-lane workgroup per (p, s); 16-byte loads when
 *   D % 4 == 0 and x is 16-byte aligned, element-wise otherwise; per-lane sums in element order, a fixed butterfly over the
 *   wave, a fixed tree over the four waves.  D <= 2^30.
 * mg_path_probs: probs (P * S1, K) fp64 = the softmax of the fp32 logits evaluated in fp64 with the row maximum (the lowest
 *   index on ties) taken out and its own term not computed (mg_cls_eval_acc's rule); then acc (G, S1, K + 1) fp64:
 *   acc[g, s, k] = sum of probs[p, s, k] over the paths with group[p] == g, p = 0 .. P-1 in order, one lane per word;
 *   acc[g, s, K] = the number of those paths.  group int32 (P,); a group outside [0, G) is skipped.  K 2..32.
 * Both: no atomics of any kind; eager runs, reruns and graph replays leave identical bits. */
int mg_path_d2(const float* x, int P, int S1, int D, double* out, mg_stream_t stream);
int mg_path_probs(const float* logits, const int32_t* group, int P, int S1, int n_classes, int n_groups, double* probs,
                  double* acc, mg_stream_t stream);

/* ---- edits in the VAE's latent space (melo_gan_amd.ae.edit; csrc/latent_edit.hip) ----
 * mg_latent_rows: the decoder's input z (rows, L) fp32 for `rows` edited latents.  mu, logvar (n_src, L) fp32 are the encoded
 *   source pieces, dirs (n_dir, L) fp32 direction vectors (NULL when n_dir is 0; mu and logvar may be NULL when n_src is 0).
 *   Row r carries kind[r] (int32: 0 padding, 1 prior, 2 posterior), src_a[r], src_b[r] (int32 rows of mu), t[r] (fp32), dir[r]
 *   (int32 row of dirs, < 0: none), alpha[r], sigma[r] (fp32) and key[r] = (piece, sample) (an int32 pair), all on the device:
 *     kind 0:  z = 0; nothing else of the row is used
 *     kind 1:  base = 0, s = 1 (src_a, src_b and t are not used)
 *     kind 2:  base = mu[a]                          when t == 0 or a == b  (mu[b] is not read)
 *              base = mu[b]                          when t == 1
 *              base = (1 - t) mu[a] + t mu[b]        otherwise, interp 0
 *              base = ca mu[a] + cb mu[b]            otherwise, interp 1: theta = acos(clamp(mu[a].mu[b] / (|mu[a]| |mu[b]|),
 *                                                    -1, 1)), ca = sin((1 - t) theta) / sin(theta), cb = sin(t theta) /
 *                                                    sin(theta) (sin(theta) < 2^-20 or not a number: ca = 1 - t, cb = t), from
 *                                                    fp64 sums of the widened elements: lane u of 64 adds the element blocks
 *                                                    q = u, u + 64, .. (elements 4q .. 4q + 3) in element order, then a fixed
 *                                                    butterfly over the lanes; ca and cb stay fp64
 *              s = exp(0.5 logvar[a])
 *     z = base + alpha * dirs[dir] + (sigma * s) * n,  added in this order
 *   n ~ N(0,1): Philox4x32-10 keyed by `seed`, counter = (element block, a tag of this kernel's own, piece, sample), Box-Muller
 *   as mg_gen_inputs applies it: a row's normals depend on its key and the seed alone, not on its position, the other rows or
 *   their number.  Everything is evaluated in fp64 from the widened fp32 inputs, every product and sum rounded on its own, with
 *   ONE rounding to fp32 at the store.  A term whose coefficient is exactly 0 is not evaluated (alpha == 0 or dir < 0: dirs is
 *   not read; sigma == 0: nothing is drawn and logvar is not read), so a posterior row with t in {0, 1}, alpha = 0 and
 *   sigma = 0 is mu[a] or mu[b] bit for bit, and a prior row with sigma = 1 and no direction is n itself.
 * mg_latent_cycle: what decode -> re-encode keeps of each edit.  z, mu2 (rows, L) fp32: the edited latents and the posterior
 *   means of their re-encoded decodings; kind, src_a, dir as above.  out (rows, 6) fp64, with m = mu[src_a] (0 for a prior row)
 *   and d = dirs[dir]:
 *     out[r] = { |z - m|^2, |mu2 - z|^2, |mu2 - m|^2, (mu2 - m).d, (z - m).d, d.d }      the last three 0 when dir < 0
 *   and six zeros for a padding row.  Every element is widened to fp64 before the subtraction (identical inputs give exactly
 *   0); lane u of 64 adds the elements u, u + 64, .. in that order, then a fixed butterfly over the wave.
 * Both: one 64-lane workgroup per row; no atomics; capturable; eager runs, reruns and graph replays leave identical bits.
 *   L 1..1024; rows >= 0 (0: nothing is launched); n_src, n_dir >= 0.  The descriptors lie on the device, so the entry points
 *   cannot see them: a row of kind 1 or 2 whose src_a / src_b (kind 2) lies outside [0, n_src), whose dir >= n_dir, or whose
 *   kind is none of 0, 1, 2 reads neither mu, logvar nor dirs and is written as NaN. */
int mg_latent_rows(const float* mu, const float* logvar, int n_src, const float* dirs, int n_dir, const int32_t* kind,
                   const int32_t* src_a, const int32_t* src_b, const float* t, const int32_t* dir, const float* alpha,
                   const float* sigma, const int32_t* key, int rows, int L, int interp, uint64_t seed, float* z, mg_stream_t stream);
int mg_latent_cycle(const float* z, const float* mu2, const float* mu, int n_src, const float* dirs, int n_dir, const int32_t* kind,
                    const int32_t* src_a, const int32_t* dir, int rows, int L, double* out, mg_stream_t stream);

/* ---- MIDI events into note rolls; the classifier's verdicts per window and per file (melo_gan_amd.midi_import,
 *      melo_gan_amd.emotion_discriminator.predict; csrc/roll_encode.hip, csrc/note_decode.h) ----
 * An event is four int32 (pitch, velocity, dur_q, step_q), durations and steps in 1/64 beat; a velocity below 0 marks a rest.
 * note_encode (csrc/note_decode.h, beside the decode it inverts) takes an event to one position of a roll, fp32, every
 * operation rounded on its own:
 *     p = clamp(pitch, 36, 96)       x0 = (p + 0.5) / 63.5 - 1
 *     v = clamp(velocity, 60, 127)   x1 = ((v + 0.5 - 60) / 67) * 1.2 + (-0.2f), and 1.0 for v = 127
 *     d = clamp(dur_q, 16, 256)      x2 = d / 128 - 1
 *     s = clamp(step_q, 0, 256)      x3 = s / 128 - 1                           a rest: (-1, -1, -1, x3)
 *   The generator's output contract (mg_note_stats' decode, midi.notes_from_roll) takes (x0 .. x3) back to (p, v, d / 64 beats,
 *   s / 64 beats, or 0.1 beat for s < 7): on pitches 36..96, velocities 60..127, durations 16..256 and steps 7..256 the encode
 *   is the decode's exact inverse.
 * mg_roll_encode: one batch x (rows, T, 4) of windows of `events` (n_events, 4).  Batch row r is window
 *     w = (counter[0] - base[0]) * rows + r            (mg_scatter_rows_cursor's rule; the launch does not advance the cursor)
 *   of the W windows win_start (int64), win_len (int32): position i < win_len[w] = note_encode(events[win_start[w] + i]);
 *   positions i >= win_len[w], and every position of a row with w >= W, hold the padding row (-1, -1, -1, -1).
 *   loss[w, 0:8] (int64, written for w < dst_rows; zeros for w >= W) counts over the window's events: pitch raised, pitch
 *   lowered, velocity raised, duration lengthened, duration shortened, steps in 1..6, steps of 0 (both decode as 0.1 beat),
 *   rests.  The descriptors lie on the device, so the entry point cannot see them: a window with win_start < 0, win_len outside
 *   [0, T] or win_start + win_len > n_events reads nothing of `events`; its row is NaN and its counts are -1.
 *   One 64-lane workgroup per row, one 16-byte load and one 16-byte store per position, the counts summed per lane and by a
 *   fixed butterfly.  events and x 16-byte aligned; rows 1..65535; T 1..2^20.
 * mg_window_votes: logits (W, K) fp32 of W windows that belong to F files, file f owning the windows file_off[f] ..
 *   file_off[f + 1] - 1 (int64, F + 1 entries):
 *     probs (W, K) fp64       mg_path_probs' softmax (one device function under both)
 *     win_pred (W) int32      the first index of the largest logit, NaN counting as the largest (mg_emotion_score's rule)
 *     file_mean (F, K) fp64   the sum of the file's probs in window order over their number, one lane per word
 *     file_pred (F) int32     the first index of the largest mean, by the same rule
 *     switches (F) int32      the file's windows whose win_pred differs from the window's before it
 *   A file without windows gets zeros, -1 and 0; a file whose offsets leave [0, W] or run backwards reads nothing: NaN, -1, -1.
 *   K 2..32; W >= 0; F >= 1.
 * Both: no atomics; capturable; eager runs, reruns and graph replays leave identical bits. */
int mg_roll_encode(const int32_t* events, long n_events, const int64_t* win_start, const int32_t* win_len, long W, int T, int rows,
                   float* x, int64_t* loss, long dst_rows, const uint64_t* counter, const uint64_t* base, mg_stream_t stream);
int mg_window_votes(const float* logits, const int64_t* file_off, int F, int n_classes, long W, double* probs, int32_t* win_pred,
                    double* file_mean, int32_t* file_pred, int32_t* switches, mg_stream_t stream);

/* ---- integrated gradients of the frozen emotion classifier, per note (melo_gan_amd.emotion_discriminator.explain;
 *      csrc/explain.hip) ----
 * X (W, T, 4) fp32 holds W resident windows, win_len (W) int32 their lengths; the baseline b is the silent roll, every value
 * -1 (mg_roll_encode's padding row).  A batch of B rows holds G = B / R windows of R consecutive rows each; batch row r
 * belongs to window
 *     w = (counter[0] - base[0]) * G + r / R           (mg_scatter_rows_cursor's rule with G for the batch; no launch
 *                                                       advances the cursor)
 * and has no window when r >= G * R or w >= W.
 * mg_ig_rows: out (B, T, 4) fp32.  A row without a window is b.
 *     MG_IG_PATH    (R = S steps):  b + alpha (x_w - b) with alpha = ((r % R) + 0.5) / R, evaluated in fp64 from the widened
 *                   fp32 input, every operation rounded on its own, ONE rounding to fp32 at the store: a value equal to b
 *                   stays b bit for bit.  win_len, rank and n_del are not read (may be NULL; D is ignored).
 *     MG_IG_DELETE  (R = 2 D, n_del (D) int32, rank (W, T) int32 as mg_ig_rank leaves it):  x_w, with the positions
 *                   t < win_len[w] whose rank is >= 0 and  < n_del[j]               for row j = r % R < D      (the strongest
 *                   supporters), or                       >= win_len[w] - n_del[j - D]  for row j >= D         (the strongest
 *                   opponents) replaced by b.
 * mg_ig_seed: logits (B, K) fp32 of the batch, target (W) int32 -> dlogits (B, K) fp32, dlogits[r, j] = (j == target[w]) -
 *   p[j] with p the fp64 softmax mg_window_votes reports (one device function under both), rounded once; logp (B) fp64 =
 *   (z[k] - max) - log(1 + the other classes' terms in class order).  A row without a window gets zeros; a target outside
 *   [0, K) gives NaN.  K 2..32.
 * mg_ig_accumulate: dnotes (B, T, 4) fp32, the classifier's input gradients of a MG_IG_PATH batch -> for each of the batch's
 *   windows w < W, all fp64:
 *     attr[w, t, c] = (x - b) * (sum over the window's R rows, in row order, of dnotes / R);  exactly 0 where x = b
 *     note[w, t]    = ((attr[w,t,0] + attr[w,t,1]) + attr[w,t,2]) + attr[w,t,3]
 *     sums[w, 0:5]  = the sum over t of note, then of attr[.., c] for c = 0..3: thread u of 256 adds its positions u,
 *                     u + 256, .. in order, then a fixed butterfly over each wave, then the four waves in order
 *   Windows >= W are not written.  One workgroup per window; one 16-byte load per gradient position.
 * mg_ig_rank: rank (W, T) int32 of note (W, T) fp64 within each window: for t < win_len[w] the number of u < win_len[w]
 *   with note[u] > note[t], or note[u] == note[t] and u < t (descending, ties to the lower position: a permutation of
 *   0 .. win_len - 1); -1 for t >= win_len[w].  Counted over tiles of mg_ig_rank_tile() values held in LDS.  A window with a
 *   NaN among its real events, or a length outside [0, T], gets -1 everywhere.
 * All: T 1..4096; B 1..65535 (mg_ig_seed: 2^24); X, out and dnotes 16-byte, attr 32-byte aligned; no atomics; capturable;
 *   eager runs, reruns and graph replays leave identical bits. */
enum { MG_IG_PATH = 0, MG_IG_DELETE = 1 };
int mg_ig_rows(const float* X, const int32_t* win_len, const int32_t* rank, const int32_t* n_del, int D, long W, int T, int B, int R,
               int mode, float* out, const uint64_t* counter, const uint64_t* base, mg_stream_t stream);
int mg_ig_seed(const float* logits, const int32_t* target, long W, int B, int n_classes, int R, float* dlogits, double* logp,
               const uint64_t* counter, const uint64_t* base, mg_stream_t stream);
int mg_ig_accumulate(const float* dnotes, const float* X, long W, int T, int B, int R, double* attr, double* note, double* sums,
                     const uint64_t* counter, const uint64_t* base, mg_stream_t stream);
int mg_ig_rank(const double* note, const int32_t* win_len, long W, int T, int32_t* rank, mg_stream_t stream);
int mg_ig_rank_tile(void);

/* ---- shared motifs between note rolls, transposition-invariant (melo_gan_amd.motifs; csrc/motif.hip) ----
 * Tokens.  A row (T, 4) fp32 is decoded position by position by the generator's output contract (csrc/note_decode.h, the
 * decode of mg_note_stats).  A position with a non-finite value is skipped and takes no time; every other one, note or rest,
 * takes ticks = (int)floor(step_beats * 64.0 + 0.5), in fp64.  With the row's sounding notes n_0 .. n_{M-1} in order, the row
 * has max(M - 1, 0) tokens; token k - 1 (1 <= k < M) is
 *     interval = pitch_k - pitch_{k-1}                                  -60..60
 *     ioi      = the ticks of the positions from n_{k-1}'s up to the one in front of n_k's (rests between them count)
 *     rhythm   = (ioi >= 12) + (ioi >= 24) + (ioi >= 48) + (ioi >= 96) + (ioi >= 192), and 0 in mode MG_MOTIF_INTERVAL
 *     token    = (interval + 64) | (rhythm << 7)
 * mg_motif_tokens: rolls (N, T, 4) -> tokens (N, T) uint16, 0xFFFF from the row's length on, and lengths (N) int32.  One
 *   workgroup per row, chunks of 256 positions.  Every element of both outputs is written.
 * Matching.  For token rows a (Mq tokens) and b (Mc tokens), run(i, j) = run(i - 1, j - 1) + 1 where a[i] == b[j], else 0;
 * nothing carries across the start of either row.  L = the largest run, (i_end, j_end) the cell that attains it with the
 * smallest i, then the smallest j.
 * mg_motif_lcs: q_tokens (Nq, T), q_len (Nq), c_tokens (Nc, T), c_len (Nc) ->
 *     packed (Nq, Nc) int64   (L << 32) | ((0xFFFF - i_end) << 16) | (0xFFFF - j_end), and 0 for L = 0: larger is better
 *     reach (Nq, T) int32     reach[q, i] = the largest run(i, .) over the corpus rows that are not skipped; 0 from q_len[q] on
 *   q_groups (Nq) / c_groups (Nc) int32, both or neither: a pair with equal group ids is skipped, packed 0, nothing in reach.
 *   Lengths outside [0, T] are clamped into it; tokens from a row's length on are not read.  reach is cleared by the entry
 *   point, collected by integer atomic maxima over workgroups of mg_motif_corpus_tile() corpus rows and finished in place by
 *   a second launch; every element of both outputs is written.  Nq 1..65535.
 * mg_motif_rank: packed (Nq, Nc), non-negative -> vals (Nq, k) int64 and idx (Nq, k) int32: the k largest values of each row in
 *   descending order with their columns, equal values by ascending column; value 0 and column -1 from Nc on.  k 1..1024.
 * All: T 1..4096; the token buffers 2-byte, int32 buffers 4-byte, int64 buffers 8-byte, rolls 16-byte aligned; integer
 *   arithmetic throughout, so eager runs, reruns and graph replays leave identical bits; capturable. */
enum { MG_MOTIF_INTERVAL_RHYTHM = 0, MG_MOTIF_INTERVAL = 1 };
int mg_motif_tokens(const float* rolls, long N, int T, int mode, uint16_t* tokens, int32_t* lengths, mg_stream_t stream);
int mg_motif_lcs(const uint16_t* q_tokens, const int32_t* q_len, int Nq, const uint16_t* c_tokens, const int32_t* c_len, long Nc,
                 int T, const int32_t* q_groups, const int32_t* c_groups, int64_t* packed, int32_t* reach, mg_stream_t stream);
int mg_motif_rank(const int64_t* packed, int Nq, long Nc, int k, int64_t* vals, int32_t* idx, mg_stream_t stream);
int mg_motif_corpus_tile(void);

/* ---- rendering note lists to audio (csrc/render.hip; melo_gan_amd.audio, melo_gan_amd.render, generate --wav) ----
 * The reference stops at the .mid file; hearing one takes a synthesiser from outside.  mg_render_notes is an additive
 * synthesiser with an integer phase accumulator: F files in ONE launch, a lane per output sample.
 *   per note (device):  onset, release  int32 sample indices, file-local, release > onset
 *                       inc             uint32, the fundamental's phase increment per sample in units of 2^-32 turns
 *                       gain            fp32
 *   per file (device):  note_ptr[F+1]   int64 CSR offsets into the note arrays; WITHIN A FILE THE NOTES ARE SORTED BY ONSET
 *                                       (ascending; the kernel bounds its candidate search by it and does not check)
 *                       pcm_ptr[F+1]    int64 offsets of the file's samples in pcm; every element of [pcm_ptr[f], pcm_ptr[f+1])
 *                                       is written, 0 where nothing sounds and for a file without notes
 *                       n_begin[F]      int32 file-local index of the first sample rendered: 0 = the file from its start,
 *                                       otherwise a window  pcm[pcm_ptr[f] + j] = y[n_begin[f] + j]
 *                       max_len[F]      int32 >= release - onset + release_len of every note of the file
 *   host:               max_samples     >= pcm_ptr[f+1] - pcm_ptr[f] of every file (sizes the grid), 1 .. 2^31 - 1
 *                       voice           the instrument, read before the call returns (see mg_voice)
 *                       peak            NULL, or F floats: mg_pcm_peak of what this launch wrote, in the same launch
 * For the file-local sample n a note is live while onset <= n < release + release_len; with k = n - onset, kr = max(n - release, 0)
 *   y[n] = sum over live notes i in array order, over partials h ascending, skipped when (uint64)mult[h] * inc[i] >= 2^31 (Nyquist)
 *            gain[i] * min((k + 1) / attack, 1) * exp(-kr / (fs * release_tau)) * weight[h] * exp(-decay[h] * k / fs) * sin(2 pi x)
 *   x    = ((((uint32)(mult[h] * inc[i])) * (uint32)k mod 2^32) >> 8) * 2^-24          (exact in fp32)
 * The terms are evaluated in fp32 (one expf for both envelopes, sinpif on the exact x) and added in fp32 in exactly that order by
 * the lane that owns n, every operation rounded on its own.  A sample is therefore a function of its file's notes and of n alone:
 * windows, batches, batch positions, eager launches and graph replays agree bit for bit.  Against the fp64 evaluation each
 * sample lies within (32 + 2 A + M) 2^-24 S (S = sum of |amplitude| of its M terms, A = its largest envelope exponent):
 * tests/render_ref.py, tests/test_render_gpu.py.
 * mg_pcm_peak: peak[f] = max |pcm| over the file, taken as the integer maximum of the absolute values' bit patterns: exact, and
 *   independent of the order (0 for an empty file; a NaN sample yields a NaN peak).
 * mg_pcm_quantise: q = (int16) clamp(rint(pcm * s_f), -32767, 32767), s_f = (target * 32767.0f) / peak[f] in fp32, IEEE divide,
 *   s_f = 0 where peak[f] == 0; q is laid out as pcm.
 * All three are capturable (the peak is zeroed by a memset node in front of the kernel), use no floating-point atomics and return
 * -1 before any launch for: a null pointer (peak of mg_render_notes excepted); F outside 1..65535; max_samples < 1; n_partials
 * outside 1..16; attack < 1; release_len < 0; fs, release_tau or a used decay[h] not finite or not positive (decay may be 0); a used
 * weight[h] not finite; target outside (0, 1]. */
#define MG_VOICE_MAX_PARTIALS 16
typedef struct mg_voice {
    int n_partials;                           /* 1..16; entries past it are ignored */
    uint32_t mult[MG_VOICE_MAX_PARTIALS];     /* partial h sounds at mult[h] times the fundamental */
    float weight[MG_VOICE_MAX_PARTIALS];
    float decay[MG_VOICE_MAX_PARTIALS];       /* 1/s, from the onset on */
    int attack;                               /* samples of the linear ramp, >= 1 */
    float release_tau;                        /* s, time constant after the release */
    int release_len;                          /* samples a note sounds after its release, >= 0 */
    float fs;                                 /* sample rate, Hz */
} mg_voice;
int mg_render_notes(const int32_t* onset, const int32_t* release, const uint32_t* inc, const float* gain, const int64_t* note_ptr,
                    const int64_t* pcm_ptr, const int32_t* n_begin, const int32_t* max_len, int F, long max_samples,
                    const mg_voice* voice, float* pcm, float* peak /* may be NULL */, mg_stream_t stream);
int mg_pcm_peak(const float* pcm, const int64_t* pcm_ptr, int F, long max_samples, float* peak, mg_stream_t stream);
int mg_pcm_quantise(const float* pcm, const int64_t* pcm_ptr, const float* peak, int F, long max_samples, float target, int16_t* q,
                    mg_stream_t stream);

/* ---- held-out evaluation of a trained GAN (melo_gan_amd.gan.evaluate) ----
 * The reference judges a generator with host scripts over files: src/gan/analyze_midi.py:28-45 (mean / min / max of pitch,
 * mean velocity of written .mid files, per emotion), src/gan/diagnose.py:53-80 (per-column range, mean and standard deviation
 * of a split) and the classifier's loss and accuracy of src/emotion_discriminator/train_ed.py:31-32 (argmax == label).
 * mg_eval_acc adds ONE evaluated batch to a device-resident accumulator that lives for a whole pass over a split: no host
 * round trip per batch.  Capturable.  Rows whose emot_idx lies outside [0, n_classes) are padding and count nowhere.
 *   real, fake      (B, T, C) fp32, 16-byte aligned, C a multiple of 4 in 4..1024
 *   emot_idx        (B) int64, the true class
 *   d_real, d_fake  (B) critic scores, or both NULL (their sums stay untouched)
 *   logits_fake, logits_real   (B, n_classes) classifier logits of the generated / the real rolls, or NULL (that side untouched)
 * Accumulator: mg_eval_acc_words(K = n_classes, C) 8-byte words, in this order:
 *   int64   n[K]                        rows of true class k
 *   int64   conf_fake[K][K], conf_real[K][K]       [true class][predicted class]; prediction = first index of the maximum,
 *                                       NaN counts as the maximum (mg_ed_metrics_acc's and mg_emotion_score's rule)
 *   double  d_sum[2]                    sum d_real, sum d_fake
 *   double  cls[2][2][K]                [fake, real][cross-entropy, softmax probability of the true class][true class]: sums of
 *                                       lse(z) - z[y] with mg_softmax_ce's row-maximum-subtracted log-sum-exp, and of
 *                                       exp(z[y] - max) / sum exp(z - max), both evaluated in fp64 from the fp32 logits
 *   double  nsum[2][K][C], nsq[2][K][C] [real, fake][true class][channel]: sum of x and of x * x over rows and time, every
 *                                       element widened to fp64 before it is added
 *   float   nmin[2][K][C], nmax[2][K][C]   fminf / fmaxf over the same elements (NaN elements are skipped); +inf / -inf when empty
 * mg_eval_acc_reset writes the empty accumulator (zeros, +inf, -inf).
 * Launch shape: a workgroup of 256 lanes takes one row and one chunk of its time axis, 16 bytes per lane with the channel
 * innermost (C = 4: one time position per lane; C = 128: 32 lanes per position), about 512 workgroups per call; it reduces
 * its lanes by a fixed tree and writes its partials to its own entry of `work` (mg_eval_acc_workspace_bytes; every entry
 * is written before the fold reads it).  A second launch of the same call folds the entries in a fixed order into the
 * accumulator.  No floating-point atomics: two runs, and an eager run and a graph replay, leave identical bits.  The integer
 * counts use integer atomics.  tick != NULL: tick[0] += 1 (the batch counter that mg_stage_rows_cursor and mg_eval_noise of
 * the NEXT batch read, so a pass replays one graph and nothing else). */
long mg_eval_acc_words(int n_classes, int C);
size_t mg_eval_acc_workspace_bytes(int B, int T, int C);
int mg_eval_acc_reset(void* acc, int n_classes, int C, mg_stream_t stream);
int mg_eval_acc(const float* real, const float* fake, int B, int T, int C, const int64_t* emot_idx, const float* d_real,
                const float* d_fake, const float* logits_fake, const float* logits_real, int n_classes, void* acc, void* work,
                size_t work_bytes, uint64_t* tick, mg_stream_t stream);
/* The noise of an evaluation batch: row r belongs to split row i = (counter[0] - base[0]) * rows + r and gets
 *   noise[r, 0:noise_dim] ~ N(0,1)   Philox4x32-10 keyed by `seed`, counter = (element block, 0x4556414C, i lo, i hi)
 * (Box-Muller, as mg_gen_inputs), zeros when i >= n (the padded tail of the last batch).  A split row's noise depends on
 * (seed, i) alone -- not on the batch size or on what else is evaluated -- so two checkpoints evaluated under one seed are a
 * paired comparison.  Counter word 1 keeps the stream apart from mg_rng_fill's, mg_stage_augment's and mg_gen_inputs'. */
int mg_eval_noise(float* noise, int rows, int noise_dim, const uint64_t* counter, const uint64_t* base, long n, uint64_t seed,
                  mg_stream_t stream);

/* ---- pairwise metrics between two feature sets (melo_gan_amd.gan.evaluate --feature-metrics; csrc/pair_metrics.hip) ----
 * The reference suspects mode collapse and memorisation (src/gan/diagnose.py: "latent vectors are very collapsed";
 * src/gan/tsne.py plots clusters) and measures neither.  KID, k-NN precision / recall and the nearest-training-neighbour check
 * all reduce to the dot products between two sets, reduced in the GEMM's epilogue: the nA x nB matrix is never stored.
 *   A (nA, D), B (nB, D)   contiguous fp32, row-major, 16-byte aligned; D a multiple of 4 in 4..1024; 1 <= nA, nB <= 2^20
 *   g_ij  = a_i . b_j      exact fp32 on v_mfma_f32_32x32x2_f32, accumulated in fp32
 *   d2_ij = max(|a_i|^2 + |b_j|^2 - 2 g_ij, 0)      the row norms are computed once per call into the workspace, by the same
 *                          multiply-add chain as g: the d2 between a row and an identical row is exactly 0
 * mg_pair_ksum:   out[0] (fp64) = sum_ij (g_ij / D + 1)^3, every g widened to fp64 before the cube and the sum (the cubic
 *                 kernel of the Kernel Inception Distance).  exclude_diag (needs A == B, nA == nB) leaves i == j out.
 * mg_pair_knn:    out (nA, k) fp32 = the k smallest d2_ij over j, ascending, 1 <= k <= 8.  exclude_self (needs A == B,
 *                 nA == nB) skips j == i.  k > nB - exclude_self is an argument error.  Ties and duplicate rows are legal: the
 *                 output is a multiset of values.
 * mg_pair_margin: out[i] (fp32) = min_j (d2_ij - r2B[j]); row i lies in B's k-NN manifold (r2B[j] = b_j's k-th neighbour
 *                 distance within B) iff out[i] <= 0.
 * Launch shape: a workgroup of 256 lanes owns 64 rows of A and a run of 64-row tiles of B; D streams through LDS in chunks of
 * 32 with rows past the end zero-filled; columns j >= nB and the excluded column enter the epilogue as +inf.  Per-workgroup
 * partials (an fp64 sum; per row a sorted candidate list, +inf where a run holds fewer than k columns) go to `work`
 * (mg_pair_workspace_bytes(nA, nB, D, k); k = 1 for mg_pair_ksum and mg_pair_margin), and a second launch of the same call
 * folds them in a fixed order.  No floating-point atomics: two runs, and an eager run and a graph replay, leave identical bits.
 * Capturable. */
size_t mg_pair_workspace_bytes(long nA, long nB, int D, int k);
int mg_pair_ksum(const float* A, long nA, const float* B, long nB, int D, int exclude_diag, double* out, void* work,
                 size_t work_bytes, mg_stream_t stream);
int mg_pair_knn(const float* A, long nA, const float* B, long nB, int D, int exclude_self, int k, float* out, void* work,
                size_t work_bytes, mg_stream_t stream);
int mg_pair_margin(const float* A, long nA, const float* B, long nB, int D, const float* r2B, float* out, void* work,
                   size_t work_bytes, mg_stream_t stream);
/* ---- Frechet distance and covariance spectra of feature sets (melo_gan_amd.gan.evaluate --feature-metrics --frechet;
 *      csrc/frechet.hip) ----
 * The one metric of the feature_space block that is no function of pairwise dot products: it needs second moments and a
 * symmetric eigensolver, both in fp64.  For row sets X, Y with means mx, my and unbiased covariances Sx, Sy
 *   FD = |mx - my|^2 + tr Sx + tr Sy - 2 tr (Sx Sy)^(1/2),   tr (Sx Sy)^(1/2) = sum_i sqrt(max(lambda_i(B), 0)),
 *   B = H^T Sy H,   H = V diag(sqrt(max(w, 0))),   Sx = V diag(w) V^T
 * B is symmetric positive semi-definite by construction and stays well defined for rank-deficient covariances (fewer rows
 * than D); no square root of a non-symmetric product is formed.
 * mg_feat_moments:  X (n, D) contiguous fp32, 16-byte aligned, D a multiple of 4 in 4..256, 2 <= n <= 2^20 -> mean (D) and
 *                   cov (D, D) fp64, the full matrix, exactly symmetric.  Two passes: column sums / n, then the sum of outer
 *                   products of the centred rows (fp32 widened to fp64, minus the fp64 mean) on v_mfma_f64_16x16x4_f64,
 *                   divided by n - 1.  Rows past the end of a 16-row tile and columns past D are zero after centring.
 * mg_sym_eig:       A (batch, D, D) fp64, D in 1..256, 1 <= batch <= 4096; the symmetric part (A + A^T) / 2 is decomposed.
 *                   w (batch, D) ascending; V (batch, D, D) or null: orthonormal columns in w's order; info (batch, 2) int32 =
 *                   {sweeps run, converged 0 / 1}.  Cyclic two-sided Jacobi: one workgroup of 1024 lanes per matrix, barriers
 *                   only; a sweep is the D - 1 (D odd: D) steps of a round-robin tournament, each step D / 2 disjoint
 *                   rotations applied as one J^T A J.  A pair is left alone when |a_pq| <= 2^-53 sqrt|a_pp a_qq| or
 *                   |a_pq| <= 2^-53 |A|_F / m (m = D rounded up to even); t = tan of the angle comes from theta = (a_qq - a_pp) / (2 a_pq) as
 *                   sign / (|theta| + hypot(1, theta)), never from theta^2.  The solve ends with the first sweep that rotates
 *                   nothing (that sweep is counted) or after 30 sweeps: converged = 0 then, w = the current diagonal.  The
 *                   columns of V are normalised once, after the last sweep (their norms drift with c^2 + s^2's rounding).
 * mg_frechet_pairs: means (S, D), covs (S, D, D) fp64 of S sets (1..4096), D in 1..256; pairs (P, 2) int32 on the device,
 *                   P in 1..65535, ordered (a, b): H comes from set a.  Launches: one mg_sym_eig of the S covariances (a set is
 *                   decomposed once however many pairs name it); the batched fp64 product kernel twice (T = S_b H_a, then
 *                   B = H_a^T T); one eigenvalue-only solve of the P matrices B; one finishing launch.
 *                   out (P, 4) = {fd, |ma - mb|^2, tr Sa + tr Sb, sum_i sqrt(max(lambda_i, 0))}: fd and the last entry are NaN
 *                   when set a's or the pair's solve did not converge; all four when a pair names a set outside 0 .. S - 1.
 *                   spectrum (S, 3) = {participation ratio (sum w)^2 / sum w^2, effective rank exp(-sum p ln p), top-1 share
 *                   max w / sum w} of each covariance's eigenvalues clamped at 0; NaN when they sum to 0 or the solve did not
 *                   converge.  info (S + P, 2): mg_sym_eig's, sets first.
 * Partials (column sums and 16 x 16 tiles per run of rows) and the solver's working copies live in `work`, 16-byte aligned:
 * mg_frechet_workspace_bytes(n, D, S, P) serves mg_feat_moments on n rows (n = 0: not asked), mg_sym_eig on a batch of S
 * (P = 0) and mg_frechet_pairs on S sets and P pairs; 0 for sizes outside the limits.  Folds run in a fixed order and there
 * are no floating-point atomics: two runs, and an eager run and a graph replay, leave identical bits.  Capturable; bad
 * arguments return -1 before any launch. */
size_t mg_frechet_workspace_bytes(long n, int D, int S, int P);
int mg_feat_moments(const float* X, long n, int D, double* mean, double* cov, void* work, size_t work_bytes, mg_stream_t stream);
int mg_sym_eig(const double* A, int batch, int D, double* w, double* V, int32_t* info, void* work, size_t work_bytes,
               mg_stream_t stream);
int mg_frechet_pairs(const double* means, const double* covs, int S, int D, const int32_t* pairs, int P, double* out,
                     double* spectrum, int32_t* info, void* work, size_t work_bytes, mg_stream_t stream);
/* The inverse of mg_stage_rows_cursor for one fp32 array: row r of src (rows, width) goes to row
 *   p = (counter[0] - base[0]) * rows + r   of dst (dst_rows, width); rows with p >= dst_rows are dropped (the padded tail of
 * a pass's last batch).  Capturable: a replayed evaluation batch leaves its features at their split position. */
int mg_scatter_rows_cursor(const float* src, int rows, int width, float* dst, long dst_rows, const uint64_t* counter,
                           const uint64_t* base, mg_stream_t stream);

/* ---- note-level musical statistics of real and generated rolls (melo_gan_amd.gan.evaluate --music-metrics;
 *      csrc/note_metrics.hip) ----
 * The reference's instrument for "is the GAN learning different emotions" is src/gan/analyze_midi.py:28-54: note count, mean
 * pitch, pitch range, unique pitches, mean velocity and density of .mid files written one by one.  mg_note_stats computes the
 * same quantities, and the histograms the music-generation literature compares (pitch, pitch class, pitch-class transitions,
 * interval, duration, inter-onset step), from the rolls of ONE evaluated batch where they lie on the device.  Capturable.
 * The launch sits in front of mg_eval_acc, which advances the cursor.
 *   real, fake      (B, T, 4) fp32, 16-byte aligned; C != 4 is an argument error: only the note-row format decodes into notes
 *   emot_idx        (B) int64, the true class; rows with a label outside [0, n_classes) are padding, count nowhere and write
 *                   nothing
 *   B in 1..32767, T in 1..2^20, n_classes in 1..32; anything else returns -1 before a launch
 * The decode of a time position x = (x0, x1, x2, x3) is the output contract src/gan/utils.py:102-156 (notes_from_roll with the
 * chromatic scale, for which snapping is the identity), every fp32 operation rounded on its own, no fused multiply-add, an
 * IEEE divide:
 *   invalid = any of the four not finite       counted as such and otherwise absent (the host function would raise)
 *   rest    = x1 < -0.2f
 *   pitch   = clip(trunc((x0 + 1f) * 63.5f), 36, 96)
 *   vel     = clip(trunc(60f + ((x1 - -0.2f) / 1.2f) * 67f), 0, 127)
 *   dur     = d > 0.25f ? double(d) : 0.25,   d = ((x2 + 1f) / 2f) * 4f       beats
 *   step    = s > 0.1f ? double(s) : 0.1,     s = ((x3 + 1f) / 2f) * 4f       beats (0.1 enters as the Python double)
 * Accumulator: mg_note_acc_words(K = n_classes) = 2 K 504 int64 words, one block per [side: real, fake][true class]:
 *   counters[8]        rows, valid events, notes, rests, invalid events, overlaps, transitions, 0
 *   pitch[128]         notes by MIDI pitch
 *   velocity[128]      notes by MIDI velocity
 *   dur16[16]          notes by min(15, floor(dur * 4))
 *   step16[16]         valid events, rests included, by min(15, floor(step * 4))
 *   interval[64]       per transition, min(63, |pitch - previous pitch|)
 *   pctm[12][12]       per transition, [previous pitch % 12][pitch % 12]
 * A transition is a pair of consecutive sounding notes of one row (rests and invalid positions between them are skipped); an
 * overlap is a note at position t < T - 1 with dur > step (it still sounds when the next position begins).
 * mg_note_acc_reset writes zeros.
 * Per-row outputs at the split position p = (counter[0] - base[0]) * B + row (mg_scatter_rows_cursor's rule; rows with
 * p >= dst_rows are dropped; the caller zeroes both arrays):
 *   row_i      [side][dst_rows][8] int32: notes, rests, invalid, unique pitches, lowest pitch, highest pitch (0 and 0 without
 *              a note), overlaps, transitions
 *   row_beats  [side][dst_rows][2] double: sum of step over valid events, sum of dur over notes; every term is fp64 before it is
 *              added, a lane adds its positions in order and the 256 lanes are reduced by a fixed tree
 * Launch shape: one workgroup of 256 lanes per (side, row), 2 B workgroups; a lane loads one time position as one 16-byte
 * load and the workgroup walks the row in chunks of 256 positions.  The previous sounding pitch comes from the wave's ballot
 * of sounding lanes, across waves and chunks through LDS.  Histograms are integer LDS atomics, the unique pitches a 61-bit
 * mask OR-ed over the workgroup; at the end only the non-zero bins go to the accumulator, as integer atomics.  No
 * floating-point atomics: two runs, and an eager run and a graph replay, leave identical bits. */
long mg_note_acc_words(int n_classes);
int mg_note_acc_reset(void* acc, int n_classes, mg_stream_t stream);
int mg_note_stats(const float* real, const float* fake, int B, int T, int C, const int64_t* emot_idx, int n_classes, void* acc,
                  int32_t* row_i, double* row_beats, long dst_rows, const uint64_t* counter, const uint64_t* base,
                  mg_stream_t stream);

/* ---- held-out evaluation of a trained VAE (melo_gan_amd.ae.evaluate; csrc/vae_metrics.hip) ----
 * The reference asks twice whether the VAE's latents are any good -- src/gan/diagnose.py:82-91 warns of posterior collapse
 * when latents.std() < 0.1, src/gan/tsne.py asks whether they cluster by emotion -- and measures neither; of the
 * reconstruction it keeps one MSE over four channels of different scales.  mg_vae_eval_acc adds ONE evaluated batch to a
 * device-resident accumulator that lives for a whole pass.  Capturable; no host round trip.
 *   x, recon        (B, T, 4) fp32, 16-byte aligned; C != 4 is an argument error
 *   mu, logvar      (B, L) fp32, 1 <= L <= 1024
 *   labels          (B) int64, the true class; a label outside [0, n_classes) is padding: the row counts nowhere and writes
 *                   nothing
 *   B in 1..32767, T in 1..2^20, n_classes in 1..32; anything else, a null pointer or a workspace smaller than
 *   mg_vae_eval_acc_workspace_bytes(B, L) returns -1 before a launch
 * A time position is decoded on both sides by mg_note_stats' decode (one function, csrc/note_decode.h); it is valid when all
 * four values are finite on both sides, and an invalid position is counted as such and otherwise absent.
 * Accumulator: mg_vae_eval_acc_words(K = n_classes, L) = K (26 + 5 L) 8-byte words, one block per true class:
 *   int64  c[16]       rows; valid positions; invalid positions; both sounding; both rest; missed (real sounding,
 *                      reconstruction rest); extra (real rest, reconstruction sounding); over both-sounding positions: pitch
 *                      equal, |pitch difference| <= 1, pitch class equal, sum |pitch difference|, sum |velocity difference|;
 *                      four zero words
 *   double se[4], ae[4]   per channel, sum (recon - x)^2 and sum |recon - x| over valid positions, each element widened to
 *                      fp64 before the subtraction
 *   double dur_abs, step_abs   sum |dur difference| in beats over both-sounding positions, sum |step difference| over valid ones
 *   double lat[5][L]   per latent dimension, summed over rows, in fp64 from the fp32 inputs: mu, mu^2, logvar, exp(logvar),
 *                      -1/2 (1 + logvar - mu^2 - exp(logvar))
 * mg_vae_eval_acc_reset writes zeros.
 * Per-row outputs at the split position p = (counter[0] - base[0]) * B + row (mg_scatter_rows_cursor's rule; rows with
 * p >= dst_rows are dropped; the caller zeroes both arrays):
 *   row_d  [dst_rows][4] double: squared error summed over the four channels, KL summed over the dimensions, sum |dur
 *          difference|, sum |step difference|
 *   row_i  [dst_rows][8] int32: c[1 .. 8] of the row
 * Launch shape: launch 1 has one workgroup of 256 lanes per row; a lane loads one time position of x and one of recon as a
 * 16-byte load each, the workgroup walks the row in chunks of 256 positions, a lane adds its own positions in order (and the
 * KL terms of dimensions u, u + 256, ...), the 256 lanes are reduced by a fixed tree, and the row's partial goes to the row's
 * own entry of `work` and to row_d / row_i.  In launch 2 of the same call one lane owns one accumulator word of one class and
 * adds the batch's rows of that class onto it one at a time, rows 0 .. B-1 in order: acc = ((acc + r0) + r1) + ...; the latent
 * words are computed there straight from mu / logvar.  No atomics of any kind: two runs, and an eager run and a graph
 * replay, leave identical bits, and for fixed input arrays the accumulator does not depend on how the rows are cut into
 * batches.  tick != NULL: tick[0] += 1 at the end of launch 2 (mg_eval_acc's batch counter). */
long mg_vae_eval_acc_words(int n_classes, int L);
size_t mg_vae_eval_acc_workspace_bytes(int B, int L);
int mg_vae_eval_acc_reset(void* acc, int n_classes, int L, mg_stream_t stream);
int mg_vae_eval_acc(const float* x, const float* recon, int B, int T, int C, const float* mu, const float* logvar, int L,
                    const int64_t* labels, int n_classes, void* acc, int32_t* row_i, double* row_d, long dst_rows,
                    const uint64_t* counter, const uint64_t* base, void* work, size_t work_bytes, uint64_t* tick,
                    mg_stream_t stream);

/* ---- held-out evaluation of a trained emotion classifier (melo_gan_amd.emotion_discriminator.evaluate; csrc/cls_metrics.hip) ----
 * The classifier is the frozen judge of every number gan.evaluate reports, and the reference's own evaluation of it
 * (src/emotion_discriminator/evaluate_ed.py) is a copy of the model file.  mg_cls_eval_acc adds ONE evaluated batch to a
 * device-resident accumulator that lives for a whole pass.  Capturable; no host round trip.
 *   logits          (B, K = n_classes) fp32;  clean_logits: NULL, or (B, K) fp32 of the same rows without augmentation
 *   labels          (B) int64, the true class; a label outside [0, K) is a padding or unlabelled row: it counts nowhere and
 *                   writes nothing
 *   inv_temps       HOST pointer to n_temps = G fp64 inverse temperatures, copied into the launch's arguments (host and
 *                   device then use the same values); inv_temperature scales the logits before everything else (1.0: plain)
 *   B in 1..32767, K in 2..16, n_bins in 1..32, G in 1..64, every inverse temperature positive and finite; anything else, a
 *   null pointer or a workspace smaller than mg_cls_eval_acc_workspace_bytes(B, G) returns -1 before a launch
 * Per row, in fp64, without contraction, in this order:
 *   z_k = (double)logit_k * inv_temperature;  pred = argmax z (lowest index on ties);  m = z_pred
 *   rest = sum over k != pred, in class order, of exp(z_k - m);  s = 1 + rest;  p_pred = 1 / s, p_k = exp(z_k - m) / s
 *   ce = -log p_y computed as log1p(rest) + (m - z_y): finite for any finite logits
 *   brier = sum_k (p_k - [k = y])^2 in class order;  conf = p_pred;  margin = conf - max_{k != pred} p_k
 *   bin = min(n_bins - 1, floor(conf * n_bins));  correct = pred == y
 *   nll_g = the same ce with z_k * inv_temps[g] for z_k (m = z_pred * inv_temps[g])
 *   flipped = clean_logits given and its argmax (same scaling and tie rule) differs from pred
 * Accumulator: mg_cls_eval_acc_words(K, n_bins, G) = K (7 + K + 3 n_bins + G) 8-byte words, one block per TRUE class, zeroed
 * by the caller:
 *   int64  rows, correct, flipped, confusion[K] (by predicted class), bin_count[n_bins], bin_correct[n_bins]
 *   double ce, brier, conf, margin, bin_conf[n_bins] (sum of conf of the bin's rows), nll_T[G]
 * Per-row outputs at the split position p = (counter[0] - base[0]) * B + row (mg_scatter_rows_cursor's rule; rows with
 * p >= dst_rows are dropped; the caller zeroes the arrays):
 *   probs  [dst_rows][K] double;  row_i [dst_rows][4] int32: pred, bin, correct, flipped
 *   row_d  [dst_rows][4] double: ce, conf, p_y, margin
 * Launch shape: launch 1 has one wave per row; lane g computes nll_g, lane 0 the rest, and the row's partial goes to the row's
 * own entry of `work`.  In launch 2 one lane owns one accumulator word of one class and adds the batch's rows of that class
 * onto it one at a time, rows 0 .. B-1 in order.  No atomics: two runs, and an eager run and a graph replay, leave identical
 * bits, and the accumulator does not depend on how the rows are cut into batches.  tick != NULL: tick[0] += 1 at the end of
 * launch 2.
 * mg_cls_auroc_pairs: the exact one-vs-rest Mann-Whitney counts of a finished pass from its stored probs (n, K) fp64 and
 * labels (n) int64, 1 <= n <= 131072.  out [4][K] int64 (zeroed by the call): for every class k
 *   wins[k] = #{(i, j): y_i = k, y_j valid and != k, p_ik > p_jk},  ties[k] likewise with ==,  n_pos[k] = #{y_i = k},
 *   n_neg[k] = #{y_j valid and != k}
 * A workgroup owns a tile of 256 rows i and walks tiles of 256 rows j through LDS; counts are summed inside the wave and the
 * workgroup, then one integer atomicAdd per workgroup, array and class: integer addition does not depend on the order. */
long mg_cls_eval_acc_words(int n_classes, int n_bins, int n_temps);
size_t mg_cls_eval_acc_workspace_bytes(int B, int n_temps);
int mg_cls_eval_acc(const float* logits, const float* clean_logits, int B, int n_classes, const int64_t* labels, int n_bins,
                    const double* inv_temps, int n_temps, double inv_temperature, void* acc, double* probs, int32_t* row_i,
                    double* row_d, long dst_rows, const uint64_t* counter, const uint64_t* base, void* work, size_t work_bytes,
                    uint64_t* tick, mg_stream_t stream);
int mg_cls_auroc_pairs(const double* probs, const int64_t* labels, long n, int n_classes, int64_t* out, mg_stream_t stream);

/* ---- exact t-SNE of a feature set (melo_gan_amd.gan.tsne, melo_gan_amd.gan.evaluate --tsne; csrc/tsne.hip) ----
 * The reference's tsne.py asks whether the VAE latents cluster by emotion and hands the answer to scikit-learn; here the
 * affinities and the descent run on the device.  4 <= N <= 16384 (the dense P is 1 GiB there), everything fp32 unless said.
 * mg_tsne_affinities: X (N, D) contiguous, D >= 1 -> the symmetric joint P (N, N) and, if `beta` is not null, the N precisions.
 *   d2_ij = max(|x_i|^2 + |x_j|^2 - 2 x_i . x_j, 0)   mg_pair_*'s formula on the exact-fp32 matrix pipe; the row norms are the
 *                          rows' own Gram diagonal by the same multiply-add chain, so identical rows are exactly 0 apart
 *   p_j|i ~ exp(-beta_i (d2_ij - min_{j != i} d2_ij)), j != i, with beta_i the root of  entropy(p_.|i) = log(perplexity):
 *                          bracketed by doubling from beta = 1 (at most 100 times), then bisected 64 times; no early exit.  The
 *                          sums of an entropy evaluation are fp64.  1 <= perplexity < N - 1, there is no root otherwise.
 *   P_ij = (p_j|i + p_i|j) / 2N                        P_ij and P_ji hold the same bits, the diagonal is exactly 0
 *   Four launches: norms, one 64x64 tile of d2 per workgroup (into P), one workgroup per row with the row of d2 in LDS, one
 *   workgroup per tile pair (I <= J) for the symmetric sum in place.
 * mg_tsne_step: one iteration of scikit-learn's _gradient_descent on Y (N, 2), in place, with w_ij = 1 / (1 + |y_i - y_j|^2):
 *   launch 1  a workgroup owns 16 rows and a run of 64-column tiles (runs sized for ~1024 workgroups) and writes, per row,
 *             attr = sum_j p_ij w_ij (y_i - y_j) and rep = sum_j w_ij^2 (y_i - y_j) to its slab entry, and z = sum_{j != i} w_ij
 *             of its rows to its own entry; every sum is fp64 under a fixed lane tree.  With a trace the instantiation that
 *             also sums p_ij (log p_ij - log w_ij) (fp64 logarithms) runs instead.
 *   launch 2  every workgroup folds the z entries in the same fixed order into Z, then per row
 *             grad = 4 (exaggeration attr - rep / Z);  gains += 0.2 where update grad < 0, else gains *= 0.8, floored at 0.01;
 *             update = momentum update - lr gains grad;  Y += update.      grad (N, 2), if not null, receives the gradient.
 *   trace     if not null, record r = trace_cursor ? trace_cursor[0] : 0 of `trace` (4 doubles each; dropped when
 *             r >= trace_cap) receives KL = sum p log p - sum p log w + log Z (of the plain P, whatever the exaggeration),
 *             |grad|_2, Z, and sum p (log p - log w); trace_cursor[0], if given, is then advanced by one, so that a replayed
 *             graph of iterations fills consecutive records without the host.
 * `work`: mg_tsne_workspace_bytes(N) bytes (0 for an N outside the range), 16-byte aligned, shared by both calls.  No grid-wide
 * barrier, no signalling between workgroups, no floating-point atomics: workgroups of a launch write disjoint memory, and two
 * runs, an eager run and a graph replay, and runs on different streams leave identical bits.  Capturable. */
size_t mg_tsne_workspace_bytes(long N);
int mg_tsne_affinities(const float* X, long N, int D, float perplexity, float* P, float* beta, void* work, size_t work_bytes,
                       mg_stream_t stream);
int mg_tsne_step(const float* P, long N, float* Y, float* update, float* gains, float exaggeration, float momentum, float lr,
                 float* grad, double* trace, uint64_t* trace_cursor, long trace_cap, void* work, size_t work_bytes,
                 mg_stream_t stream);

/* ---- fused flat Adam / AdamW (torch.optim.Adam defaults; src/gan/train_gan.py:136-145,
 *      src/ae/train_ae.py:79).  state: double[4] = {step, beta1^step, beta2^step, unused},
 *      advanced on device so the launch is hipGraph-replayable.  grad_scale multiplies g first
 *      (used for 1/world_size and for clip_grad_norm_ via a device scalar if gs_dev != NULL).
 *      state_ticked: the Adam state was already advanced by mg_rng_fill's adam_state rider and is only read here; rng_step,
 *      if not NULL, is then advanced here (NULL for the second of the two updates behind one two-state draw).
 *      Otherwise the state is advanced by this call (a launch of its own in front of the update).
 *      table / n_table (NULL / 0: none): the update ALSO keeps WQ-layout copies (mg_conv16) of some weight tensors current:
 *      entry = a dense tensor W(n,c,k) = w[n*w_sn + c*w_sc + k] at [start, start + N*Cc*K) of the flat buffer, in (N,Cc,K) order
 *      (w_sn = Cc*K, w_sc = K) or (Cc,N,K) order (w_sn = K, w_sc = N*K); dst (N*Cc*K floats) receives the updated values in WQ
 *      order. */
#define MG_MAX_WQ_ENTRIES 8
typedef struct mg_wq_entry {
    long start;
    int N, Cc, K, w_sn, w_sc;
    float* dst;
} mg_wq_entry;
int mg_adam_flat(float* p, const float* g, float* m, float* v, long n,
                 float lr, float beta1, float beta2, float eps, float weight_decay,
                 double* state, float grad_scale, const float* gs_dev, int state_ticked, uint64_t* rng_step,
                 const mg_wq_entry* table, int n_table, mg_stream_t stream);
/* ---- exponential moving average of a flat parameter buffer (csrc/ema.hip): the rider behind the generator's mg_adam_flat ----
 * Per element, in fp64, every operation rounded on its own (no contraction):
 *     shadow[i] = shadow[i] + (1.0 - d) * ((double)p[i] - shadow[i])
 * d is computed on the device: t = adam_state[0] - 1 - step_offset (adam_state: mg_adam_flat's `state`, already advanced by the
 * update in front of this launch and only read here; step_offset: the step count at which averaging began, so t = averaged
 * updates before this one); d = ramp ? min(decay, (1 + t) / (10 + t)) : decay, an IEEE fp64 divide.  Only `shadow` is written:
 * one launch, hipGraph-replayable with constant arguments.  -1 before any launch for n < 1, decay outside [0, 1) or a null
 * pointer; non-finite parameters propagate into the shadow.  n need not be a multiple of 4; 16-byte aligned p and shadow take
 * the vector path. */
int mg_ema_flat(const float* p, double* shadow, long n, double decay, int ramp, const double* adam_state, double step_offset,
                mg_stream_t stream);
/* out[0] = sqrt(sum g^2) ; out[1] = min(1, max_norm/(norm+1e-6))  (clip_grad_norm_, train_ae.py:121) */
int mg_grad_norm_clip(const float* g, long n, float max_norm, float* out, void* work, size_t work_bytes,
                      mg_stream_t stream);
size_t mg_grad_norm_workspace_bytes(long n);

/* ---- the latent-mode emotion classifier's training step in two launches (csrc/mlp_train.hip) ----
 * The network is MLPClassifier (src/emotion_discriminator/ed_model.py:72-95): n_hidden x [Linear, GELU (exact erf),
 * Dropout(p)] and a Linear head, on (rows, in_dim) latents; the loss is the mean cross-entropy of train_ed.py:51-82.
 * Supported: n_hidden 1..4, in_dim and every width 1..512 (no multiple of anything), n_classes 2..32, rows >= 1; anything
 * else returns -1 before a launch.  Exact fp32 on v_mfma_f32_16x16x4_f32; no atomics: reruns and replays give identical bits.
 * Layer l < n_hidden is hidden layer l, layer n_hidden is the head; w[l] is (out, in) row-major as in the state_dict. */
#define MG_MLP_MAX_HIDDEN 4
typedef struct mg_mlp_cls {
    int n_hidden, in_dim, width[MG_MLP_MAX_HIDDEN], n_classes;
    const float* w[MG_MLP_MAX_HIDDEN + 1];  /* the weights the layers compute with (w_orig / sigma under spectral norm) */
    const float* b[MG_MLP_MAX_HIDDEN + 1];
    float* z[MG_MLP_MAX_HIDDEN];            /* (rows, width[l]) pre-activation x W^T + b */
    float* a[MG_MLP_MAX_HIDDEN];            /* (rows, width[l]) GELU(z) * mask */
    float* dz[MG_MLP_MAX_HIDDEN];           /* (rows, width[l]) d loss / d z = (dz[l+1] W[l+1]) * GELU'(z) * mask */
    float* mask[MG_MLP_MAX_HIDDEN];         /* (rows, width[l]) dropout keep-mask / (1 - p) */
} mg_mlp_cls;
/* Launch A, the per-row half: a workgroup owns 16 rows and walks them through every layer with the activations in LDS,
 * then the cross-entropy, then the data gradients back to hidden layer 0.  Writes z / a / dz of every hidden layer,
 * logits (rows, n_classes), loss_rows[r] = logsumexp(logits[r]) - logits[r, y[r]] and dlogits = (softmax - onehot) / rows;
 * a label outside [0, n_classes) makes its row's term and dlogits NaN (as mg_softmax_ce) and is never used as an index.
 *   rows' source: x (rows, in_dim) / y (rows) as they are, or, with split_x != NULL, gathered from split_x (src_rows, in_dim) /
 *     split_y by mg_stage_augment's position rules (`rule`, order, order_len, counter = step_counter, base) -- the staged
 *     rows and labels are then also written to x / y.
 *   train = 0 (eval): no masks, no backward: logits and loss_rows only (z / a are written where not NULL).
 *   draw = 0: mask[l] is read.  draw = 1: mask[l] is drawn and written: Philox4x32-10 keyed by seed, counter = (e / 4,
 *     (e / 4 >> 32) ^ (stream << 28), step lo, step hi), word e % 4, e = the element's index in (rows, width[l]), stream =
 *     l for l < 2 -- element for element what mg_rng_fill(NULL, 0, NULL, 0, mask0, ., mask1, ., p_drop, seed, step_counter, ...)
 *     writes -- and l + 2 for l = 2, 3.  *step_counter is read, never written.
 *   tick_state != NULL: the Adam state {step, beta1^step, beta2^step} is advanced as by mg_rng_fill's adam_state rider (not read here). */
int mg_mlp_cls_fwd_bwd(const mg_mlp_cls* net, int rows, float* x, int64_t* y, const float* split_x, const int64_t* split_y,
                       long src_rows, const int64_t* order, long order_len, const uint64_t* base, int rule, int train, int draw,
                       float p_drop, uint64_t seed, const uint64_t* step_counter, double* tick_state, float beta1, float beta2,
                       float* logits, float* loss_rows, float* dlogits, mg_stream_t stream);
/* Launch B, the per-parameter half: the grid is tiled over every layer's (out, in) weight and its bias; a wave reduces its
 * 16 x 16 tile over the rows in row order.  g[w_off[l] + o * in + i] = sum_r dz[l][r, o] * a[l-1][r, i] (a[-1] = x, dz[n_hidden]
 * = dlogits) and g[b_off[l] + o] = sum_r dz[l][r, o], always; w_off / b_off: n_hidden + 1 element offsets into the flat
 * buffers of n_flat floats (host arrays).  apply != 0: the same threads then apply AdamW to their elements of p / m / v from
 * the gradient in registers -- mg_adam_flat(state_ticked = 1)'s formula and `state` semantics (state is read, never written; weight
 * decay decoupled).  One workgroup also writes loss[0] = (sum of loss_rows in row order) / rows, adds the batch to `metrics`
 * (if not NULL) exactly as mg_ed_metrics_acc does, and advances *rng_step (if not NULL; apply mode only). */
int mg_mlp_cls_wgrad_update(const mg_mlp_cls* net, int rows, const float* x, const float* dlogits, const long* w_off,
                            const long* b_off, long n_flat, float* g, float* p, float* m, float* v, int apply, float lr,
                            float beta1, float beta2, float eps, float weight_decay, const double* state,
                            const float* loss_rows, float* loss, const float* logits, const int64_t* y, float* metrics,
                            uint64_t* rng_step, mg_stream_t stream);

/* ---- VAE extras (src/ae/model.py:127-133, src/ae/train_ae.py:35-51) ---- */
/* z = mu + eps*exp(0.5*logvar) */
int mg_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, long n, mg_stream_t stream);
/* backward of the reparameterisation: dmu = dz + dmu_kld ; dlv = dz*eps*0.5*exp(0.5*logvar) + dlv_kld */
int mg_reparam_bwd(const float* dz, const float* logvar, const float* eps, const float* dmu_kld,
                   const float* dlv_kld, float* dmu, float* dlv, long n, mg_stream_t stream);
/* mse = mean((recon-x)^2); kld = -0.5*mean(1+lv-mu^2-exp(lv)); out = {total, mse, kld};
 * drecon = 2(recon-x)/n_x ; dmu, dlv include beta-weighted KLD grads PLUS the z-path grads are added by caller */
size_t mg_vae_loss_workspace_bytes(void);
int mg_vae_loss(const float* recon, const float* x, long n_x, const float* mu, const float* logvar, long n_z,
                float beta, float* out, float* drecon, float* dmu_kld, float* dlv_kld,
                void* work, size_t work_bytes, mg_stream_t stream);

/* ---- hipGraph capture of a launch sequence issued through this library (or anything else on the stream) ---- */
int mg_graph_begin(mg_stream_t stream);
/* Ends the capture and instantiates it n (1..8) times into execs_out[0..n) (launches may then alternate between the executables). */
int mg_graph_end(mg_stream_t stream, void** execs_out, int n);
/* kernel nodes of the graph the calling thread captured last (-1: unknown): the launches one replay stands for */
int mg_graph_last_kernel_nodes(void);
int mg_graph_launch(void* graph_exec, mg_stream_t stream);
int mg_graph_destroy(void* graph_exec);

/* ---- timing helper: HIP events on an arbitrary stream (bench.py roofline leg) ---- */
int mg_event_create(void** ev);
int mg_event_record(void* ev, mg_stream_t stream);
int mg_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int mg_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* MELO_GAN_HIP_H */
