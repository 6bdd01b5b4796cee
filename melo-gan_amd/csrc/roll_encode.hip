// MIDI events into note rolls, and the classifier's verdicts on a file's windows folded per file (melo_gan_amd/midi_import.py,
// melo_gan_amd/emotion_discriminator/predict.py).  mg_roll_encode writes one batch of windows of an event list in the
// generator's output contract, by note_decode.h's note_encode, with the count of what the encode had to clamp;
// mg_window_votes turns the windows' logits into probabilities, per-window verdicts and per-file means.  The layout is in
// include/melo_gan_hip.h; the host restatement is melo_gan_amd/midi_rolls.py.  No atomics: every output word has one writer and
// a fixed summation order.
#include "common.h"
#include "note_decode.h"
#include "softmax64.h"

#define ST ((hipStream_t)stream)

constexpr int RE_LOSS = 8;
constexpr int WV_THREADS = 256;
constexpr int WV_MAX_K = 32;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// One 64-lane workgroup per batch row: window w = (counter - base) * B + row (mg_scatter_rows_cursor's rule).  Lane u encodes
// the positions u, u + 64, ..: one 16-byte load of the event, one 16-byte store of the position.  The eight counts are summed
// per lane and then by a fixed butterfly over the wave; lane k stores count k.
__global__ __launch_bounds__(64) void roll_encode_kernel(const i32x4* __restrict__ events, long n_events,
                                                         const long* __restrict__ win_start, const int* __restrict__ win_len,
                                                         long W, int T, f32x4* __restrict__ x, long* __restrict__ loss,
                                                         long dst_rows, const unsigned long long* __restrict__ counter,
                                                         const unsigned long long* __restrict__ base) {
    const int lane = threadIdx.x;
    const unsigned long long w = (counter[0] - base[0]) * (unsigned long long)gridDim.x + blockIdx.x;
    f32x4* out = x + (long)blockIdx.x * T;
    const bool live = w < (unsigned long long)W;
    long start = 0;
    int len = 0;
    if (live) {
        start = win_start[w];
        len = win_len[w];
    }
    // a window that points outside the event list reads nothing of it (mg_latent_rows' rule): NaN, and -1 for its counts
    const bool ok = start >= 0 && len >= 0 && len <= T && start <= n_events - len;
    int cnt[RE_LOSS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lane; i < T; i += 64) {
        f32x4 v;
        if (!ok) {
            v[0] = v[1] = v[2] = v[3] = __builtin_nanf("");
        } else if (i < len) {
            const i32x4 e = events[start + i];
            unsigned fired;
            v = note_encode(e[0], e[1], e[2], e[3], fired);
#pragma unroll
            for (int k = 0; k < RE_LOSS; ++k) cnt[k] += (int)((fired >> k) & 1u);
        } else {
            v[0] = v[1] = v[2] = v[3] = -1.0f;      // the reference's padding row (src/ae/dataset.py:73-74)
        }
        out[i] = v;
    }
    if (w >= (unsigned long long)dst_rows) return;       // uniform over the workgroup
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < RE_LOSS; ++k) cnt[k] += __shfl_xor(cnt[k], m, 64);
    if (lane < RE_LOSS) {
        int mine = 0;
#pragma unroll
        for (int k = 0; k < RE_LOSS; ++k)
            if (k == lane) mine = cnt[k];
        loss[(long)w * RE_LOSS + lane] = ok ? (long)mine : -1L;
    }
}

// One lane per window: its probabilities (softmax64.h) and its verdict, the first index of the maximum with NaN counting as
// the maximum (mg_emotion_score's rule).
__global__ __launch_bounds__(WV_THREADS) void window_probs_kernel(const float* __restrict__ logits, long W, int K,
                                                                  double* __restrict__ probs, int* __restrict__ win_pred) {
    const long w = (long)blockIdx.x * WV_THREADS + threadIdx.x;
    if (w >= W) return;
    const float* z = logits + w * K;
    softmax64_row(z, K, probs + w * K);
    float mx = z[0];
    int am = 0;
    for (int j = 1; j < K; ++j) {
        const float v = z[j];
        if (v > mx || (isnan(v) && !isnan(mx))) { mx = v; am = j; }
    }
    win_pred[w] = am;
}

// One 64-lane workgroup per file over its windows lo .. hi - 1: lane k < K owns file_mean[f, k], the sum of probs[w, k] in
// window order over their number; lane 0 then takes the first argmax of the K means (NaN counting as the maximum); the lanes
// count the changes of verdict between neighbouring windows, summed by a fixed butterfly.  Offsets outside [0, W], or out of
// order, read nothing: NaN means, -1 and -1.
__global__ __launch_bounds__(64) void window_fold_kernel(const double* __restrict__ probs, const int* __restrict__ win_pred,
                                                         const long* __restrict__ file_off, long W, int K,
                                                         double* __restrict__ file_mean, int* __restrict__ file_pred,
                                                         int* __restrict__ switches) {
#pragma clang fp contract(off)
    const long f = blockIdx.x;
    const int lane = threadIdx.x;
    const long lo = file_off[f], hi = file_off[f + 1];
    double* fm = file_mean + f * K;
    if (lo < 0 || hi < lo || hi > W) {
        if (lane < K) fm[lane] = __builtin_nan("");
        if (lane == 0) { file_pred[f] = -1; switches[f] = -1; }
        return;
    }
    if (hi == lo) {
        if (lane < K) fm[lane] = 0.0;
        if (lane == 0) { file_pred[f] = -1; switches[f] = 0; }
        return;
    }
    double mean = 0.0;
    if (lane < K) {
        double s = 0.0;
        for (long w = lo; w < hi; ++w) s = s + probs[w * K + lane];
        mean = s / (double)(hi - lo);
        fm[lane] = mean;
    }
    int sw = 0;
    for (long w = lo + 1 + lane; w < hi; w += 64) sw += win_pred[w] != win_pred[w - 1];
    for (int m = 1; m < 64; m <<= 1) sw += __shfl_xor(sw, m, 64);
    double mx = mean;       // lane 0's
    int am = 0;
    for (int j = 1; j < K; ++j) {
        const double v = __shfl(mean, j, 64);
        if (lane == 0 && (v > mx || (isnan(v) && !isnan(mx)))) { mx = v; am = j; }
    }
    if (lane == 0) { file_pred[f] = am; switches[f] = sw; }
}

extern "C" {

int mg_roll_encode(const int32_t* events, long n_events, const int64_t* win_start, const int32_t* win_len, long W, int T, int rows,
                   float* x, int64_t* loss, long dst_rows, const uint64_t* counter, const uint64_t* base, mg_stream_t stream) {
    MG_CHECK_ARG(win_start && win_len && x && loss && counter && base,
                 "mg_roll_encode: null win_start / win_len / x / loss / counter / base");
    MG_CHECK_ARG(n_events >= 0 && (events || n_events == 0), "mg_roll_encode: null events with n_events = %ld", n_events);
    MG_CHECK_ARG(W >= 1 && dst_rows >= 1, "mg_roll_encode: W = %ld, dst_rows = %ld: both must be positive", W, dst_rows);
    MG_CHECK_ARG(T >= 1 && T <= (1 << 20), "mg_roll_encode: T = %d: 1..2^20", T);
    MG_CHECK_ARG(rows >= 1 && rows <= 65535, "mg_roll_encode: rows = %d: 1..65535", rows);
    MG_CHECK_ARG((((uintptr_t)events | (uintptr_t)x) & 15) == 0, "mg_roll_encode: events and x must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)win_start | (uintptr_t)loss | (uintptr_t)counter | (uintptr_t)base) & 7) == 0 &&
                     ((uintptr_t)win_len & 3) == 0,
                 "mg_roll_encode: win_start, loss, counter and base must be 8-byte, win_len 4-byte aligned");
    hipLaunchKernelGGL(roll_encode_kernel, dim3((unsigned)rows), dim3(64), 0, ST, (const i32x4*)events, n_events,
                       (const long*)win_start, (const int*)win_len, W, T, (f32x4*)x, (long*)loss, dst_rows,
                       (const unsigned long long*)counter, (const unsigned long long*)base);
    MG_CHECK_LAUNCH("roll_encode");
    return MG_OK;
}

int mg_window_votes(const float* logits, const int64_t* file_off, int F, int n_classes, long W, double* probs, int32_t* win_pred,
                    double* file_mean, int32_t* file_pred, int32_t* switches, mg_stream_t stream) {
    MG_CHECK_ARG(file_off && file_mean && file_pred && switches, "mg_window_votes: null file_off / file_mean / file_pred / switches");
    MG_CHECK_ARG(F >= 1 && F <= 0x7FFFFFFF && W >= 0 && W <= 0x7FFFFFFFL, "mg_window_votes: F = %d, W = %ld: F >= 1, W in 0..2^31 - 1",
                 F, W);
    MG_CHECK_ARG(n_classes >= 2 && n_classes <= WV_MAX_K, "mg_window_votes: %d classes: 2..32", n_classes);
    MG_CHECK_ARG(W == 0 || (logits && probs && win_pred), "mg_window_votes: null logits / probs / win_pred with W = %ld", W);
    MG_CHECK_ARG((((uintptr_t)logits | (uintptr_t)win_pred | (uintptr_t)file_pred | (uintptr_t)switches) & 3) == 0 &&
                     (((uintptr_t)probs | (uintptr_t)file_mean | (uintptr_t)file_off) & 7) == 0,
                 "mg_window_votes: logits, win_pred, file_pred and switches must be 4-byte, probs, file_mean and file_off 8-byte aligned");
    if (W > 0) {
        hipLaunchKernelGGL(window_probs_kernel, dim3((unsigned)mg_cdiv(W, WV_THREADS)), dim3(WV_THREADS), 0, ST, logits, W, n_classes,
                           probs, (int*)win_pred);
        MG_CHECK_LAUNCH("window_probs");
    }
    hipLaunchKernelGGL(window_fold_kernel, dim3((unsigned)F), dim3(64), 0, ST, (const double*)probs, (const int*)win_pred,
                       (const long*)file_off, W, n_classes, file_mean, (int*)file_pred, (int*)switches);
    MG_CHECK_LAUNCH("window_fold");
    return MG_OK;
}

}  // extern "C"
