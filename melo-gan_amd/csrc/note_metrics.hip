// Note-level musical statistics of an evaluated batch (melo_gan_amd/gan/evaluate.py --music-metrics): every real and every
// generated (T, 4) row decoded into note events by the generator's output contract (melo_gan_amd/midi.py, notes_from_roll)
// and added to device-resident integer histograms per side and true emotion.  The layout, the decode and the reference lines
// these answer to are in include/melo_gan_hip.h (mg_note_stats); the host restatement is melo_gan_amd/gan/music_metrics.py.
#include "common.h"
#include "note_decode.h"

#define ST ((hipStream_t)stream)

constexpr int NS_THREADS = 256;
constexpr int NS_WAVES = NS_THREADS / 64;
// one accumulator block per [side][true class], int64 words (include/melo_gan_hip.h)
constexpr int NS_COUNTERS = 0;      // rows, valid events, notes, rests, invalid events, overlaps, transitions, 0
constexpr int NS_PITCH = 8;
constexpr int NS_VELOCITY = NS_PITCH + 128;
constexpr int NS_DUR16 = NS_VELOCITY + 128;
constexpr int NS_STEP16 = NS_DUR16 + 16;
constexpr int NS_INTERVAL = NS_STEP16 + 16;
constexpr int NS_PCTM = NS_INTERVAL + 64;
constexpr int NS_WORDS = NS_PCTM + 144;

__device__ __forceinline__ int note_bin16(double beats) {     // min(15, floor(beats * 4)), beats > 0
    const double q = beats * 4.0;
    return q >= 15.0 ? 15 : (int)q;
}

// One workgroup per (side, row).  Lane u takes time positions u, u + 256, ...; the only order-dependent quantity is the
// previous sounding pitch of a note: inside a wave it comes from the ballot of sounding lanes, across waves from the
// per-wave last pitches in LDS (double-buffered: one barrier per chunk), across chunks from `carry`, which every lane
// derives from the same LDS words.
__global__ __launch_bounds__(NS_THREADS) void note_stats_kernel(
    const float* __restrict__ real, const float* __restrict__ fake, const int64_t* __restrict__ labels, int B, int T, int K,
    long long* __restrict__ acc, int* __restrict__ row_i, double* __restrict__ row_beats, long dst_rows,
    const unsigned long long* __restrict__ counter, const unsigned long long* __restrict__ base) {
    __shared__ unsigned s_bins[NS_WORDS];
    __shared__ int s_wlast[2][NS_WAVES];
    __shared__ unsigned long long s_mask;
    __shared__ double s_red[2][NS_THREADS];
    const int side = (int)blockIdx.x / B, row = (int)blockIdx.x % B;
    const int64_t y = labels[row];
    if (y < 0 || y >= K) return;                // a padding row: counts nowhere, writes nothing (uniform over the workgroup)
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    for (int i = u; i < NS_WORDS; i += NS_THREADS) s_bins[i] = 0u;
    if (u == 0) s_mask = 0ull;
    __syncthreads();
    const f32x4* src = reinterpret_cast<const f32x4*>((side ? fake : real) + (long)row * T * 4);
    int carry = -1;                             // last sounding pitch of the chunks behind this one
    unsigned n_notes = 0, n_rests = 0, n_invalid = 0, n_overlaps = 0, n_trans = 0;      // of this lane's wave
    unsigned long long pmask = 0ull;            // bit (pitch - 36)
    double sum_step = 0.0, sum_dur = 0.0;
    int buf = 0;
    for (int t0 = 0; t0 < T; t0 += NS_THREADS, buf ^= 1) {
        const int t = t0 + u;
        const bool in = t < T;
        NoteEvent e = {false, false, 0, 0, 0.0, 0.0};
        if (in) e = note_decode(src[t]);
        const unsigned long long m = __ballot(e.sounding);
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        const int prev_in = __shfl(e.pitch, below ? 63 - __clzll((long long)below) : 0);
        const int wave_last = __shfl(e.pitch, m ? 63 - __clzll((long long)m) : 0);
        if (lane == 0) s_wlast[buf][w] = m ? wave_last : -1;
        __syncthreads();
        int chunk_last = -1, before = carry;
#pragma unroll
        for (int j = 0; j < NS_WAVES; ++j) {
            const int v = s_wlast[buf][j];
            if (v >= 0) {
                chunk_last = v;
                if (j < w) before = v;
            }
        }
        const int prev = below ? prev_in : before;
        if (chunk_last >= 0) carry = chunk_last;
        if (e.valid) {
            atomicAdd(&s_bins[NS_STEP16 + note_bin16(e.step)], 1u);
            sum_step += e.step;
        }
        bool overlap = false, trans = false;
        if (e.sounding) {
            atomicAdd(&s_bins[NS_PITCH + e.pitch], 1u);
            atomicAdd(&s_bins[NS_VELOCITY + e.vel], 1u);
            atomicAdd(&s_bins[NS_DUR16 + note_bin16(e.dur)], 1u);
            sum_dur += e.dur;
            pmask |= 1ull << (e.pitch - NS_PITCH_LO);
            overlap = t < T - 1 && e.dur > e.step;
            if (prev >= 0) {
                trans = true;
                const int d = abs(e.pitch - prev);
                atomicAdd(&s_bins[NS_INTERVAL + (d < 63 ? d : 63)], 1u);
                atomicAdd(&s_bins[NS_PCTM + (prev % 12) * 12 + e.pitch % 12], 1u);
            }
        }
        n_notes += (unsigned)__popcll(m);
        n_rests += (unsigned)__popcll(__ballot(e.valid && !e.sounding));
        n_invalid += (unsigned)__popcll(__ballot(in && !e.valid));
        n_overlaps += (unsigned)__popcll(__ballot(overlap));
        n_trans += (unsigned)__popcll(__ballot(trans));
    }
    if (lane == 0) {
        atomicAdd(&s_bins[NS_COUNTERS + 1], n_notes + n_rests);
        atomicAdd(&s_bins[NS_COUNTERS + 2], n_notes);
        atomicAdd(&s_bins[NS_COUNTERS + 3], n_rests);
        atomicAdd(&s_bins[NS_COUNTERS + 4], n_invalid);
        atomicAdd(&s_bins[NS_COUNTERS + 5], n_overlaps);
        atomicAdd(&s_bins[NS_COUNTERS + 6], n_trans);
    }
    if (u == 0) s_bins[NS_COUNTERS] = 1u;
    if (pmask) atomicOr(&s_mask, pmask);
    s_red[0][u] = sum_step;
    s_red[1][u] = sum_dur;
    __syncthreads();
    for (int s = NS_THREADS / 2; s > 0; s >>= 1) {      // the fixed tree of the two fp64 sums
        if (u < s) {
            s_red[0][u] += s_red[0][u + s];
            s_red[1][u] += s_red[1][u + s];
        }
        __syncthreads();
    }
    long long* blk = acc + ((long)side * K + (long)y) * NS_WORDS;
    for (int i = u; i < NS_WORDS; i += NS_THREADS) {
        const unsigned v = s_bins[i];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&blk[i]), (unsigned long long)v);
    }
    if (u == 0) {
        const unsigned long long p = (counter[0] - base[0]) * (unsigned long long)B + (unsigned long long)row;
        if (p < (unsigned long long)dst_rows) {         // the padded tail of the last batch falls off the end
            const unsigned long long pm = s_mask;
            int* ri = row_i + ((long)side * dst_rows + (long)p) * 8;
            ri[0] = (int)s_bins[NS_COUNTERS + 2];
            ri[1] = (int)s_bins[NS_COUNTERS + 3];
            ri[2] = (int)s_bins[NS_COUNTERS + 4];
            ri[3] = __popcll(pm);
            ri[4] = pm ? NS_PITCH_LO + (__ffsll((long long)pm) - 1) : 0;
            ri[5] = pm ? NS_PITCH_LO + 63 - __clzll((long long)pm) : 0;
            ri[6] = (int)s_bins[NS_COUNTERS + 5];
            ri[7] = (int)s_bins[NS_COUNTERS + 6];
            double* rb = row_beats + ((long)side * dst_rows + (long)p) * 2;
            rb[0] = s_red[0][0];
            rb[1] = s_red[1][0];
        }
    }
}

__global__ void note_reset_kernel(long long* acc, long words) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) acc[i] = 0;
}

extern "C" {

long mg_note_acc_words(int n_classes) {
    if (n_classes < 1 || n_classes > 32) return 0;
    return 2L * n_classes * NS_WORDS;
}

int mg_note_acc_reset(void* acc, int n_classes, mg_stream_t stream) {
    MG_CHECK_ARG(acc && ((uintptr_t)acc & 7) == 0, "mg_note_acc_reset: acc must be an 8-byte aligned device pointer");
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32, "mg_note_acc_reset: 1..32 classes");
    const long words = 2L * n_classes * NS_WORDS;
    hipLaunchKernelGGL(note_reset_kernel, dim3((unsigned)mg_cdiv(words, 256)), dim3(256), 0, ST, (long long*)acc, words);
    MG_CHECK_LAUNCH("note_reset");
    return MG_OK;
}

int mg_note_stats(const float* real, const float* fake, int B, int T, int C, const int64_t* emot_idx, int n_classes, void* acc,
                  int32_t* row_i, double* row_beats, long dst_rows, const uint64_t* counter, const uint64_t* base,
                  mg_stream_t stream) {
    MG_CHECK_ARG(real && fake && emot_idx && acc && row_i && row_beats && counter && base,
                 "mg_note_stats: null real / fake / emot_idx / acc / row_i / row_beats / counter / base");
    MG_CHECK_ARG(C == 4, "mg_note_stats: C = %d: only the (T, 4) note-row format decodes into notes", C);
    MG_CHECK_ARG(B >= 1 && B <= 32767 && T >= 1 && T <= (1 << 20), "mg_note_stats: B must be in 1..32767 and T in 1..2^20");
    MG_CHECK_ARG(n_classes >= 1 && n_classes <= 32, "mg_note_stats: 1..32 classes");
    MG_CHECK_ARG(dst_rows >= 1, "mg_note_stats: dst_rows must be positive");
    MG_CHECK_ARG((((uintptr_t)real | (uintptr_t)fake) & 15) == 0, "mg_note_stats: real and fake must be 16-byte aligned");
    MG_CHECK_ARG((((uintptr_t)acc | (uintptr_t)row_beats) & 7) == 0 && ((uintptr_t)row_i & 3) == 0,
                 "mg_note_stats: acc and row_beats must be 8-byte aligned, row_i 4-byte aligned");
    hipLaunchKernelGGL(note_stats_kernel, dim3(2u * (unsigned)B), dim3(NS_THREADS), 0, ST, real, fake, emot_idx, B, T, n_classes,
                       (long long*)acc, (int*)row_i, row_beats, dst_rows, (const unsigned long long*)counter,
                       (const unsigned long long*)base);
    MG_CHECK_LAUNCH("note_stats");
    return MG_OK;
}

}  // extern "C"
