// Additive synthesis of note lists to PCM (melo_gan_amd/audio.py: Renderer): what turns a generated roll or a .mid file into
// something one can listen to without leaving the project.  Every note is a sum of partials under an attack ramp, a per-partial
// exponential decay and an exponential release.  The phase of a partial is an integer: (mult * inc) * k mod 2^32, in units of
// 2^-32 turns, k = samples since the onset -- no accumulated rounding, so a sample is a function of its file's notes and its
// own index and of nothing else: not of the tile it falls in, the window that is rendered, or the files beside it.  The sum over
// (note, partial) is taken in fp32 in array order by the one lane that owns the sample; there is no floating-point atomic and no
// cross-lane sum.  tests/render_ref.py restates the formula in fp64; include/melo_gan_hip.h states the contract.
//
// Pure VALU: a term costs one sinpif, one expf (both envelopes share it) and a handful of multiplies; the per-note and
// per-partial constants are wave-uniform (scalar loads, the voice in the kernel arguments), lanes run across samples.
#include "common.h"
#include <math.h>

#define ST ((hipStream_t)stream)

namespace {

constexpr int RN_THREADS = 256;            // samples per tile: one per lane
constexpr int PQ_PER_THREAD = 8;           // peak / quantise: elements per lane and tile
constexpr int PQ_TILE = RN_THREADS * PQ_PER_THREAD;

// mg_voice with the divisions done once, in double, on the host
struct RenderVoice {
    int n_partials, attack, release_len;
    float inv_attack;                      // 1 / attack
    float rel_rate;                        // 1 / (fs * release_tau)
    unsigned mult[MG_VOICE_MAX_PARTIALS];
    float weight[MG_VOICE_MAX_PARTIALS];
    float rate[MG_VOICE_MAX_PARTIALS];     // decay[h] / fs
};

// max over the block of non-negative fp32 bit patterns, added to *dst by at most one integer atomic per wave: exact and
// order-free.  *dst only grows, so whatever a plain read of it returns is a lower bound of its value: a wave whose maximum does
// not exceed that has nothing to add and skips the atomic.  Without the read every wave of a file hits one address: 290 k
// serialised atomics for a seven-minute file at 44.1 kHz made the launch 2040 us; with it 245, against 207 without a peak
// (profiles/render_bench.txt).
__device__ __forceinline__ void block_max_bits(unsigned bits, unsigned* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, bits);
}

// first index in [lo, hi) whose onset is >= v (onsets ascending); every lane walks the same path
__device__ __forceinline__ long lower_bound_onset(const int32_t* __restrict__ onset, long lo, long hi, long v) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if ((long)onset[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid = (tiles of the longest file, F).  Tile j0 of file f covers the file-local samples n_begin[f] + j0 .. + 255.
__global__ __launch_bounds__(RN_THREADS) void render_notes_kernel(
        const int32_t* __restrict__ onset, const int32_t* __restrict__ release, const uint32_t* __restrict__ inc,
        const float* __restrict__ gain, const int64_t* __restrict__ note_ptr, const int64_t* __restrict__ pcm_ptr,
        const int32_t* __restrict__ n_begin, const int32_t* __restrict__ max_len, RenderVoice V, float* __restrict__ pcm,
        unsigned* __restrict__ peak) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const long p0 = pcm_ptr[f], len = pcm_ptr[f + 1] - p0;
    const long j0 = (long)blockIdx.x * RN_THREADS;
    if (j0 >= len) return;
    const long t0 = (long)n_begin[f] + j0;                                   // first sample of the tile, file-local
    const long t1 = t0 + (len - j0 < RN_THREADS ? len - j0 : RN_THREADS);    // one past its last
    const long n = t0 + threadIdx.x;
    const bool mine = n < t1;
    const long a0 = note_ptr[f], a1 = note_ptr[f + 1];
    // a note sounds for at most max_len samples from its onset: candidates have t0 - max_len < onset < t1
    const long lo = lower_bound_onset(onset, a0, a1, t0 - (long)max_len[f] + 1);
    const long hi = lower_bound_onset(onset, lo, a1, t1);
    float acc = 0.f;
    for (long i = lo; i < hi; ++i) {
        const long on = onset[i], rel = release[i], end = rel + V.release_len;
        if (end <= t0) continue;                                             // uniform: silent before this tile begins
        const unsigned inc_i = inc[i];
        const float g = gain[i];
        if (mine && n >= on && n < end) {
            const long k = n - on;
            const long kr = n > rel ? n - rel : 0;
            const float kf = (float)k;
            const float att = k + 1 >= V.attack ? 1.0f : (float)(k + 1) * V.inv_attack;
            const float ga = g * att;
            const float er = -((float)kr * V.rel_rate);                      // the release envelope's exponent
            for (int h = 0; h < V.n_partials; ++h) {
                const unsigned long long step = (unsigned long long)V.mult[h] * inc_i;
                if (step >= 0x80000000ull) continue;                         // at or above fs / 2
                const unsigned phase = (unsigned)step * (unsigned)k;         // mod 2^32
                const float x = (float)(phase >> 8) * 5.9604644775390625e-8f;      // turns, exact: 24 bits * 2^-24
                const float e = expf(fmaf(-kf, V.rate[h], er));              // both envelopes in one exponential
                const float s = sinpif(2.0f * x);
                const float term = ((ga * V.weight[h]) * e) * s;
                acc = acc + term;
            }
        }
    }
    if (mine) pcm[p0 + j0 + threadIdx.x] = acc;
    if (peak) block_max_bits(mine ? (__float_as_uint(acc) & 0x7fffffffu) : 0u, peak + f);
}

__global__ __launch_bounds__(RN_THREADS) void pcm_peak_kernel(const float* __restrict__ pcm, const int64_t* __restrict__ pcm_ptr,
                                                              unsigned* __restrict__ peak) {
    const int f = blockIdx.y;
    const long p0 = pcm_ptr[f], len = pcm_ptr[f + 1] - p0;
    const long j0 = (long)blockIdx.x * PQ_TILE;
    if (j0 >= len) return;
    unsigned bits = 0;
#pragma unroll
    for (int q = 0; q < PQ_PER_THREAD; ++q) {
        const long j = j0 + q * RN_THREADS + threadIdx.x;
        if (j < len) {
            const unsigned b = __float_as_uint(pcm[p0 + j]) & 0x7fffffffu;
            bits = b > bits ? b : bits;
        }
    }
    block_max_bits(bits, peak + f);
}

__global__ __launch_bounds__(RN_THREADS) void pcm_quantise_kernel(const float* __restrict__ pcm, const int64_t* __restrict__ pcm_ptr,
                                                                  const float* __restrict__ peak, float full, int16_t* __restrict__ q16) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const long p0 = pcm_ptr[f], len = pcm_ptr[f + 1] - p0;
    const long j0 = (long)blockIdx.x * PQ_TILE;
    if (j0 >= len) return;
    const float pk = peak[f];
    const float s = pk == 0.f ? 0.f : full / pk;
#pragma unroll
    for (int q = 0; q < PQ_PER_THREAD; ++q) {
        const long j = j0 + q * RN_THREADS + threadIdx.x;
        if (j < len) {
            float v = rintf(pcm[p0 + j] * s);
            v = v < -32767.f ? -32767.f : v;
            v = v > 32767.f ? 32767.f : v;         // a NaN sample takes neither branch and converts to 0
            q16[p0 + j] = (int16_t)(int)v;
        }
    }
}

int check_files(const char* who, int F, long max_samples) {
    MG_CHECK_ARG(F >= 1, "%s: F = %d: at least one file", who, F);
    MG_CHECK_ARG(F <= 65535, "%s: F = %d: at most 65535 files per launch", who, F);
    MG_CHECK_ARG(max_samples >= 1, "%s: max_samples = %ld: the longest file's sample count, >= 1", who, max_samples);
    return MG_OK;
}

bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

int mg_render_notes(const int32_t* onset, const int32_t* release, const uint32_t* inc, const float* gain, const int64_t* note_ptr,
                    const int64_t* pcm_ptr, const int32_t* n_begin, const int32_t* max_len, int F, long max_samples,
                    const mg_voice* voice, float* pcm, float* peak, mg_stream_t stream) {
    MG_CHECK_ARG(onset && release && inc && gain, "mg_render_notes: null onset / release / inc / gain");
    MG_CHECK_ARG(note_ptr && pcm_ptr && n_begin && max_len, "mg_render_notes: null note_ptr / pcm_ptr / n_begin / max_len");
    MG_CHECK_ARG(voice && pcm, "mg_render_notes: null voice / pcm");
    if (int rc = check_files("mg_render_notes", F, max_samples)) return rc;
    MG_CHECK_ARG(max_samples <= 0x7fffffffL, "mg_render_notes: max_samples = %ld: a file holds fewer than 2^31 samples", max_samples);
    const mg_voice& v = *voice;
    MG_CHECK_ARG(v.n_partials >= 1 && v.n_partials <= MG_VOICE_MAX_PARTIALS, "mg_render_notes: n_partials = %d: must be in 1..%d",
                 v.n_partials, MG_VOICE_MAX_PARTIALS);
    MG_CHECK_ARG(v.attack >= 1, "mg_render_notes: attack = %d samples: must be >= 1", v.attack);
    MG_CHECK_ARG(v.release_len >= 0, "mg_render_notes: release_len = %d samples: must be >= 0", v.release_len);
    MG_CHECK_ARG(positive_finite(v.fs), "mg_render_notes: fs must be finite and positive");
    MG_CHECK_ARG(positive_finite(v.release_tau), "mg_render_notes: release_tau must be finite and positive");
    RenderVoice R;
    R.n_partials = v.n_partials;
    R.attack = v.attack;
    R.release_len = v.release_len;
    R.inv_attack = (float)(1.0 / (double)v.attack);
    R.rel_rate = (float)(1.0 / ((double)v.fs * (double)v.release_tau));
    for (int h = 0; h < MG_VOICE_MAX_PARTIALS; ++h) {
        const bool used = h < v.n_partials;
        if (used) {
            MG_CHECK_ARG(std::isfinite(v.decay[h]) && v.decay[h] >= 0.f, "mg_render_notes: decay[%d] must be finite and >= 0", h);
            MG_CHECK_ARG(std::isfinite(v.weight[h]), "mg_render_notes: weight[%d] must be finite", h);
        }
        R.mult[h] = used ? v.mult[h] : 0u;
        R.weight[h] = used ? v.weight[h] : 0.f;
        R.rate[h] = used ? (float)((double)v.decay[h] / (double)v.fs) : 0.f;
    }
    if (peak) MG_HIP(hipMemsetAsync(peak, 0, (size_t)F * sizeof(float), ST));
    const dim3 grid((unsigned)mg_cdiv(max_samples, RN_THREADS), (unsigned)F);
    hipLaunchKernelGGL(render_notes_kernel, grid, dim3(RN_THREADS), 0, ST, onset, release, inc, gain, note_ptr, pcm_ptr, n_begin,
                       max_len, R, pcm, reinterpret_cast<unsigned*>(peak));
    MG_CHECK_LAUNCH("render_notes");
    return MG_OK;
}

int mg_pcm_peak(const float* pcm, const int64_t* pcm_ptr, int F, long max_samples, float* peak, mg_stream_t stream) {
    MG_CHECK_ARG(pcm && pcm_ptr && peak, "mg_pcm_peak: null pcm / pcm_ptr / peak");
    if (int rc = check_files("mg_pcm_peak", F, max_samples)) return rc;
    MG_HIP(hipMemsetAsync(peak, 0, (size_t)F * sizeof(float), ST));
    const dim3 grid((unsigned)mg_cdiv(max_samples, PQ_TILE), (unsigned)F);
    hipLaunchKernelGGL(pcm_peak_kernel, grid, dim3(RN_THREADS), 0, ST, pcm, pcm_ptr, reinterpret_cast<unsigned*>(peak));
    MG_CHECK_LAUNCH("pcm_peak");
    return MG_OK;
}

int mg_pcm_quantise(const float* pcm, const int64_t* pcm_ptr, const float* peak, int F, long max_samples, float target, int16_t* q,
                    mg_stream_t stream) {
    MG_CHECK_ARG(pcm && pcm_ptr && peak && q, "mg_pcm_quantise: null pcm / pcm_ptr / peak / q");
    if (int rc = check_files("mg_pcm_quantise", F, max_samples)) return rc;
    MG_CHECK_ARG(target > 0.f && target <= 1.f, "mg_pcm_quantise: target must be in (0, 1]");      // false for a NaN too
    const dim3 grid((unsigned)mg_cdiv(max_samples, PQ_TILE), (unsigned)F);
    hipLaunchKernelGGL(pcm_quantise_kernel, grid, dim3(RN_THREADS), 0, ST, pcm, pcm_ptr, peak, target * 32767.0f, q);
    MG_CHECK_LAUNCH("pcm_quantise");
    return MG_OK;
}
