// Shared motifs between note rolls, transposition-invariant (melo_gan_amd/motifs.py): every (T, 4) row becomes a row of
// interval (+ rhythm class) tokens, every (query, corpus) pair of token rows gets its longest common contiguous run, every
// query position the longest run that ends there against any corpus row, and every query its k best corpus rows.  The
// definitions and the layout are in include/melo_gan_hip.h (mg_motif_tokens); the host restatement is melo_gan_amd/motifs.py.
// All integer: the results are the host's bit for bit, in any launch order.  The only atomics are integer maxima.
#include "common.h"
#include "note_decode.h"

#define ST ((hipStream_t)stream)

typedef unsigned short u16;

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_T = 4096;
constexpr int MT_PAD = 0xFFFF;
constexpr int ML_TILE = 32;             // corpus rows per workgroup of motif_lcs_kernel, eight per wave
constexpr int ML_BITWORDS = 65536 / 32; // one bit per token value: which values the tile's rows hold
constexpr int MR_MAX_K = 1024;

// floor(step * 64 + 0.5) in fp64: step * 64 is exact, so there is one rounding, the add's, with or without contraction
__device__ __forceinline__ int motif_ticks(double step_beats) {
#pragma clang fp contract(off)
    return (int)floor(step_beats * 64.0 + 0.5);
}

// One workgroup per row; lane u takes the positions u, u + 256, ...  What depends on order -- a note's rank among the
// sounding notes, its onset in ticks, and the pitch and onset of the sounding note before it -- comes from the ballot and
// an inclusive scan inside the wave, from per-wave words in LDS across waves (double-buffered: one barrier per chunk, as in
// note_stats_kernel) and from carries, which every lane derives from the same words, across chunks.
__global__ __launch_bounds__(MT_THREADS) void motif_tokens_kernel(const f32x4* __restrict__ rolls, int T, int mode,
                                                                  u16* __restrict__ tokens, int* __restrict__ lengths) {
    __shared__ int s_cnt[2][MT_WAVES], s_ticks[2][MT_WAVES], s_lastp[2][MT_WAVES], s_lastt[2][MT_WAVES];
    const long row = blockIdx.x;
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    const f32x4* src = rolls + row * T;
    u16* out = tokens + row * T;
    int n_behind = 0, t_behind = 0;     // sounding notes and ticks of the chunks behind this one
    int carry_p = -1, carry_t = 0;      // the last sounding note behind this chunk: pitch and onset
    int buf = 0;
    for (int t0 = 0; t0 < T; t0 += MT_THREADS, buf ^= 1) {
        const int t = t0 + u;
        NoteEvent e = {false, false, 0, 0, 0.0, 0.0};
        if (t < T) e = note_decode(src[t]);
        const int tk = e.valid ? motif_ticks(e.step) : 0;
        int inc = tk;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        const int onset_in = inc - tk;          // ticks of the wave's valid events in front of this one
        const int wave_ticks = __shfl(inc, 63);
        const unsigned long long m = __ballot(e.sounding);
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        const int prev_lane = below ? 63 - __clzll((long long)below) : 0;
        const int last_lane = m ? 63 - __clzll((long long)m) : 0;
        const int prev_p_in = __shfl(e.pitch, prev_lane), prev_t_in = __shfl(onset_in, prev_lane);
        const int last_p_in = __shfl(e.pitch, last_lane), last_t_in = __shfl(onset_in, last_lane);
        if (lane == 0) {
            s_cnt[buf][w] = __popcll(m);
            s_ticks[buf][w] = wave_ticks;
            s_lastp[buf][w] = m ? last_p_in : -1;
            s_lastt[buf][w] = last_t_in;
        }
        __syncthreads();
        int cnt_base = 0, tick_base = 0, before_p = -1, before_t = 0;
        int run_cnt = n_behind, run_ticks = t_behind, last_p = carry_p, last_t = carry_t;
#pragma unroll
        for (int j = 0; j < MT_WAVES; ++j) {
            if (j == w) {
                cnt_base = run_cnt;
                tick_base = run_ticks;
                before_p = last_p;
                before_t = last_t;
            }
            if (s_lastp[buf][j] >= 0) {
                last_p = s_lastp[buf][j];
                last_t = run_ticks + s_lastt[buf][j];
            }
            run_cnt += s_cnt[buf][j];
            run_ticks += s_ticks[buf][j];
        }
        n_behind = run_cnt;
        t_behind = run_ticks;
        carry_p = last_p;
        carry_t = last_t;
        if (e.sounding) {
            const int rank = cnt_base + __popcll(below);
            if (rank >= 1) {
                const int prev_p = below ? prev_p_in : before_p;
                const int prev_t = below ? tick_base + prev_t_in : before_t;
                const int ioi = tick_base + onset_in - prev_t;
                const int rhythm = mode ? 0 : (ioi >= 12) + (ioi >= 24) + (ioi >= 48) + (ioi >= 96) + (ioi >= 192);
                out[rank - 1] = (u16)((e.pitch - prev_p + 64) | (rhythm << 7));
            }
        }
    }
    const int len = n_behind > 1 ? n_behind - 1 : 0;
    for (int j = len + u; j < T; j += MT_THREADS) out[j] = (u16)MT_PAD;
    if (u == 0) lengths[row] = len;
}

__device__ __forceinline__ long long motif_wave_max(long long v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One cell of a lane's diagonal: a and b are the two tokens, `run` the run that ended in the cell before, `cut` (WRAP only)
// that this cell lies in b's first column, where nothing carries on.  A run of two or more that ends in front of this cell
// goes to reach; the cell's own run to the lane's key.
template <bool WRAP>
__device__ __forceinline__ void motif_step(int i, unsigned a, unsigned b, bool active, bool cut, int& run, unsigned& key,
                                           int* s_reach) {
    const bool eq = a == b && active;
    const int nr = eq ? (WRAP && cut ? 1 : run + 1) : 0;
    if (run >= 2 && (WRAP ? nr != run + 1 : !eq)) atomicMax(&s_reach[i - 1], run);
    run = nr;
    key = max(key, ((unsigned)nr << 16) | (unsigned)(0xFFFF - i));
}

// Workgroup (tile, q): query row q against the corpus rows tile * 32 .. + 31, wave w taking the rows w, w + 4, ...  The
// query's tokens lie in LDS, and each wave stages its corpus row b (Mc tokens) in LDS words of its own.  Lane k walks the
// wrapped diagonal j = (i + k) mod Mc for i = 0 .. Mq - 1, 64 diagonals per pass: a[i] is one address for the whole wave (a
// broadcast), b[j] 64 consecutive halfwords (32 banks, two lanes per word: no conflict), and every lane makes exactly Mq
// steps.  A run is cut where j returns to 0: nothing carries from b's end into its start.  The best cell of a lane is one
// 32-bit maximum of (run << 16) | (0xFFFF - i); i only grows, so the earliest i of a run length wins, and j follows from i
// and k.  Across lanes, passes and rows the packed 64-bit value orders by (L, smaller i, smaller j).
// reach: a maximal run of r >= 2 tokens that ends at query position e is one LDS atomic maximum on word e; runs of one token
// are taken from a bitmap of the token values the tile's rows hold.  The words go to the global buffer by atomic maxima;
// motif_reach_kernel then spreads every run over the positions it covers.
__global__ __launch_bounds__(MT_THREADS) void motif_lcs_kernel(const u16* __restrict__ q_tokens, const int* __restrict__ q_len,
                                                               const u16* __restrict__ c_tokens, const int* __restrict__ c_len,
                                                               const int* __restrict__ q_groups, const int* __restrict__ c_groups,
                                                               long Nc, int T, long long* __restrict__ packed,
                                                               int* __restrict__ reach) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Tp = (T + 1) & ~1;
    int* s_reach = reinterpret_cast<int*>(smem);                // [T]
    unsigned* s_bits = reinterpret_cast<unsigned*>(s_reach + T);    // [ML_BITWORDS]
    u16* s_a = reinterpret_cast<u16*>(s_bits + ML_BITWORDS);    // [Tp]
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    u16* s_b = s_a + (long)(1 + w) * Tp;                        // [Tp] of this wave
    const long q = blockIdx.y;
    const int Mq = min(max(q_len[q], 0), T);
    for (int i = u; i < T; i += MT_THREADS) {
        s_a[i] = q_tokens[q * T + i];
        s_reach[i] = 0;
    }
    for (int i = u; i < ML_BITWORDS; i += MT_THREADS) s_bits[i] = 0u;
    __syncthreads();
    const long c_lo = (long)blockIdx.x * ML_TILE;
    const long c_hi = min(Nc, c_lo + ML_TILE);
    const int qg = q_groups ? q_groups[q] : 0;
    for (long c = c_lo + w; c < c_hi; c += MT_WAVES) {
        const bool skip = q_groups && qg == c_groups[c];
        const int Mc = skip ? 0 : min(max(c_len[c], 0), T);
        for (int j = lane; j < Mc; j += 64) {
            const unsigned tok = c_tokens[c * T + j];
            s_b[j] = (u16)tok;
            atomicOr(&s_bits[tok >> 5], 1u << (tok & 31u));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        long long best = 0;
        for (int k0 = 0; k0 < Mc; k0 += 64) {
            const int k = k0 + lane;
            const bool active = k < Mc;
            int j = active ? k : k0;    // a lane without a diagonal walks the pass' first one, and matches nothing
            int run = 0;
            unsigned key = 0u;
            // Lane k returns to j = 0 at the steps i = n * Mc - k: for the 64 lanes of the pass, inside the windows
            // [n * Mc - k0 - 63, n * Mc - k0].  Between the windows j = i + k - const for every lane: four steps per trip,
            // their eight LDS reads ahead of the first.
            int i = 0;
            for (int wrap = Mc - k0 - 63; i < Mq; wrap += Mc) {
                const int plain_end = min(Mq, wrap);
                for (; i + 4 <= plain_end; i += 4, j += 4) {
                    const unsigned a0 = s_a[i], a1 = s_a[i + 1], a2 = s_a[i + 2], a3 = s_a[i + 3];
                    // b[j .. j + 3] from the three aligned words that hold them: the wave reads 34 consecutive words, two
                    // lanes per word, where an 8-byte read per lane at a 2-byte stride would fetch every token four times
                    const unsigned* wb = reinterpret_cast<const unsigned*>(s_b) + (j >> 1);
                    const unsigned d0 = wb[0], d1 = wb[1], d2 = wb[2], odd = (unsigned)(j & 1) << 4;
                    const unsigned e0 = __builtin_amdgcn_alignbit(d1, d0, odd), e1 = __builtin_amdgcn_alignbit(d2, d1, odd);
                    const unsigned b0 = e0 & 0xFFFFu, b1 = e0 >> 16, b2 = e1 & 0xFFFFu, b3 = e1 >> 16;
                    motif_step<false>(i, a0, b0, active, false, run, key, s_reach);
                    motif_step<false>(i + 1, a1, b1, active, false, run, key, s_reach);
                    motif_step<false>(i + 2, a2, b2, active, false, run, key, s_reach);
                    motif_step<false>(i + 3, a3, b3, active, false, run, key, s_reach);
                }
                for (; i < plain_end; ++i, ++j) motif_step<false>(i, s_a[i], s_b[j], active, false, run, key, s_reach);
                const int window_end = min(Mq, wrap + 64);
                if (j == Mc) j = 0;     // the pass' last lane returns at the window's first step
                for (; i < window_end; ++i) {
                    motif_step<true>(i, s_a[i], s_b[j], active, j == 0, run, key, s_reach);
                    j = j + 1 == Mc ? 0 : j + 1;
                }
            }
            if (run >= 2) atomicMax(&s_reach[Mq - 1], run);
            const int L = (int)(key >> 16);
            if (L > 0) {
                const int i_end = 0xFFFF - (int)(key & 0xFFFFu);
                const int j_end = (i_end + k) % Mc;
                const long long p = ((long long)L << 32) | ((long long)(0xFFFF - i_end) << 16) | (long long)(0xFFFF - j_end);
                best = p > best ? p : best;
            }
        }
        best = motif_wave_max(best);
        if (lane == 0) packed[q * Nc + c] = best;
        __builtin_amdgcn_wave_barrier();        // the row's last reads stay in front of the next row's staging stores
    }
    __syncthreads();
    for (int i = u; i < Mq; i += MT_THREADS) {
        const unsigned tok = s_a[i];
        int r = s_reach[i];
        if (r == 0 && ((s_bits[tok >> 5] >> (tok & 31u)) & 1u)) r = 1;
        if (r > 0) atomicMax(&reach[q * T + i], r);
    }
}

// One workgroup per query row, in place.  In: R[e] = the longest run that ends at e (0: none).  Out: reach[i] = the longest
// run(i, .) = max over e >= i of R[e] - (e - i) = i + the suffix maximum of R[e] - e; an e without a run adds i - e <= 0.
// Chunks of 256 positions from the row's end: the suffix maximum inside a wave by shuffles, across waves from LDS
// (double-buffered), across chunks from `carry`.
__global__ __launch_bounds__(MT_THREADS) void motif_reach_kernel(int* __restrict__ reach, int T) {
    __shared__ int s_w[2][MT_WAVES];
    const int NONE = -(1 << 24);
    int* R = reach + (long)blockIdx.x * T;
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    int carry = NONE, buf = 0;
    for (int ch = (T - 1) / MT_THREADS; ch >= 0; --ch, buf ^= 1) {
        const int i = ch * MT_THREADS + u;
        int v = NONE;
        if (i < T) {
            const int r = R[i];
            if (r > 0) v = r - i;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(v, d);
            if (lane + d < 64) v = max(v, o);
        }
        const int wave_max = __shfl(v, 0);
        if (lane == 0) s_w[buf][w] = wave_max;
        __syncthreads();
        int after = carry, all = carry;
#pragma unroll
        for (int j = 0; j < MT_WAVES; ++j) {
            const int x = s_w[buf][j];
            all = max(all, x);
            if (j > w) after = max(after, x);
        }
        carry = all;
        if (i < T) R[i] = max(0, i + max(v, after));
    }
}

// One workgroup per query row, k rounds.  Round r takes the best (value, then lower index) among the corpus rows behind
// round r - 1's pick in that order: a lane's candidates, a butterfly over the wave, the four waves from LDS (double-buffered).
__global__ __launch_bounds__(MT_THREADS) void motif_rank_kernel(const long long* __restrict__ packed, long Nc, int k,
                                                                long long* __restrict__ vals, int* __restrict__ idx) {
    __shared__ long long s_v[2][MT_WAVES];
    __shared__ int s_c[2][MT_WAVES];
    const long q = blockIdx.x;
    const long long* row = packed + q * Nc;
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    const int NONE = 0x7FFFFFFF;
    long long prev_v = 0;
    int prev_c = -1, buf = 0;       // prev_c < 0: nothing picked yet
    for (int r = 0; r < k; ++r) {
        if (r >= Nc) {
            if (u == 0) {
                vals[q * k + r] = 0;
                idx[q * k + r] = -1;
            }
            continue;
        }
        long long bv = 0;
        int bc = NONE;
        for (long c = u; c < Nc; c += MT_THREADS) {
            const long long v = row[c];
            const bool behind = prev_c < 0 || v < prev_v || (v == prev_v && c > prev_c);
            if (behind && (bc == NONE || v > bv)) {     // c only grows: an equal value never replaces
                bv = v;
                bc = (int)c;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const long long ov = __shfl_xor(bv, m, 64);
            const int oc = __shfl_xor(bc, m, 64);
            if (oc != NONE && (bc == NONE || ov > bv || (ov == bv && oc < bc))) {
                bv = ov;
                bc = oc;
            }
        }
        if (lane == 0) {
            s_v[buf][w] = bv;
            s_c[buf][w] = bc;
        }
        __syncthreads();
        bv = s_v[buf][0];
        bc = s_c[buf][0];
#pragma unroll
        for (int j = 1; j < MT_WAVES; ++j) {
            const long long ov = s_v[buf][j];
            const int oc = s_c[buf][j];
            if (oc != NONE && (bc == NONE || ov > bv || (ov == bv && oc < bc))) {
                bv = ov;
                bc = oc;
            }
        }
        buf ^= 1;
        prev_v = bv;        // r < Nc: a row is left, so bc != NONE
        prev_c = bc;
        if (u == 0) {
            vals[q * k + r] = bv;
            idx[q * k + r] = bc;
        }
    }
}

extern "C" {

int mg_motif_corpus_tile(void) { return ML_TILE; }

int mg_motif_tokens(const float* rolls, long N, int T, int mode, uint16_t* tokens, int32_t* lengths, mg_stream_t stream) {
    MG_CHECK_ARG(rolls && tokens && lengths, "mg_motif_tokens: null rolls / tokens / lengths");
    MG_CHECK_ARG(N >= 1 && N <= 0x7FFFFFFFL, "mg_motif_tokens: N = %ld: 1..2^31 - 1", N);
    MG_CHECK_ARG(T >= 1 && T <= MT_MAX_T, "mg_motif_tokens: T = %d: 1..%d", T, MT_MAX_T);
    MG_CHECK_ARG(mode == MG_MOTIF_INTERVAL_RHYTHM || mode == MG_MOTIF_INTERVAL,
                 "mg_motif_tokens: mode = %d: MG_MOTIF_INTERVAL_RHYTHM or MG_MOTIF_INTERVAL", mode);
    MG_CHECK_ARG(((uintptr_t)rolls & 15) == 0 && ((uintptr_t)tokens & 1) == 0 && ((uintptr_t)lengths & 3) == 0,
                 "mg_motif_tokens: rolls must be 16-byte, tokens 2-byte and lengths 4-byte aligned");
    hipLaunchKernelGGL(motif_tokens_kernel, dim3((unsigned)N), dim3(MT_THREADS), 0, ST, (const f32x4*)rolls, T, mode, (u16*)tokens,
                       (int*)lengths);
    MG_CHECK_LAUNCH("motif_tokens");
    return MG_OK;
}

int mg_motif_lcs(const uint16_t* q_tokens, const int32_t* q_len, int Nq, const uint16_t* c_tokens, const int32_t* c_len, long Nc,
                 int T, const int32_t* q_groups, const int32_t* c_groups, int64_t* packed, int32_t* reach, mg_stream_t stream) {
    static std::atomic<uint64_t> optin{0};
    MG_CHECK_ARG(q_tokens && q_len && c_tokens && c_len && packed && reach,
                 "mg_motif_lcs: null q_tokens / q_len / c_tokens / c_len / packed / reach");
    MG_CHECK_ARG((q_groups == nullptr) == (c_groups == nullptr), "mg_motif_lcs: q_groups and c_groups go together");
    MG_CHECK_ARG(Nq >= 1 && Nq <= 65535, "mg_motif_lcs: Nq = %d: 1..65535", Nq);
    MG_CHECK_ARG(Nc >= 1 && Nc <= 0x7FFFFFFFL, "mg_motif_lcs: Nc = %ld: 1..2^31 - 1", Nc);
    MG_CHECK_ARG(T >= 1 && T <= MT_MAX_T, "mg_motif_lcs: T = %d: 1..%d", T, MT_MAX_T);
    MG_CHECK_ARG((((uintptr_t)q_tokens | (uintptr_t)c_tokens) & 1) == 0, "mg_motif_lcs: the token buffers must be 2-byte aligned");
    MG_CHECK_ARG((((uintptr_t)q_len | (uintptr_t)c_len | (uintptr_t)q_groups | (uintptr_t)c_groups | (uintptr_t)reach) & 3) == 0 &&
                     ((uintptr_t)packed & 7) == 0,
                 "mg_motif_lcs: the lengths, the groups and reach must be 4-byte, packed 8-byte aligned");
    const int Tp = (T + 1) & ~1;
    // the last wave's aligned word reads may reach two tokens past its row
    const size_t lds = (size_t)T * 4 + (size_t)ML_BITWORDS * 4 + (size_t)(1 + MT_WAVES) * Tp * 2 + 8;
    if (lds > 48 * 1024 && mg_lds_optin((const void*)motif_lcs_kernel, optin) != MG_OK) return MG_EHIP;
    MG_HIP(hipMemsetAsync(reach, 0, (size_t)Nq * T * sizeof(int32_t), ST));
    hipLaunchKernelGGL(motif_lcs_kernel, dim3((unsigned)mg_cdiv(Nc, ML_TILE), (unsigned)Nq), dim3(MT_THREADS), lds, ST,
                       (const u16*)q_tokens, (const int*)q_len, (const u16*)c_tokens, (const int*)c_len, (const int*)q_groups,
                       (const int*)c_groups, Nc, T, (long long*)packed, (int*)reach);
    MG_CHECK_LAUNCH("motif_lcs");
    hipLaunchKernelGGL(motif_reach_kernel, dim3((unsigned)Nq), dim3(MT_THREADS), 0, ST, (int*)reach, T);
    MG_CHECK_LAUNCH("motif_reach");
    return MG_OK;
}

int mg_motif_rank(const int64_t* packed, int Nq, long Nc, int k, int64_t* vals, int32_t* idx, mg_stream_t stream) {
    MG_CHECK_ARG(packed && vals && idx, "mg_motif_rank: null packed / vals / idx");
    MG_CHECK_ARG(Nq >= 1 && Nq <= 0x7FFFFFFF, "mg_motif_rank: Nq = %d: must be positive", Nq);
    MG_CHECK_ARG(Nc >= 1 && Nc <= 0x7FFFFFFEL, "mg_motif_rank: Nc = %ld: 1..2^31 - 2", Nc);
    MG_CHECK_ARG(k >= 1 && k <= MR_MAX_K, "mg_motif_rank: k = %d: 1..%d", k, MR_MAX_K);
    MG_CHECK_ARG((((uintptr_t)packed | (uintptr_t)vals) & 7) == 0 && ((uintptr_t)idx & 3) == 0,
                 "mg_motif_rank: packed and vals must be 8-byte, idx 4-byte aligned");
    hipLaunchKernelGGL(motif_rank_kernel, dim3((unsigned)Nq), dim3(MT_THREADS), 0, ST, (const long long*)packed, Nc, k,
                       (long long*)vals, (int*)idx);
    MG_CHECK_LAUNCH("motif_rank");
    return MG_OK;
}

}  // extern "C"
