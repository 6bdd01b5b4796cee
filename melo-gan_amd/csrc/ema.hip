// Exponential moving average of the generator's flat parameter buffer (melo_gan_amd/gan/engine.py: GanEngine.g_update), after
// Yazici et al. 2019: a read-only rider behind the generator's Adam launch.  The shadow is fp64 -- at decay 0.999 the increment
// (1 - d)(p - s) is routinely below half an ulp of an fp32 s, which would then stop moving -- and every operation is rounded on
// its own (no contraction), so the shadow is a defined function of its inputs: melo_gan_amd/gan/ema.py restates it in numpy and
// tests/test_ema_gpu.py compares bit for bit.  Memory-bound streaming: 20 bytes per parameter, no LDS, no atomics.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_MAX_BLOCKS = 2048;       // 256 CUs x 8 workgroups; the rest of the buffer by grid stride

typedef double f64x2 __attribute__((ext_vector_type(2)));

// The decay of this update.  t = averaged updates before this one: the Adam step count, which the update in front of this
// launch has already advanced, less one, less the count at which averaging began.  ramp: min(decay, (1 + t) / (10 + t)), the
// warm-up that keeps the first updates from being averaged against the initial weights for 1 / (1 - decay) steps.  Every lane
// derives the same value from the same word; nothing but the shadow is written, so the launch replays with constant arguments.
__device__ __forceinline__ double ema_decay_now(const double* __restrict__ adam_state, double step_offset, double decay, int ramp) {
#pragma clang fp contract(off)
    if (!ramp) return decay;
    const double t = (adam_state[0] - 1.0) - step_offset;
    const double r = (1.0 + t) / (10.0 + t);
    return r < decay ? r : decay;
}

__device__ __forceinline__ double ema_update(double s, float p, double omd) {
#pragma clang fp contract(off)
    const double diff = (double)p - s;
    const double inc = omd * diff;
    return s + inc;
}

// vec = 1: p is 16-byte and shadow 16-byte aligned: a lane takes 4 parameters per iteration (one 16-byte load of p, two
// 16-byte loads and stores of the shadow); the n % 4 tail, or everything when vec = 0, goes element by element.
__global__ __launch_bounds__(EMA_THREADS) void ema_flat_kernel(const float* __restrict__ p, double* __restrict__ shadow, long n,
                                                               double decay, int ramp, const double* __restrict__ adam_state,
                                                               double step_offset, int vec) {
#pragma clang fp contract(off)
    const double d = ema_decay_now(adam_state, step_offset, decay, ramp);
    const double omd = 1.0 - d;
    const long tid = (long)blockIdx.x * EMA_THREADS + threadIdx.x, stride = (long)gridDim.x * EMA_THREADS;
    const long nq = vec ? (n >> 2) : 0;
    const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
    f64x2* __restrict__ s2 = reinterpret_cast<f64x2*>(shadow);
    for (long q = tid; q < nq; q += stride) {
        const f32x4 pv = p4[q];
        f64x2 a = s2[2 * q], b = s2[2 * q + 1];
        a[0] = ema_update(a[0], pv[0], omd);
        a[1] = ema_update(a[1], pv[1], omd);
        b[0] = ema_update(b[0], pv[2], omd);
        b[1] = ema_update(b[1], pv[3], omd);
        s2[2 * q] = a;
        s2[2 * q + 1] = b;
    }
    for (long i = 4 * nq + tid; i < n; i += stride) shadow[i] = ema_update(shadow[i], p[i], omd);
}

}  // namespace

int mg_ema_flat(const float* p, double* shadow, long n, double decay, int ramp, const double* adam_state, double step_offset,
                mg_stream_t stream) {
    MG_CHECK_ARG(p && shadow && adam_state, "mg_ema_flat: null p / shadow / adam_state");
    MG_CHECK_ARG(n >= 1, "mg_ema_flat: n must be positive");
    MG_CHECK_ARG(decay >= 0.0 && decay < 1.0, "mg_ema_flat: decay must be in [0, 1)");     // false for a NaN too
    const int vec = ((((uintptr_t)p) | ((uintptr_t)shadow)) & 15) == 0 && n >= 4;
    long nb = mg_cdiv(vec ? mg_cdiv(n, 4) : n, EMA_THREADS);
    if (nb > EMA_MAX_BLOCKS) nb = EMA_MAX_BLOCKS;
    hipLaunchKernelGGL(ema_flat_kernel, dim3((unsigned)nb), dim3(EMA_THREADS), 0, ST, p, shadow, n, decay, ramp ? 1 : 0, adam_state,
                       step_offset, vec);
    MG_CHECK_LAUNCH("ema_flat");
    return MG_OK;
}
