// Edits in the VAE's latent space (melo_gan_amd/ae/edit.py): the decoder's input for a chunk of edited latents, and what a
// decode -> re-encode round trip keeps of each edit.  One 64-lane workgroup per row in both; a row depends on its own
// descriptors (and, for its normals, on its key and the seed) alone.  The layout is in include/melo_gan_hip.h (mg_latent_rows,
// mg_latent_cycle); the host restatement is melo_gan_amd/ae/latent_edit.py.  No atomics: every output word has one writer and a
// fixed summation order.
#include "common.h"

#define ST ((hipStream_t)stream)

constexpr int LE_MAX_L = 1024;
constexpr unsigned LAT_TAG = 0x4C415400u;       // keeps these counters apart from gen_inputs_kernel's (GEN_TAG) and rng_fill_kernel's

enum { LE_PAD = 0, LE_PRIOR = 1, LE_POST = 2 };

// A row that names an index outside its array reads nothing of that array: the host refuses such rows (ae/edit.py), and a
// caller that sends one all the same finds NaN where the row's result would be.
__device__ __forceinline__ bool le_row_ok(int kind, int a, int b, int dir, int n_src, int n_dir, bool needs_b) {
    if (kind != LE_PRIOR && kind != LE_POST) return false;
    if (dir >= n_dir) return false;
    if (kind == LE_POST && (a < 0 || a >= n_src || (needs_b && (b < 0 || b >= n_src)))) return false;
    return true;
}

// z[r, :] = base + alpha * dirs[dir] + sigma * s * n in fp64, rounded once at the store (mg_latent_rows).  The slerp angle
// follows gen_inputs_mix_kernel: per-lane partial sums over the lane's element blocks q = lane, lane + 64, .. in element order,
// a fixed butterfly over the 64 lanes (every lane ends with the same bits).
__global__ __launch_bounds__(64) void latent_rows_kernel(const float* __restrict__ mu, const float* __restrict__ logvar, int n_src,
                                                         const float* __restrict__ dirs, int n_dir, const int* __restrict__ kind,
                                                         const int* __restrict__ src_a, const int* __restrict__ src_b,
                                                         const float* __restrict__ t, const int* __restrict__ dir,
                                                         const float* __restrict__ alpha, const float* __restrict__ sigma,
                                                         const int* __restrict__ key, int L, int interp, unsigned long long seed,
                                                         float* __restrict__ z) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    float* out = z + (long)r * L;
    const int kd = kind[r];
    if (kd == LE_PAD) {
        for (int i = lane; i < L; i += 64) out[i] = 0.f;
        return;
    }
    const int a = src_a[r], b = src_b[r], dr = dir[r];
    const float tr = t[r], al = alpha[r], sg = sigma[r];
    const bool post = kd == LE_POST;
    const bool only_a = !post || tr == 0.f || a == b, only_b = !only_a && tr == 1.f;
    if (!le_row_ok(kd, a, b, dr, n_src, n_dir, !only_a)) {
        for (int i = lane; i < L; i += 64) out[i] = __builtin_nanf("");
        return;
    }
    const float* ma = post ? mu + (long)a * L : nullptr;
    const float* mb = post && !only_a ? mu + (long)b * L : nullptr;
    const float* lv = post ? logvar + (long)a * L : nullptr;
    const float* dv = (dr >= 0 && al != 0.f) ? dirs + (long)dr * L : nullptr;
    const int nb = (L + 3) >> 2;
    double ca = 1.0, cb = 0.0;
    if (!only_a && !only_b) {
        const double td = (double)tr;
        ca = 1.0 - td;
        cb = td;
        if (interp == 1) {
            double dot = 0.0, na = 0.0, nbb = 0.0;
            for (int q = lane; q < nb; q += 64)
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < L) {
                        const double x = (double)ma[4 * q + j], y = (double)mb[4 * q + j];
                        dot = dot + x * y;
                        na = na + x * x;
                        nbb = nbb + y * y;
                    }
            for (int m = 1; m < 64; m <<= 1) {
                dot = dot + __shfl_xor(dot, m, 64);
                na = na + __shfl_xor(na, m, 64);
                nbb = nbb + __shfl_xor(nbb, m, 64);
            }
            const double theta = acos(fmin(fmax(dot / (sqrt(na) * sqrt(nbb)), -1.0), 1.0));    // a NaN quotient: theta = pi
            const double s = sin(theta);
            if (s >= 0x1p-20) {                 // otherwise (anti)parallel or zero vectors: the chord
                ca = sin((1.0 - td) * theta) / s;
                cb = sin(td * theta) / s;
            }
        }
    }
    const int piece = key[2 * r], sample = key[2 * r + 1];
    for (int q = lane; q < nb; q += 64) {
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (sg != 0.f) {
            unsigned c[4] = {(unsigned)q, LAT_TAG, (unsigned)piece, (unsigned)sample};
            philox4(c, (unsigned)seed, (unsigned)(seed >> 32));
            box_muller4(c, n);
        }
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * q + j;
            if (col >= L) break;
            double v = 0.0;
            if (post) v = only_a ? (double)ma[col] : only_b ? (double)mb[col] : ca * (double)ma[col] + cb * (double)mb[col];
            if (dv) v = v + (double)al * (double)dv[col];
            if (sg != 0.f) {
                const double s = post ? exp(0.5 * (double)lv[col]) : 1.0;
                v = v + ((double)sg * s) * (double)n[j];
            }
            out[col] = (float)v;
        }
    }
}

// out[r, 0:6] (mg_latent_cycle): lane u sums the elements u, u + 64, .. in that order, then a fixed butterfly over the wave.
__global__ __launch_bounds__(64) void latent_cycle_kernel(const float* __restrict__ z, const float* __restrict__ mu2,
                                                          const float* __restrict__ mu, int n_src, const float* __restrict__ dirs,
                                                          int n_dir, const int* __restrict__ kind, const int* __restrict__ src_a,
                                                          const int* __restrict__ dir, int L, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    double* o = out + (long)r * 6;
    const int kd = kind[r];
    if (kd == LE_PAD) {
        if (lane < 6) o[lane] = 0.0;
        return;
    }
    const int a = src_a[r], dr = dir[r];
    if (!le_row_ok(kd, a, 0, dr, n_src, n_dir, false)) {
        if (lane < 6) o[lane] = __builtin_nan("");
        return;
    }
    const float* zr = z + (long)r * L;
    const float* m2 = mu2 + (long)r * L;
    const float* ma = kd == LE_POST ? mu + (long)a * L : nullptr;
    const float* dv = dr >= 0 ? dirs + (long)dr * L : nullptr;
    double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < L; i += 64) {
        const double zi = (double)zr[i], mi = (double)m2[i], m0 = ma ? (double)ma[i] : 0.0;
        const double e0 = zi - m0, e1 = mi - zi, e2 = mi - m0;
        w[0] = w[0] + e0 * e0;
        w[1] = w[1] + e1 * e1;
        w[2] = w[2] + e2 * e2;
        if (dv) {
            const double d = (double)dv[i];
            w[3] = w[3] + e2 * d;
            w[4] = w[4] + e0 * d;
            w[5] = w[5] + d * d;
        }
    }
    for (int m = 1; m < 64; m <<= 1)
        for (int k = 0; k < 6; ++k) w[k] = w[k] + __shfl_xor(w[k], m, 64);
    if (lane == 0)
        for (int k = 0; k < 6; ++k) o[k] = w[k];
}

extern "C" {

int mg_latent_rows(const float* mu, const float* logvar, int n_src, const float* dirs, int n_dir, const int32_t* kind,
                   const int32_t* src_a, const int32_t* src_b, const float* t, const int32_t* dir, const float* alpha,
                   const float* sigma, const int32_t* key, int rows, int L, int interp, uint64_t seed, float* z, mg_stream_t stream) {
    MG_CHECK_ARG(kind && src_a && src_b && t && dir && alpha && sigma && key && z,
                 "mg_latent_rows: null kind / src_a / src_b / t / dir / alpha / sigma / key / z");
    MG_CHECK_ARG(L >= 1 && L <= LE_MAX_L, "mg_latent_rows: L = %d: 1..%d", L, LE_MAX_L);
    MG_CHECK_ARG(rows >= 0, "mg_latent_rows: rows = %d: must be >= 0", rows);
    MG_CHECK_ARG(n_src >= 0 && n_dir >= 0, "mg_latent_rows: n_src = %d, n_dir = %d: must be >= 0", n_src, n_dir);
    MG_CHECK_ARG((mu && logvar) || n_src == 0, "mg_latent_rows: null mu / logvar with n_src = %d", n_src);
    MG_CHECK_ARG(dirs || n_dir == 0, "mg_latent_rows: null dirs with n_dir = %d", n_dir);
    MG_CHECK_ARG(interp == 0 || interp == 1, "mg_latent_rows: interp = %d: 0 (lerp) or 1 (slerp)", interp);
    if (rows == 0) return MG_OK;
    hipLaunchKernelGGL(latent_rows_kernel, dim3((unsigned)rows), dim3(64), 0, ST, mu, logvar, n_src, dirs, n_dir, (const int*)kind,
                       (const int*)src_a, (const int*)src_b, t, (const int*)dir, alpha, sigma, (const int*)key, L, interp,
                       (unsigned long long)seed, z);
    MG_CHECK_LAUNCH("latent_rows");
    return MG_OK;
}

int mg_latent_cycle(const float* z, const float* mu2, const float* mu, int n_src, const float* dirs, int n_dir, const int32_t* kind,
                    const int32_t* src_a, const int32_t* dir, int rows, int L, double* out, mg_stream_t stream) {
    MG_CHECK_ARG(z && mu2 && kind && src_a && dir && out, "mg_latent_cycle: null z / mu2 / kind / src_a / dir / out");
    MG_CHECK_ARG(L >= 1 && L <= LE_MAX_L, "mg_latent_cycle: L = %d: 1..%d", L, LE_MAX_L);
    MG_CHECK_ARG(rows >= 0, "mg_latent_cycle: rows = %d: must be >= 0", rows);
    MG_CHECK_ARG(n_src >= 0 && n_dir >= 0, "mg_latent_cycle: n_src = %d, n_dir = %d: must be >= 0", n_src, n_dir);
    MG_CHECK_ARG(mu || n_src == 0, "mg_latent_cycle: null mu with n_src = %d", n_src);
    MG_CHECK_ARG(dirs || n_dir == 0, "mg_latent_cycle: null dirs with n_dir = %d", n_dir);
    MG_CHECK_ARG(((uintptr_t)out & 7) == 0, "mg_latent_cycle: out must be 8-byte aligned");
    if (rows == 0) return MG_OK;
    hipLaunchKernelGGL(latent_cycle_kernel, dim3((unsigned)rows), dim3(64), 0, ST, z, mu2, mu, n_src, dirs, n_dir, (const int*)kind,
                       (const int*)src_a, (const int*)dir, L, out);
    MG_CHECK_LAUNCH("latent_cycle");
    return MG_OK;
}

}  // extern "C"
