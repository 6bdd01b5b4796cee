// The decode of one time position of a (T, 4) note row into a note event: the generator's output contract
// (melo_gan_amd/midi.py, notes_from_roll; include/melo_gan_hip.h, mg_note_stats).  Shared by every kernel that counts notes
// (note_metrics.hip, vae_metrics.hip), so that they cannot disagree about what a note is.
#pragma once
#include "common.h"

constexpr int NS_PITCH_LO = 36, NS_PITCH_HI = 96;

struct NoteEvent {
    bool valid, sounding;       // all four values finite; valid and not a rest
    int pitch, vel;
    double dur, step;           // beats
};

// The decode of one time position.  Every fp32 operation is rounded on its own, as numpy evaluates the scalar code of
// notes_from_roll.  Contraction is off for this function and the operators are plain: the __fmul_rn / __fadd_rn wrappers
// are inline functions of their own, outside the pragma's reach, and hipcc does fuse a pair of them.  So 60 + q * 67 stays
// a multiply and an add, and the divide by 1.2f is the compiler's correctly rounded one (v_div_scale / fmas / fixup).
// Clamping in float before the conversion equals int() followed by the integer clip and also takes an overflow to infinity.
__device__ __forceinline__ NoteEvent note_decode(const f32x4 x) {
#pragma clang fp contract(off)
    NoteEvent e;
    e.valid = __builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]) && __builtin_isfinite(x[3]);
    const float thr = -0.2f;
    e.sounding = e.valid && !(x[1] < thr);
    const float pf = (x[0] + 1.0f) * 63.5f;
    e.pitch = (int)fminf(fmaxf(pf, (float)NS_PITCH_LO), (float)NS_PITCH_HI);
    const float q = (x[1] - thr) / 1.2f;
    const float qs = q * 67.0f;
    const float vf = 60.0f + qs;
    e.vel = (int)fminf(fmaxf(vf, 0.0f), 127.0f);
    const float df = ((x[2] + 1.0f) / 2.0f) * 4.0f;
    const float sf = ((x[3] + 1.0f) / 2.0f) * 4.0f;
    e.dur = df > 0.25f ? (double)df : 0.25;     // max(0.25, .) and max(0.1, .): the comparison is made in fp32, the
    e.step = sf > 0.1f ? (double)sf : 0.1;      // constant enters as the Python double
    return e;
}

// The inverse on the decode's image (melo_gan_amd/midi_rolls.py, host_roll_encode; include/melo_gan_hip.h, mg_roll_encode): one
// event (pitch, velocity, dur_q, step_q), durations and steps in 1/64 beat, to the four values that note_decode takes back to
// it.  A velocity below 0 marks a rest, (-1, -1, -1, step).  What lies outside the image is clamped into it, and `fired` says
// which clamps did: the bits index mg_roll_encode's eight loss counts.
constexpr int NE_VEL_LO = 60, NE_VEL_HI = 127, NE_DUR_LO = 16, NE_Q_HI = 256, NE_STEP_FLOOR = 7;
enum { NE_PITCH_UP = 1, NE_PITCH_DOWN = 2, NE_VEL_UP = 4, NE_DUR_UP = 8, NE_DUR_DOWN = 16, NE_STEP_SHORT = 32, NE_STEP_ZERO = 64,
       NE_REST = 128 };

// Same rules as note_decode: contraction off, plain operators, every fp32 operation rounded on its own, so that numpy's
// float32 arithmetic gives the same bits.  (p + 0.5) / 63.5 - 1 lands inside the interval that decodes to p for every p in
// 36..96; ((v + 0.5 - 60) / 67) * 1.2 - 0.2 does for v in 60..126 and 127 takes 1.0; q / 128 - 1 is exact for q in 0..256.
__device__ __forceinline__ f32x4 note_encode(int pitch, int vel, int dur_q, int step_q, unsigned& fired) {
#pragma clang fp contract(off)
    const int s = min(max(step_q, 0), NE_Q_HI);
    fired = s == 0 ? NE_STEP_ZERO : s < NE_STEP_FLOOR ? NE_STEP_SHORT : 0u;
    f32x4 x;
    x[3] = (float)s / 128.0f - 1.0f;
    if (vel < 0) {
        fired |= NE_REST;
        x[0] = x[1] = x[2] = -1.0f;
        return x;
    }
    const int p = min(max(pitch, NS_PITCH_LO), NS_PITCH_HI), v = min(max(vel, NE_VEL_LO), NE_VEL_HI);
    const int d = min(max(dur_q, NE_DUR_LO), NE_Q_HI);
    fired |= (pitch < p ? NE_PITCH_UP : 0u) | (pitch > p ? NE_PITCH_DOWN : 0u) | (vel < v ? NE_VEL_UP : 0u) |
             (dur_q < d ? NE_DUR_UP : 0u) | (dur_q > d ? NE_DUR_DOWN : 0u);
    const float thr = -0.2f;
    x[0] = ((float)p + 0.5f) / 63.5f - 1.0f;
    const float q = (((float)v + 0.5f) - 60.0f) / 67.0f;
    const float qs = q * 1.2f;
    x[1] = v == NE_VEL_HI ? 1.0f : qs + thr;
    x[2] = (float)d / 128.0f - 1.0f;
    return x;
}
