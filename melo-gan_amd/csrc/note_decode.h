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
