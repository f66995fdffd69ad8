// Masked consistency sampling on frame windows (retake.hip; include/cmtts_hip.h: cmtts_retake; the definition in
// numpy: cmtts_amd/retake.py).
#pragma once
#include <stdint.h>

#include "stream_windows.h"

// What the sampler's one kernel between evaluations does (retake_step_kernel):
enum RetakeMode {
    RETAKE_INIT = 0,      // x[n][t][m] = sigma_max * z(draw 0): x_T of the window rows, with a start frame per row
    RETAKE_MID = 1,       // x[n][t][m] = (regen ? x0 : known) + (z * nstd) * 0.85f on every frame of the window
    RETAKE_LAST = 2,      // out[b][start + t][m] = x0 (+ (z * nstd) * 0.85f when nstd >= 0) where regen; nothing else is written
};

struct RetakeStepArgs {
    const float* x0;            // [N][Tw][M]: the evaluation's output (MID, LAST)
    const float* known;         // [N][Tw][M]: the gathered known frames (MID)
    const uint8_t* regen;       // [N][Tw]: non-zero = regenerate (MID, LAST; the gather already cut it to the window's core)
    const int64_t* seeds;       // [N]: the seed of each row's utterance
    const StreamWindow* win;    // device [N]: z is drawn at frame win[n].start + t; LAST writes utterance win[n].b
    float* out;                 // INIT, MID: [N][Tw][M]; LAST: the mel [B][T][M]
    int N, Tw, M, T;            // T: frames per utterance of `out` (LAST)
    int draw;                   // 0 (INIT), 1 + i after evaluation i
    float scale;                // INIT: sigma_max; MID, LAST: nstd (LAST: negative = no re-noise term)
    int mode;
};

#ifdef __cplusplus
extern "C" {
#endif
// known_w[n] = mel[win[n].b][start .. start + Tw), regen_w[n][t] = regen[b][start + t] inside the window's core and 0 outside,
// spk_w[n] = spk[b] (spk may be NULL), seeds_w[n] = seeds[b]: one launch.  win: device [N], NOT validated here.  0, or -3.
int cmtts_launch_retake_gather(const float* mel, const uint8_t* regen, const float* spk, const int64_t* seeds, const StreamWindow* win, int N, int T,
                               int Tw, int M, int H, float* known_w, uint8_t* regen_w, float* spk_w, int64_t* seeds_w, void* stream);
// 0, -2 (N > 65535 or Tw * ceil(M / 4) >= 2^31) or -3 (launch error).  Arguments are NOT validated here.
int cmtts_launch_retake_step(const RetakeStepArgs* a, void* stream);
#ifdef __cplusplus
}
#endif
