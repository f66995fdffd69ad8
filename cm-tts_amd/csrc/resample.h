// Polyphase resampling + output encoding of fp32 waveform rows (resample.hip; include/cmtts_hip.h: cmtts_resample_encode;
// DESIGN.md §3.5e; the definition in executable form: cmtts_amd/resample.py).
#pragma once
#include <stdint.h>

// One output row: outputs m in [m0, m1) of an utterance with n_valid source samples, read from source row `row` whose element 0 is
// the utterance's absolute sample `origin`.  Host and device share this layout ([N][5] int32).
struct ResampleSegment {
    int32_t row, origin, m0, m1, n_valid;
};

constexpr int RS_ENC_F32 = 0, RS_ENC_S16 = 1, RS_ENC_MULAW = 2, RS_ENC_ALAW = 3;
constexpr int RS_TILE = 256;                  // outputs per workgroup, one per lane
constexpr int RS_MAX_TABLE = 1 << 16;         // floats of the tap table [L][2 R + 1]
constexpr int RS_MAX_SPAN = 8192;             // floats of a tile's staged source span (32 KB of LDS)

#ifdef __cplusplus
extern "C" {
#endif
// taps [2 half + 1] (device) -> table [L][2 R + 1]: table[p][d + R] = taps[p - d L + half], 0 outside the taps.
int cmtts_launch_resample_table(const float* taps, int L, int half, int R, float* table, void* stream);
// wav [rows][ld] fp32 -> out [N][out_ld] (float / int16 / uint8 by `enc`): row n holds outputs [m0, m1) of segment n, then zeros.
// y[m] = sum over d = -R .. R (ascending, fmaf) of x[floor(m M / L) + d] * table[(m M) mod L][d + R]; x is zero outside
// [0, n_valid) and outside the row's coverage [origin, origin + ld).  -2: the tile's source span exceeds RS_MAX_SPAN.
int cmtts_launch_resample_encode(const float* wav, long ld, const ResampleSegment* seg, int N, const float* table, int L, int M, int R,
                                 int enc, float max_wav, void* out, long out_ld, void* stream);
// The same with a gain per SOURCE row (gains [rows], device): x is replaced by fl32(gains[row] * x), one multiplication per source sample
// as it is staged.  gains == NULL is cmtts_launch_resample_encode: the instantiation without the multiplication.
int cmtts_launch_resample_encode_gain(const float* wav, long ld, const ResampleSegment* seg, int N, const float* table, int L, int M, int R,
                                      int enc, float max_wav, void* out, long out_ld, const float* gains, void* stream);
#ifdef __cplusplus
}
#endif
