// Pitch of a recording (pitch.hip, pitch_tables.cpp; include/cmtts_hip.h: cmtts_pitch_*; the definition in executable form:
// cmtts_amd/pitch.py): the normalised autocorrelation of every frame, the tracker's candidates and Viterbi path, and the CWT pitch targets.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int PT_NC = 8;                      // candidates kept per frame
constexpr int PT_STATES = PT_NC + 1;          // state 0 is "unvoiced"
constexpr int PT_MAX_W = 2048;                // samples of a frame's window
constexpr int PT_MAX_LAGS = 512;              // columns of r: lags 0 .. LMAX + 1
constexpr int PT_MAX_HOP = 1024;
constexpr int PT_MAX_T = 4096;                // frames per row
constexpr int PT_MAX_B = 65535;
constexpr int PT_FPB = 4;                     // consecutive frames per workgroup of the autocorrelation: one per wave
constexpr int PT_CWT_SCALES = 10;
constexpr int PT_CWT_MIN_N = 4, PT_CWT_MAX_N = 4096;
constexpr int PT_CWT_LD = 2 * PT_CWT_MAX_N - PT_CWT_MIN_N;      // 4 + 8 + .. + 4096: the table of transform length N starts at column N - 4

struct PitchGeometry {
    int fs, hop;
    int W;                                    // window: 3 periods of the floor, rounded up to even
    int lmin, lmax;                           // ceil(fs / ceiling), floor(fs / floor)
};

// pitch_tables.cpp (host only; everything in double, rounded once).  -1 for fs < 1, hop outside [1, 1024], not 0 < floor < ceiling <= fs / 2,
// W > 2048 or LMAX + 2 > 512.
int pitch_geometry(int fs, int hop, double floor_hz, double ceiling_hz, PitchGeometry* g);
// window [W]: 0.5 - 0.5 cos(2 pi (i + 0.5) / W); rw [lmax + 2]: its autocorrelation, normalised to rw[0] = 1
void pitch_window(const PitchGeometry& g, float* window, double* rw);
// lg [lmax + 2]: (float)log2(tau), lg[0] = 0; *lg_floor = (float)log2(fs / floor)
void pitch_lg(const PitchGeometry& g, double floor_hz, float* lg, float* lg_floor);
// out [10][PT_CWT_LD]: for every N = 4 .. 4096 the periodised DOG-2 wavelet h_j[m], m < N, at columns [N - 4, 2 N - 4): the inverse DFT of
// sqrt(2 pi s_j / dt) psi^(s_j w_k), s_j = 0.01 2^j, dt = 0.005
void pitch_cwt_tables(float* out);

struct PitchTables {                          // device pointers a cmtts_pitch handle owns
    const float* window;                      // [W]
    const double* rw;                         // [lmax + 2]
    const float* lg;                          // [lmax + 2]
    const float* cwt;                         // [10][PT_CWT_LD]
    float lg_floor;
    PitchGeometry g;
};

#ifdef __cplusplus
extern "C" {
#endif
// wav float or int16 [rows][ld], n_valid [rows] (clamped to [0, ld]) -> r [rows][T][lmax + 2], pk [rows][T], frames [rows] = min(1 + n / hop, T);
// zeros at and beyond a row's frames.  One launch.
int cmtts_launch_pitch_nacf(const PitchTables* t, const void* wav, int is_int16, long ld, int rows, const int32_t* n_valid, int T, float* r, float* pk,
                            int32_t* frames, void* stream);
// r, pk, frames -> lag int32 [B][T], f0 [B][T]; cand_lag int32 [B][T][8], cand_str, cand_lg [B][T][8]: scratch.  Two launches.
int cmtts_launch_pitch_track(const PitchTables* t, const float* r, const float* pk, const int32_t* frames, int B, int T, int32_t* cand_lag,
                             float* cand_str, float* cand_lg, int32_t* lag, float* f0, void* stream);
// f0, frames -> cwt_spec [B][T][10], f0_mean [B], f0_std [B], uv uint8 [B][T], status int32 [B].  One launch.
int cmtts_launch_pitch_targets(const PitchTables* t, const float* f0, const int32_t* frames, int B, int T, float* cwt_spec, float* f0_mean,
                               float* f0_std, uint8_t* uv, int32_t* status, void* stream);
#ifdef __cplusplus
}
#endif
