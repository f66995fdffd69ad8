// Alignment of a recording to its phonemes by dynamic time warping (align.hip; include/cmtts_hip.h: cmtts_align_*; the
// definition in executable form: cmtts_amd/align.py): the cost matrix of two log-mels, the DP with its walk back, durations per phoneme.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int AL_CH = 80;                     // mel channels
constexpr int AL_MAX_SIDE = 4096;             // frames per side
constexpr int AL_MAX_B = 65535;
constexpr int AL_MAX_L = 65536;               // phonemes per row
constexpr int AL_STRIP = 64;                  // rows of the DP one wave carries: one per lane
constexpr int AL_SS = 16;                     // anti-diagonal steps between two workgroup barriers (a multiple of 8)
constexpr int AL_LAG = 2 + 62 / AL_SS;        // a strip starts this many barrier intervals behind the strip above it: the column an interval ends
                                              // with leaves the upper strip's lane 63 at step (column + 63), one whole interval earlier
constexpr int AL_RING = 256;                  // columns of a strip's last row kept for the strip below: >= (AL_LAG + 1) * AL_SS - 63
constexpr int AL_MAX_WAVES = 16;

// dwords per lane a strip's step codes take: one byte per anti-diagonal step t = j + lane, steps 0 .. (intervals * AL_SS) - 1, and the eight
// steps the DP's cost loads run ahead
inline int align_nt4(int Tr) { return (Tr + 63 + AL_SS - 1) / AL_SS * (AL_SS / 4) + 2; }
inline int align_strips(int Ts) { return (Ts + AL_STRIP - 1) / AL_STRIP; }

struct AlignWs {                              // carved from the caller's workspace, the same for the three entry points
    int32_t* lens;                            // [2][B]: x_len, y_len
    double* means;                            // [B][2][80]
    uint32_t* steps;                          // [B][strips(Ts)][nt4(Tr)][64]
    float* skew;                              // [B][strips(Ts)][4 nt4(Tr)][64]: the cost in the DP's order, [step][lane] = c[64 strip + lane][step - lane]
    size_t bytes;
};
AlignWs align_carve(void* ws, int B, int Ts, int Tr);

#ifdef __cplusplus
extern "C" {
#endif
// x [B][Ts][80], y [B][Tr][80], lens int32 [2][B] (device) -> cost [B][Ts][Tr]; cells at or beyond a pair's lengths are neither read nor written.
// means: [B][2][80] scratch (written when normalise != 0, else not touched).  Two launches (one without normalise).
int cmtts_launch_align_cost(const float* x, const float* y, const int32_t* lens, int B, int Ts, int Tr, int normalise, double* means, float* cost,
                            void* stream);
// cost [B][Ts][Tr], lens -> row int32 [B][Tr] (entries < y_len), total [B], path_len [B]; steps, skew: scratch.  Two launches: the cost into the
// DP's order (fully parallel), then the DP and the walk back, one workgroup per pair.
int cmtts_launch_align_dtw(const float* cost, const int32_t* lens, int B, int Ts, int Tr, uint32_t* steps, float* skew, int32_t* row, float* total,
                           int32_t* path_len, void* stream);
// row, cost, d_syn int32 [B][L] (negative counts as 0) -> d_rec int32 [B][L], phoneme_cost [B][L].  One launch.
int cmtts_launch_align_durations(const int32_t* row, const float* cost, const int32_t* d_syn, const int32_t* lens, int B, int Ts, int Tr, int L,
                                 int32_t* d_rec, float* phoneme_cost, void* stream);
#ifdef __cplusplus
}
#endif
