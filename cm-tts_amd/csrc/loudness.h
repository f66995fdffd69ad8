// Integrated loudness (ITU-R BS.1770) and the output gain on the device (loudness.hip, loudness_coef.cpp; include/cmtts_hip.h:
// cmtts_loudness_measure; the definition in executable form: cmtts_amd/loudness.py).
#pragma once
#include <stdint.h>

constexpr int LD_THREADS = 256;               // lanes of a chunk workgroup: each filters one run of consecutive samples
constexpr int LD_SCAN_STEPS = 8;              // log2(LD_THREADS): P^(2^j), j = 0 .. 7
constexpr int LD_MIN_RATE = 8000, LD_MAX_RATE = 48000;
constexpr int LD_FINISH_THREADS = 64;

// What the chunk kernel needs of a sample rate, passed by value in its arguments.  The filter state is the 4-vector
// s = (z1, z2 of the shelf, z1, z2 of the high-pass), each biquad in transposed direct form II; with zero input one sample maps s to A s.
struct LoudnessPlan {
    int32_t fs, chunk, run;                   // chunk = fs / 10 (0.1 s); run = samples per lane: ceil(3 chunk / LD_THREADS), made odd
    float b[5], c[5];                         // b0 b1 b2 a1 a2 of the shelf and of the high-pass
    float P[LD_SCAN_STEPS][16];               // P[j] = A^(run 2^j), row-major
};

// Host only (loudness_coef.cpp, plain C++): the K-weighting biquads of `fs` by the bilinear transform, in double.
// out10 = b0 b1 b2 a1 a2 of the shelf, then of the high-pass.  -1 unless fs % 10 == 0 and LD_MIN_RATE <= fs <= LD_MAX_RATE.
int loudness_coefficients(int fs, double* out10);
// The plan of `fs`: coefficients rounded once to float, the state matrix powers formed in double and rounded once.  -1 as above.
int loudness_plan(int fs, LoudnessPlan* plan);

#ifdef __cplusplus
extern "C" {
#endif
// wav [rows][ld] fp32, n_valid [rows] (clamped to [0, ld]) -> sums / peaks [rows][n_chunks], n_chunks = ceil(ld / chunk): the sum of
// squares of the K-weighted samples and max |x| over [c chunk, min((c + 1) chunk, n_valid)); 0 for a chunk at or beyond n_valid.
int cmtts_launch_loudness_chunks(const float* wav, long ld, int rows, const int32_t* n_valid, const LoudnessPlan* plan, float* sums,
                                 float* peaks, int n_chunks, void* stream);
// sums / peaks -> stats [rows][4] = (L, sample peak, gain, gated blocks).  target may be NULL (gain 1); ceiling is LINEAR.
int cmtts_launch_loudness_finish(const float* sums, const float* peaks, int n_chunks, long ld, int rows, const int32_t* n_valid, int chunk,
                                 const float* target, float ceiling, float* stats, void* stream);
#ifdef __cplusplus
}
#endif
