// Recorded speech in (mel_analysis.hip, mel_basis.cpp; include/cmtts_hip.h: cmtts_analysis_*, cmtts_mel_analysis, cmtts_phoneme_energy,
// cmtts_pcm_crossfade; the definition in executable form: cmtts_amd/analysis.py): the log-mel / energy analysis of a
// waveform in one launch, phoneme-level energy targets, and the crossfade that joins vocoded window rows into a recording.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int MEL_NFFT = 1024;                // filter_length == win_length: the one STFT instance every reference config uses
constexpr int MEL_HOP = 256;
constexpr int MEL_BINS = MEL_NFFT / 2 + 1;
constexpr int MEL_CH = 80;
constexpr int MEL_MIN_RATE = 8000, MEL_MAX_RATE = 48000;
constexpr int MEL_FPB = 4;                    // consecutive frames per workgroup: one per wave
constexpr int MEL_NNZ_MAX = 2 * MEL_BINS;     // a bin lies between two neighbouring corners, so it feeds at most two triangles

// mel_basis.cpp (host only).  out [n_mels][n_fft / 2 + 1]: the Slaney filterbank, computed in double, stored as float.  -1 for arguments
// outside 2 <= n_fft <= 65536 (even or odd: n_fft / 2 + 1 bins on linspace(0, fs / 2, bins); cmtts_mel_basis admits even ones only), 1 <= n_mels <= 1024, 0 <= fmin < fmax <= fs / 2, fs >= 1.
int mel_basis(int fs, int n_fft, int n_mels, double fmin, double fmax, float* out);
// The periodic Hann window [1024] and the twiddles exp(-2 pi i k / 1024), k = 0 .. 511, as (cos, sin) pairs [512][2]: made in double,
// rounded to float once.
void mel_window(float* out);
void mel_twiddles(float* out);
// The basis [80][513] as sparse rows: filter m weighs bins [lo, lo + cnt) with pack[off .. off + cnt), tab[m] = (off, lo, cnt); returns the
// number of packed weights (<= MEL_NNZ_MAX), or -1 when a row's non-zero bins are not one run.
int mel_sparse_rows(const float* basis, float* pack, int32_t* tab);

#ifdef __cplusplus
extern "C" {
#endif
struct MelTables {                            // device pointers a cmtts_analysis handle owns
    const float* window;                      // [1024]
    const float* twiddle;                     // [512][2]
    const float* pack;                        // [nnz]
    const int32_t* tab;                       // [80][3]
    int nnz;
};
// wav float or int16 [rows][ld], n_valid [rows] (clamped to [0, ld]); pad: the reflected samples on either side (512: centred frames, 1 + n / 256
// of them; 384: frame f covers samples [256 f, 256 f + 256), n / 256 of them); a row with n <= pad has no frames.  mel [rows][T][80] (layout 0)
// or [rows][80][T] (1), energy [rows][T], frames [rows] = min(the row's frames, T); zeros at and beyond a row's frames.
int cmtts_launch_mel_analysis(const MelTables* t, const void* wav, int is_int16, long ld, int rows, const int32_t* n_valid, int pad, int T, int layout,
                              float* mel, float* energy, int32_t* frames, void* stream);
// energy [B][T], durations int32 [B][L] (negative counts as 0) -> out [B][L] = (mean of the phoneme's frames (0 for none) - mean) / std
int cmtts_launch_phoneme_energy(const float* energy, int B, int T, const int32_t* durations, int L, double mean, double std, float* out, void* stream);
// wav_rows fp32 [N][row], rec_rows int16 [N][row], row = (core + 2 X) * hop; table int32 [N][4] = (lead frames in the row, core frames, trail
// frames, fades: bit 0 lead, bit 1 trail) -> out_rows int16 [N][row]
int cmtts_launch_pcm_crossfade(const float* wav_rows, const int16_t* rec_rows, const int32_t* table, int N, int core, int X, int hop,
                               int16_t* out_rows, void* stream);
#ifdef __cplusplus
}
#endif
