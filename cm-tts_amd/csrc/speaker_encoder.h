// Speaker embeddings from reference audio on the device (speaker_encoder.hip; include/cmtts_hip.h: cmtts_spkenc_*; the
// definition in executable form: cmtts_amd/speaker.py): trim, fbank features in the window layout, the DeepSpeaker ResCNN as NHWC
// implicit-GEMM Conv2D launches on v_mfma_f32_16x16x4_f32, and the tail (time mean, dense, L2 norm, window mean per row).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int SPK_FBANKS = 64;                // filters = columns of a window
constexpr int SPK_FRAMES = 160;               // frames = rows of a window
constexpr int SPK_EMB = 512;
constexpr int SPK_NFFT = 1024;                // the one FFT size the fbank kernel is written for: 512 < win_length <= 1024
constexpr int SPK_HOP = 80;                   // windows = "all": hop between windows
constexpr int SPK_MAX_WINDOWS = 64;           // ... and the most windows a row can have
constexpr int SPK_MIN_RATE = 8000, SPK_MAX_RATE = 40000;      // frame_len = round(0.025 fs) must fit the FFT
constexpr int SPK_DENSE_IN = 2048;

// What the fbank kernel needs of (fs, win_length), passed by value in its arguments; made on the host in double (speaker_plan)
struct SpkPlan {
    int32_t frame_len, frame_step;
    int32_t bins[SPK_FBANKS + 2];             // corner bins of the triangular filters
};
// -1 unless SPK_MIN_RATE <= fs <= SPK_MAX_RATE and 512 < win_length <= 1024
int speaker_plan(int fs, int win_length, SpkPlan* plan);

// One Conv2D launch: NHWC activations, TensorFlow 'same' padding, BatchNorm already folded into (wf, bias).
struct SpkConvArgs {
    const float* x;       // [B][H][W][cin]
    const float* wf;      // fragment stream of weight_pack.h: to_conv2d_fragments
    const float* bias;    // [cout]
    const float* res;     // [B][Ho][Wo][cout] or null; may be y (each element is read by the lane that then writes it)
    float* y;             // [B][Ho][Wo][cout]
    int B, H, W, cin, cout, ks, stride;
};

#ifdef __cplusplus
extern "C" {
#endif
// wav [rows][ld] fp32, n_valid [rows] (clamped to [0, ld]) -> info [rows][4] int32: (first, last) of the kept span x[first:last], (-1, -1)
// where there is none; entries 2 and 3 are not written
int cmtts_launch_spk_trim(const float* wav, long ld, int rows, const int32_t* n_valid, int32_t* info, void* stream);
// info (first, last) -> info (frames, windows) and the windows [sum of the rows' windows][160][64], rows in order, each row's windows in
// offset order.  mode 0: centre window, 1: all (hop SPK_HOP, last aligned to the end, at most max_windows), 2: offsets [rows] (device; clamped
// into [0, max(frames - 160, 0)]).  twiddle: device double [512][2], exp(-2 pi i k / 1024).
int cmtts_launch_spk_fbank(const float* wav, long ld, int rows, int32_t* info, const SpkPlan* plan, int mode, const int32_t* offsets,
                           int max_windows, const double* twiddle, float* windows, void* stream);
// -2: a shape no instance covers (cin == 1 with cout == 64, or cin % 64 == 0; cout 64 / 128 / 256 / 512; ks 3 / 5; stride 1 / 2)
int cmtts_launch_spk_conv2d(const SpkConvArgs* a, void* stream);
// feat [W][10][4][512] -> emb_w [W][512] unit norm (dense [2048][512], bias [512]); then per row the normalised mean of the windows w with
// row_map[w] == row, in window order: emb [rows][512], zeros for a row without windows
int cmtts_launch_spk_tail(const float* feat, int W, const float* dense, const float* bias, float* emb_w, const int32_t* row_map, int rows,
                          float* emb, void* stream);
#ifdef __cplusplus
}
#endif
