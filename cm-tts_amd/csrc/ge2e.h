// GE2E speaker embeddings from reference audio on the device (ge2e.hip; include/cmtts_hip.h: cmtts_ge2e_*; the definition in
// executable form: cmtts_amd/ge2e.py): the 40-channel power mel at the odd transform length 551 as a DFT contraction on v_mfma_f32_16x16x4_f32,
// the three LSTM layers (one projection GEMM + one recurrence launch each) and the tail (Linear + ReLU + L2 norm, window mean per row).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int GE2E_RATE = 22050;
constexpr int GE2E_NFFT = 551, GE2E_HOP = 220, GE2E_PAD = GE2E_NFFT / 2, GE2E_BINS = GE2E_NFFT / 2 + 1;
constexpr int GE2E_MELS = 40;
constexpr int GE2E_FRAMES = 160, GE2E_WHOP = 80;      // a partial: 160 frames, one every 80
constexpr int GE2E_HID = 256, GE2E_GATES = 4 * GE2E_HID, GE2E_EMB = 256, GE2E_LAYERS = 3;
constexpr int GE2E_TILE = 16;                         // windows per recurrence workgroup (32 was measured and dropped: profiles/ge2e.md)
constexpr int GE2E_KCHUNKS = 35;                      // 551 samples in chunks of 16 (560; the table is zero behind 551)
constexpr int GE2E_PAIRS = 18;                        // 276 bins in tiles of 16 (288; the table is zero behind 276), a cos and a sin tile each
constexpr int GE2E_NNZ_MAX = 2 * GE2E_BINS;           // a bin lies between two neighbouring corners, so it feeds at most two triangles

struct Ge2eTables {                                   // device pointers a cmtts_ge2e handle owns
    const float* dft;                                 // [18 pairs][35 chunks][cos, sin][64 lanes][4]: A fragments, the periodic Hann window folded in
    const float* pack;                                // [nnz] triangle weights
    const int32_t* tab;                               // [40][3] = (offset into pack, first bin, bins)
};
// The host side of the tables: dft in double with the angle reduced as (k n mod 551), rounded once; the triangles from mel_basis() at n_fft = 551.
// Returns the number of packed weights, -1 if a row's non-zero bins are not one run.
int ge2e_host_tables(float* dft /* [18 * 35 * 2 * 64 * 4] */, float* pack /* [GE2E_NNZ_MAX] */, int32_t* tab /* [120] */);
constexpr size_t GE2E_DFT_FLOATS = (size_t)GE2E_PAIRS * GE2E_KCHUNKS * 2 * 64 * 4;

// What compute_partial_slices and the padding rule of embed_utterance give a row of n samples.  mode 1: partials; 0: the whole utterance as one window.
struct Ge2eCounts {
    int n_eff, frames, nwin;                          // the zero-padded length, its frame count 1 + (n_eff - 1) / 220, the row's windows (mode 1: at most max_windows)
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline Ge2eCounts ge2e_counts(int n, int mode, int max_windows) {
    Ge2eCounts c{0, 0, 0};
    if (n <= 0) return c;
    int cnt = 1;
    c.n_eff = n;
    if (mode == 1) {
        const int nf = (n + GE2E_HOP) / GE2E_HOP;                         // ceil((n + 1) / 220)
        const int steps = nf - GE2E_FRAMES + GE2E_WHOP + 1 > 1 ? nf - GE2E_FRAMES + GE2E_WHOP + 1 : 1;
        cnt = (steps + GE2E_WHOP - 1) / GE2E_WHOP;
        const int last = GE2E_WHOP * (cnt - 1) * GE2E_HOP;
        if (cnt > 1 && 4 * (n - last) < 3 * GE2E_FRAMES * GE2E_HOP) --cnt;  // coverage (n - start) / 35200 < 0.75
        const int stop = (GE2E_WHOP * (cnt - 1) + GE2E_FRAMES) * GE2E_HOP;
        if (stop >= n) c.n_eff = stop;
    }
    c.frames = 1 + (c.n_eff - 1) / GE2E_HOP;
    c.nwin = cnt < max_windows ? cnt : max_windows;
    return c;
}

#ifdef __cplusplus
extern "C" {
#endif
// wav [rows][ld] fp32, n_valid [rows] (clamped to [0, ld]) -> info [rows][4] = (n, padded n, frames of the padded row, windows) and the windows, rows in
// order: mode 1 [sum of windows][160][40], window j of a row = frames 80 j .. 80 j + 159; mode 0 [rows with n > 0][T][40], zero rows at and beyond the
// row's frames.  win_lens [windows] = 160 / min(frames, T).
int cmtts_launch_ge2e_mel(const float* wav, long ld, int rows, const int32_t* n_valid, int mode, int max_windows, int T, const Ge2eTables* tb,
                          float* windows, int32_t* win_lens, int32_t* info, void* stream);
// One LSTM layer on x [N][T][K] (K = 40 or 256): pre [N][T][1024] = x W_ih^T + b in packed row order (wih, whh: to_lstm_fragments streams; bias: packed rows,
// b_ih + b_hh), then the recurrence over tiles of `tile` (= GE2E_TILE) windows: hseq [N][T][256] (written up to the tile's longest window), hlast [N][256].
// lens [N] or null (every window has T frames): a window's state stays as it is from its length on.  -2: an argument no instance covers.
int cmtts_launch_ge2e_layer(const float* x, int N, int T, int K, const float* wih, const float* whh, const float* bias, const int32_t* lens, int tile,
                            float* pre, float* hseq, float* hlast, void* stream);
// hlast [W][256] -> emb_w [W][256] = relu(linear) / (norm + 1e-5) (lin_t [256 k][256 o]); then, with row_map (device int32 [W]), emb [rows][256] = the
// mean of a row's windows in window order divided by its norm, zeros for a row without windows.  row_map null: nothing more (emb unused).
int cmtts_launch_ge2e_tail(const float* hlast, int W, const float* lin_t, const float* lin_b, float* emb_w, const int32_t* row_map, int rows, float* emb,
                           void* stream);
#ifdef __cplusplus
}
#endif
