// Windowed HiFi-GAN vocoding (stream_windows.hip): the mel windows of one streaming round gathered into a batch, and the
// generator's last layer evaluated on the core columns of every window only (include/cmtts_hip.h: cmtts_vocoder_forward_windows).
#pragma once
#include <stdint.h>

// One window of a round: utterance b of the padded mel, window frames [start, start + Tw), core frames
// [start + core_off, start + core_off + core_len) of it.  Host and device share this layout ([N][4] int32).
struct StreamWindow {
    int32_t b, start, core_off, core_len;
};

#ifdef __cplusplus
extern "C" {
#endif
// mel_ct [B][M][T] -> out [N][M][Tw]: out[n][c][t] = mel_ct[win[n].b][c][win[n].start + t].  win: device [N].
int cmtts_launch_mel_window_gather(const float* mel_ct, int M, int T, const StreamWindow* win, int N, int Tw, float* out, void* stream);
// x [N][C][ld] (the generator's last MRF sum, Ti = Tw * hop valid columns per row) -> pcm [N][core * hop]:
// pcm[n][j] = int16(int(tanh(conv_post(leaky_relu(x / pre_div, slope)))[core_off * hop + j] * max_wav)) for j < core_len * hop,
// 0 after that.  The same tap / channel order as conv_post_kernel and the same cast as wav_to_int16_kernel (kernels.hip).
int cmtts_launch_conv_post_windows(const float* x, const float* w, const float* bias, float pre_div, float slope, const StreamWindow* win,
                                   int N, int C, int Ti, int ld, int KW, int hop, int core, float max_wav, int16_t* pcm, void* stream);
// The same last layer as fp32 with margins: wav [N][(core + 2 margin) * hop], row n = tanh(conv_post(.)) on the window-local frames
// [max(core_off - margin, 0), min(core_off + core_len + margin, Tw)), then zeros.  Bitwise the values the int16 kernel casts.
int cmtts_launch_conv_post_windows_f32(const float* x, const float* w, const float* bias, float pre_div, float slope, const StreamWindow* win,
                                       int N, int C, int Ti, int ld, int KW, int hop, int core, int margin, float* wav, void* stream);
#ifdef __cplusplus
}
#endif
