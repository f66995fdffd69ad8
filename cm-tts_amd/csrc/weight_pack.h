// Host-only weight packers: k-major conv weights [taps][K][M] (P[tap][input channel k][output row]) -> the MFMA A-fragment streams the
// kernels read, each in its kernel's iteration order.  Plain C++17: no HIP header, no device code (import.hip uploads the results;
// internal_hooks.h: cmtts_internal_pack_weights exposes every packer to the CPU tests).  Each layout is specified at its definition in
// weight_pack.cpp.
#pragma once
#include <vector>

constexpr int WINO_PAD_HG = 4;        // to_wino_fragments: half-groups of zero padding behind a layer's array: the kernel's weight ring runs a few stages past the end
constexpr int WINO43_PAD_KS = 4;      // to_wino43_fragments: k-steps of zero padding behind a layer's array (the weight ring runs a few stages past the end)

unsigned short host_cvt16(float f, int mode);   // mode 1 = bf16 (round to nearest even), 2 = fp16

// fp32, v_mfma_f32_32x32x2_f32 (K % 8 == 0 / K % 16 == 0 for the iteration orders, M % 32 == 0)
std::vector<float> to_fragment_order(const std::vector<float>& p, int taps, int K, int M);
std::vector<float> to_fragment_iter_order(const std::vector<float>& p, int taps, int K, int M);
std::vector<float> to_wino_fragments(const std::vector<float>& p, int K, int M);
std::vector<float> to_wino_iter_fragments(const std::vector<float>& p, int taps, int K, int M);         // {} unless taps = 3 / 7 / 11
// fp32, v_mfma_f32_16x16x4_f32 (K % 4 == 0; M % 64 == 0, the xres forms M % 32 == 0)
std::vector<float> to_wino43_fragments(const std::vector<float>& p, int K, int M);
std::vector<float> to_wino43_iter_fragments(const std::vector<float>& p, int taps, int K, int M);       // {} unless taps = 3 / 5 / 7 / 11
std::vector<float> to_wino43_xres_fragments(const std::vector<float>& p, int taps, int K, int M);       // {} unless taps = 9
std::vector<float> to_wino23_xres_fragments(const std::vector<float>& p, int taps, int K, int M);       // {} unless taps = 9
// 16-bit, v_mfma_f32_32x32x16_{bf16,f16} (K % 16 == 0 / K % 32 == 0 for the iteration order, M % 32 == 0)
std::vector<unsigned short> to_fragment16(const std::vector<float>& p, int taps, int K, int M, int mode);
std::vector<unsigned short> to_fragment16_iter(const std::vector<float>& p, int taps, int K, int M, int mode);
std::vector<unsigned short> to_fragment16_split(const std::vector<float>& p, int taps, int K, int M);
// fp32, v_mfma_f32_16x16x4_f32, the speaker encoder's NHWC Conv2D (speaker_encoder.hip): p = a Keras kernel (kh, kw, cin, cout) = k-major [taps][K][M];
// taps * K is padded with zeros to a multiple of 16, M % 16 == 0.  scale: one factor per output row applied in double before the rounding, or null.
std::vector<float> to_conv2d_fragments(const std::vector<float>& p, int taps, int K, int M, const double* scale);
// The same with the layer's BatchNorm (inference form, epsilon 1e-3) folded in, in double: bn = [4][M] gamma, beta, moving mean, moving variance, or null (no BatchNorm).
// bias_out [M] = (bias - mean) * s + beta, s = gamma / sqrt(variance + 1e-3).
// fp32, v_mfma_f32_16x16x4_f32, the GE2E encoder's LSTM matrices (ge2e.hip): p = [K][M = 1024] k-major, gate rows in torch's order; the stream is
// [ceil(K / 16)][64 row tiles][64 lanes][4] over packed rows q (lstm_packed_row(q) = the torch row q holds): row tiles 4 g .. 4 g + 3 = i, f, g, o of units 16 g .. 16 g + 15
int lstm_packed_row(int q);
std::vector<float> to_lstm_fragments(const std::vector<float>& p, int K, int M);                        // {} unless M == 1024
std::vector<float> pack_conv2d_bn(const std::vector<float>& p, int taps, int K, int M, const float* bias, const float* bn, std::vector<float>* bias_out);
