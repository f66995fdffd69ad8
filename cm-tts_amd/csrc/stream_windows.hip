// Windowed HiFi-GAN vocoding (include/cmtts_hip.h: cmtts_vocoder_forward_windows; DESIGN.md §3 "Streaming").
//
// The generator is purely convolutional: an output frame depends on mel frames [f - H, f + H] only (H = 13 for V1).  A streaming
// round gathers one mel window per live utterance into a batch [N][80][Tw] (mel_window_gather_kernel), runs the unchanged
// generator on it, and evaluates the last layer — leaky_relu -> conv_post -> tanh -> int16, the 256x-rate tail — on the CORE
// columns of every window only, straight into the round's int16 chunks (conv_post_windows_kernel).  Both kernels trust the
// window table: cmtts_vocoder_forward_windows validates a host copy of it before anything is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stream_windows.h"

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// 4 channel rows per 256-lane workgroup, 64 lanes per row; 16-byte loads and stores when the source and destination rows of
// this window are 16-byte aligned (T, Tw and the window start multiples of 4), then a scalar tail; dword copies otherwise.
__global__ __launch_bounds__(256) void mel_window_gather_kernel(const float* __restrict__ mel, int M, int T, const StreamWindow* __restrict__ win,
                                                                int Tw, float* __restrict__ out) {
    const int n = blockIdx.y;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= M) return;
    const StreamWindow wd = win[n];
    const float* src = mel + ((long)wd.b * M + c) * T + wd.start;
    float* dst = out + ((long)n * M + c) * Tw;
    int t = lane;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const int n4 = Tw >> 2;
        for (int q = lane; q < n4; q += 64) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
        t = (n4 << 2) + lane;
    }
    for (; t < Tw; t += 64) dst[t] = src[t];
}

// conv_post_kernel / conv_post_v4_kernel (kernels.hip) on window-local sample columns: a thread owns PV consecutive samples of
// one window's chunk; every sample accumulates over (channel, tap) in ascending order with fmaf, then tanhf(acc + bias), then
// wav_to_int16_kernel's cast (truncation toward zero through int32, +1.0 wraps to -32768) — the same operations on the same
// values, so the same bits.  V4: the input quads come in 16-byte loads (rows 16-byte aligned, ld >= Ti rounded up to 4,
// t0 a multiple of 4), exactly as conv_post_v4_kernel fetches them; values outside [0, Ti) are masked to 0 either way.
constexpr int PV = 4;
constexpr int PKW_MAX = 7;
template <bool V4>
__global__ __launch_bounds__(256) void conv_post_windows_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float pre_div, float slope,
                                                                const StreamWindow* __restrict__ win, int C, int Ti, int ld, int KW,
                                                                int hop, int core, float max_wav, int16_t* __restrict__ pcm) {
    extern __shared__ float wsh[];
    for (int i = threadIdx.x; i < C * KW; i += 256) wsh[i] = w[i];
    __syncthreads();
    const int n = blockIdx.y;
    const long row = (long)core * hop;
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * PV;
    if (j0 >= row) return;
    int16_t* out = pcm + n * row;
    const StreamWindow wd = win[n];
    const long jn = (long)wd.core_len * hop;          // samples of this window's core; the rest of the chunk row is zero
    if (j0 >= jn) {
#pragma unroll
        for (int v = 0; v < PV; ++v)
            if (j0 + v < row) out[j0 + v] = 0;
        return;
    }
    const int t0 = wd.core_off * hop + (int)j0;        // window-local sample of the first output
    const int pad = KW / 2;
    float acc[PV];
#pragma unroll
    for (int v = 0; v < PV; ++v) acc[v] = 0.f;
    const float* xb = x + (long)n * C * ld;
    if constexpr (V4) {
        const int tl = max(t0 - 4, 0), tr = min(t0 + 4, ((Ti + 3) & ~3) - 4);
        constexpr int CU = 4;
        for (int c0 = 0; c0 < C; c0 += CU) {
            float4 Lq[CU], Mq[CU], Rq[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const float* xr = xb + (long)min(c0 + u, C - 1) * ld;
                Lq[u] = *reinterpret_cast<const float4*>(xr + tl);
                Mq[u] = *reinterpret_cast<const float4*>(xr + t0);
                Rq[u] = *reinterpret_cast<const float4*>(xr + tr);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                if (c0 + u >= C) break;
                const float raw[12] = {Lq[u].x, Lq[u].y, Lq[u].z, Lq[u].w, Mq[u].x, Mq[u].y, Mq[u].z, Mq[u].w, Rq[u].x, Rq[u].y, Rq[u].z, Rq[u].w};
                float xv[PV + PKW_MAX - 1];
#pragma unroll
                for (int q = 0; q < PV + PKW_MAX - 1; ++q) {
                    const int tt = t0 + q - pad;
                    const int ri = q - pad + 4;
                    float v = (q < PV + KW - 1 && tt >= 0 && tt < Ti && ri >= 0 && ri < 12) ? raw[ri < 0 ? 0 : (ri > 11 ? 11 : ri)] : 0.f;
                    if (pre_div != 1.0f) v = v / pre_div;
                    xv[q] = v > 0.f ? v : v * slope;
                }
#pragma unroll
                for (int k = 0; k < PKW_MAX; ++k) {
                    if (k < KW) {
                        const float wk = wsh[(c0 + u) * KW + k];
#pragma unroll
                        for (int v = 0; v < PV; ++v) acc[v] = fmaf(wk, xv[v + k], acc[v]);
                    }
                }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float* xr = xb + (long)c * ld;
            float xv[PV + PKW_MAX - 1];
#pragma unroll
            for (int q = 0; q < PV + PKW_MAX - 1; ++q) {
                const int tt = t0 + q - pad;
                float v = (q < PV + KW - 1 && tt >= 0 && tt < Ti) ? xr[tt] : 0.f;
                if (pre_div != 1.0f) v = v / pre_div;
                xv[q] = v > 0.f ? v : v * slope;
            }
#pragma unroll
            for (int k = 0; k < PKW_MAX; ++k) {
                if (k < KW) {
                    const float wk = wsh[c * KW + k];
#pragma unroll
                    for (int v = 0; v < PV; ++v) acc[v] = fmaf(wk, xv[v + k], acc[v]);
                }
            }
        }
    }
    const float bs = bias[0];
#pragma unroll
    for (int v = 0; v < PV; ++v) {
        if (j0 + v < jn) {
            const float y = tanhf(acc[v] + bs);
            out[j0 + v] = (int16_t)(int)(y * max_wav);
        } else if (j0 + v < row) {
            out[j0 + v] = 0;
        }
    }
}

// conv_post_windows_kernel with a float, margin-carrying output (cmtts_vocoder_forward_windows_f32: the input of the resampler,
// which needs the samples up to one filter half-width beyond the core): the same accumulation — channel / tap order, fmaf, tanhf,
// the same loads — written as fp32 for the window-local frames [core_off - margin, core_off + core_len + margin) clipped to the
// window, row pitch (core + 2 margin) * hop, zeros after.  Kept apart from the int16 kernel, which stays as it is.
template <bool V4>
__global__ __launch_bounds__(256) void conv_post_windows_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float pre_div, float slope,
                                                                const StreamWindow* __restrict__ win, int C, int Ti, int ld, int KW,
                                                                int hop, int core, int margin, float* __restrict__ wav) {
    extern __shared__ float wsh[];
    for (int i = threadIdx.x; i < C * KW; i += 256) wsh[i] = w[i];
    __syncthreads();
    const int n = blockIdx.y;
    const long row = (long)(core + 2 * margin) * hop;
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * PV;
    if (j0 >= row) return;
    float* out = wav + n * row;
    const StreamWindow wd = win[n];
    const int Tw = Ti / hop;
    const int f_lo = max(wd.core_off - margin, 0), f_hi = min(wd.core_off + wd.core_len + margin, Tw);
    const long jn = (long)(f_hi - f_lo) * hop;        // samples of this window's core and margins; the rest of the row is zero
    if (j0 >= jn) {
#pragma unroll
        for (int v = 0; v < PV; ++v)
            if (j0 + v < row) out[j0 + v] = 0.f;
        return;
    }
    const int t0 = f_lo * hop + (int)j0;               // window-local sample of the first output
    const int pad = KW / 2;
    float acc[PV];
#pragma unroll
    for (int v = 0; v < PV; ++v) acc[v] = 0.f;
    const float* xb = x + (long)n * C * ld;
    if constexpr (V4) {
        const int tl = max(t0 - 4, 0), tr = min(t0 + 4, ((Ti + 3) & ~3) - 4);
        constexpr int CU = 4;
        for (int c0 = 0; c0 < C; c0 += CU) {
            float4 Lq[CU], Mq[CU], Rq[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const float* xr = xb + (long)min(c0 + u, C - 1) * ld;
                Lq[u] = *reinterpret_cast<const float4*>(xr + tl);
                Mq[u] = *reinterpret_cast<const float4*>(xr + t0);
                Rq[u] = *reinterpret_cast<const float4*>(xr + tr);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                if (c0 + u >= C) break;
                const float raw[12] = {Lq[u].x, Lq[u].y, Lq[u].z, Lq[u].w, Mq[u].x, Mq[u].y, Mq[u].z, Mq[u].w, Rq[u].x, Rq[u].y, Rq[u].z, Rq[u].w};
                float xv[PV + PKW_MAX - 1];
#pragma unroll
                for (int q = 0; q < PV + PKW_MAX - 1; ++q) {
                    const int tt = t0 + q - pad;
                    const int ri = q - pad + 4;
                    float v = (q < PV + KW - 1 && tt >= 0 && tt < Ti && ri >= 0 && ri < 12) ? raw[ri < 0 ? 0 : (ri > 11 ? 11 : ri)] : 0.f;
                    if (pre_div != 1.0f) v = v / pre_div;
                    xv[q] = v > 0.f ? v : v * slope;
                }
#pragma unroll
                for (int k = 0; k < PKW_MAX; ++k) {
                    if (k < KW) {
                        const float wk = wsh[(c0 + u) * KW + k];
#pragma unroll
                        for (int v = 0; v < PV; ++v) acc[v] = fmaf(wk, xv[v + k], acc[v]);
                    }
                }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float* xr = xb + (long)c * ld;
            float xv[PV + PKW_MAX - 1];
#pragma unroll
            for (int q = 0; q < PV + PKW_MAX - 1; ++q) {
                const int tt = t0 + q - pad;
                float v = (q < PV + KW - 1 && tt >= 0 && tt < Ti) ? xr[tt] : 0.f;
                if (pre_div != 1.0f) v = v / pre_div;
                xv[q] = v > 0.f ? v : v * slope;
            }
#pragma unroll
            for (int k = 0; k < PKW_MAX; ++k) {
                if (k < KW) {
                    const float wk = wsh[c * KW + k];
#pragma unroll
                    for (int v = 0; v < PV; ++v) acc[v] = fmaf(wk, xv[v + k], acc[v]);
                }
            }
        }
    }
    const float bs = bias[0];
#pragma unroll
    for (int v = 0; v < PV; ++v) {
        if (j0 + v < jn) {
            out[j0 + v] = tanhf(acc[v] + bs);
        } else if (j0 + v < row) {
            out[j0 + v] = 0.f;
        }
    }
}

}  // namespace

extern "C" int cmtts_launch_mel_window_gather(const float* mel_ct, int M, int T, const StreamWindow* win, int N, int Tw, float* out, void* stream) {
    if (N <= 0 || M <= 0 || Tw <= 0) return 0;
    hipLaunchKernelGGL(mel_window_gather_kernel, dim3(cdiv(M, 4), N), dim3(256), 0, (hipStream_t)stream, mel_ct, M, T, win, Tw, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_conv_post_windows(const float* x, const float* w, const float* bias, float pre_div, float slope, const StreamWindow* win,
                                              int N, int C, int Ti, int ld, int KW, int hop, int core, float max_wav, int16_t* pcm, void* stream) {
    if (KW > PKW_MAX || KW / 2 > 4) return -2;
    if (N <= 0 || core <= 0) return 0;
    const dim3 grid(cdiv((long)core * hop, 256 * PV), N);
    const size_t lds = (size_t)C * KW * sizeof(float);
    // every window-local start core_off * hop + 4 i is a multiple of 4 when hop is
    const bool v4 = (hop & 3) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld >= ((Ti + 3) & ~3) && Ti >= 4;
    if (v4)
        hipLaunchKernelGGL(conv_post_windows_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, pre_div, slope, win, C, Ti, ld,
                           KW, hop, core, max_wav, pcm);
    else
        hipLaunchKernelGGL(conv_post_windows_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, pre_div, slope, win, C, Ti, ld,
                           KW, hop, core, max_wav, pcm);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_conv_post_windows_f32(const float* x, const float* w, const float* bias, float pre_div, float slope, const StreamWindow* win,
                                                  int N, int C, int Ti, int ld, int KW, int hop, int core, int margin, float* wav, void* stream) {
    if (KW > PKW_MAX || KW / 2 > 4) return -2;
    if (N <= 0 || core <= 0 || margin < 0) return 0;
    const dim3 grid(cdiv((long)(core + 2 * margin) * hop, 256 * PV), N);
    const size_t lds = (size_t)C * KW * sizeof(float);
    // every window-local start f_lo * hop + 4 i is a multiple of 4 when hop is
    const bool v4 = (hop & 3) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld >= ((Ti + 3) & ~3) && Ti >= 4;
    if (v4)
        hipLaunchKernelGGL(conv_post_windows_f32_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, pre_div, slope, win, C, Ti,
                           ld, KW, hop, core, margin, wav);
    else
        hipLaunchKernelGGL(conv_post_windows_f32_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, pre_div, slope, win, C, Ti,
                           ld, KW, hop, core, margin, wav);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
