// Output sample rates and encodings (include/cmtts_hip.h: cmtts_resample_encode; definition: cmtts_amd/resample.py).
//
// A rational L / M polyphase FIR on fp32 waveform rows: y[m] = sum_j x[j] h[m M - j L + half].  With j0 = floor(m M / L) and the
// phase p = (m M) mod L the tap under x[j0 + d] is h[p - d L + half], so every output is a dot product of 2 R + 1 consecutive
// source samples with row p of a phase-major table [L][2 R + 1] (zero where p - d L + half leaves the taps).  The sum runs over
// ascending d with fmaf from acc = 0 and depends on the absolute m and the sample values only — not on the tile, the segment or
// the row the samples are read from — which is what makes a wave resampled in pieces bitwise equal to the wave resampled whole.
// The kernel trusts the segment table: cmtts_resample_encode validates a host copy of it before anything is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resample.h"

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

__global__ __launch_bounds__(256) void resample_table_kernel(const float* __restrict__ taps, int L, int half, int R, float* __restrict__ table) {
    const int W = 2 * R + 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)L * W) return;
    const int p = (int)(i / W), d = (int)(i % W) - R;
    const long idx = (long)p - (long)d * L + half;
    table[i] = (idx >= 0 && idx <= 2L * half) ? taps[idx] : 0.f;
}

// cmtts_wav_to_int16's cast (truncation toward zero), saturated instead of wrapped: a FIR overshoots +-1.0 routinely
__device__ __forceinline__ int to_s16(float y, float max_wav) {
    const float v = fminf(fmaxf(y * max_wav, -32768.f), 32767.f);
    return (int)v;
}
// ITU-T G.711 of a 16-bit sample: mu-law on the 14-bit value s >> 2 (bias 33, clip 8159), A-law on the 13-bit value s >> 3
__device__ __forceinline__ unsigned lin2ulaw(int s) {
    const int v = s >> 2;
    const bool neg = v < 0;
    const int mag = min(neg ? -v : v, 8159) + 0x21;              // >= 0x21: at least 6 significant bits
    const int seg = 32 - __clz(mag) - 6;
    const unsigned u = seg >= 8 ? 0x7Fu : (unsigned)((seg << 4) | ((mag >> (seg + 1)) & 0xF));
    return (u ^ (neg ? 0x7Fu : 0xFFu)) & 0xFFu;
}
__device__ __forceinline__ unsigned lin2alaw(int s) {
    const int v = s >> 3;
    const bool neg = v < 0;
    const int mag = neg ? -v - 1 : v;                             // 0 .. 4095
    const int seg = max(32 - __clz(mag) - 5, 0);                  // __clz(0) = 32
    const unsigned a = (unsigned)((seg << 4) | ((seg < 2 ? mag >> 1 : mag >> seg) & 0xF));
    return (a ^ (neg ? 0x55u : 0xD5u)) & 0xFFu;
}

template <int ENC>
struct OutT { using type = float; };
template <>
struct OutT<RS_ENC_S16> { using type = int16_t; };
template <>
struct OutT<RS_ENC_MULAW> { using type = uint8_t; };
template <>
struct OutT<RS_ENC_ALAW> { using type = uint8_t; };

// One workgroup = RS_TILE consecutive outputs of one segment, one per lane.  The tile's source span [j0(first) - R, j0(last) + R]
// is staged into LDS with consecutive lanes on consecutive samples (coalesced; everything outside [0, n_valid) or outside the row
// is 0).  In the accumulation lane i reads xs[j0(m_i) - R - base + d]: neighbouring lanes are floor-steps of M / L apart (2.76 at
// 8 kHz: 2- and 3-bank strides, at most 2 lanes per bank; < 1 when up-sampling: same address, broadcast).  The tap rows come from
// the global table (<= 90 KB, L2-resident; neighbouring lanes use rows M mod L apart, the odd row pitch 2 R + 1 spreads them).
// GAIN: the staging line stores gains[source row] * x (one fp32 multiplication per source sample); nothing else changes.
template <int ENC, bool GAIN>
__global__ __launch_bounds__(RS_TILE) void resample_encode_kernel(const float* __restrict__ wav, long ld, const ResampleSegment* __restrict__ seg,
                                                                  const float* __restrict__ table, int L, int M, int R, float max_wav,
                                                                  typename OutT<ENC>::type* __restrict__ out, long out_ld,
                                                                  const float* __restrict__ gains) {
    using T = typename OutT<ENC>::type;
    extern __shared__ float xs[];
    const int n = blockIdx.y;
    const ResampleSegment sg = seg[n];
    const long k0 = (long)blockIdx.x * RS_TILE, k = k0 + threadIdx.x;
    const long cnt = (long)sg.m1 - sg.m0;
    T* orow = out + (long)n * out_ld;
    if (k0 >= cnt) {                                              // the whole tile lies after the segment (uniform per workgroup)
        if (k < out_ld) orow[k] = (T)0;
        return;
    }
    const long mf = sg.m0 + k0, ml = (sg.m0 + (k0 + RS_TILE < cnt ? k0 + RS_TILE : cnt)) - 1;
    const long base = (mf * M) / L - R;
    const int span = (int)((ml * M) / L + R - base) + 1;
    const float* xrow = wav + (long)sg.row * ld;
    float g = 1.f;
    if constexpr (GAIN) g = gains[sg.row];
    for (int i = threadIdx.x; i < span; i += RS_TILE) {
        const long a = base + i, rel = a - sg.origin;
        const bool in = a >= 0 && a < sg.n_valid && rel >= 0 && rel < ld;
        if constexpr (GAIN) xs[i] = in ? g * xrow[rel] : 0.f;
        else xs[i] = in ? xrow[rel] : 0.f;
    }
    __syncthreads();
    if (k >= cnt) {
        if (k < out_ld) orow[k] = (T)0;
        return;
    }
    const long mm = (sg.m0 + k) * M, j0 = mm / L;
    const int p = (int)(mm - j0 * L), W = 2 * R + 1;
    const float* t = table + (long)p * W;
    const float* xp = xs + (j0 - R - base);
    float acc = 0.f;
    for (int d = 0; d < W; ++d) acc = fmaf(xp[d], t[d], acc);
    if constexpr (ENC == RS_ENC_F32) orow[k] = acc;
    else if constexpr (ENC == RS_ENC_S16) orow[k] = (int16_t)to_s16(acc, max_wav);
    else if constexpr (ENC == RS_ENC_MULAW) orow[k] = (uint8_t)lin2ulaw(to_s16(acc, max_wav));
    else orow[k] = (uint8_t)lin2alaw(to_s16(acc, max_wav));
}

template <bool GAIN>
int launch_encode(const float* wav, long ld, const ResampleSegment* seg, const float* table, int L, int M, int R, int enc, float max_wav, void* out,
                  long out_ld, const float* gains, dim3 grid, size_t lds, hipStream_t s) {
    const dim3 block(RS_TILE);
    switch (enc) {
        case RS_ENC_F32:
            hipLaunchKernelGGL((resample_encode_kernel<RS_ENC_F32, GAIN>), grid, block, lds, s, wav, ld, seg, table, L, M, R, max_wav, (float*)out, out_ld, gains);
            break;
        case RS_ENC_S16:
            hipLaunchKernelGGL((resample_encode_kernel<RS_ENC_S16, GAIN>), grid, block, lds, s, wav, ld, seg, table, L, M, R, max_wav, (int16_t*)out, out_ld, gains);
            break;
        case RS_ENC_MULAW:
            hipLaunchKernelGGL((resample_encode_kernel<RS_ENC_MULAW, GAIN>), grid, block, lds, s, wav, ld, seg, table, L, M, R, max_wav, (uint8_t*)out, out_ld, gains);
            break;
        case RS_ENC_ALAW:
            hipLaunchKernelGGL((resample_encode_kernel<RS_ENC_ALAW, GAIN>), grid, block, lds, s, wav, ld, seg, table, L, M, R, max_wav, (uint8_t*)out, out_ld, gains);
            break;
        default:
            return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int cmtts_launch_resample_table(const float* taps, int L, int half, int R, float* table, void* stream) {
    hipLaunchKernelGGL(resample_table_kernel, dim3(cdiv((long)L * (2 * R + 1), 256)), dim3(256), 0, (hipStream_t)stream, taps, L, half, R, table);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_resample_encode_gain(const float* wav, long ld, const ResampleSegment* seg, int N, const float* table, int L, int M,
                                                 int R, int enc, float max_wav, void* out, long out_ld, const float* gains, void* stream) {
    if (N <= 0 || out_ld <= 0) return 0;
    const long span = ((long)(RS_TILE - 1) * M) / L + 2L * R + 2;          // floor steps of a tile's last output + both half-widths
    if (span > RS_MAX_SPAN) return -2;
    const dim3 grid(cdiv(out_ld, RS_TILE), N);
    const size_t lds = (size_t)span * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    // gains == NULL runs the instantiation without the multiplication: the kernel as it was before the gain existed
    return gains ? launch_encode<true>(wav, ld, seg, table, L, M, R, enc, max_wav, out, out_ld, gains, grid, lds, s)
                 : launch_encode<false>(wav, ld, seg, table, L, M, R, enc, max_wav, out, out_ld, nullptr, grid, lds, s);
}

extern "C" int cmtts_launch_resample_encode(const float* wav, long ld, const ResampleSegment* seg, int N, const float* table, int L, int M, int R,
                                            int enc, float max_wav, void* out, long out_ld, void* stream) {
    return cmtts_launch_resample_encode_gain(wav, ld, seg, N, table, L, M, R, enc, max_wav, out, out_ld, nullptr, stream);
}
