// Seeded per-utterance sampler noise, generated on the device (include/cmtts_hip.h: cmtts_noise_fill, cmtts_noise_fill_groups,
// cmtts_sample_seeded; cmtts_amd/noise.py is the same definition in numpy).
//
// The value at (utterance seed, draw, frame, mel bin) is a pure function of those four numbers — not of the batch size, the row,
// the padded T, the bucket, the rank or the launch shape:
//
//   bits     Philox4x32-10, standard constants: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85,
//            ten rounds; per round c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key bump
//   key      the utterance's 64-bit seed: (seed mod 2^32, seed >> 32)
//   counter  (j mod 2^32, j >> 32, draw, 0x434D5454) with j = (t0 + t) * ceil(M / 4) + floor(m / 4); t = frame row of the tensor,
//            t0 = the tensor's first frame, m = mel bin, M = n_mels.  Element (t, m) is lane m mod 4 of its block.
//   normals  Box-Muller on 24-bit uniforms, every conversion exact in fp32: u1 = ((x_a >> 8) + 1) * 2^-24, u2 = (x_b >> 8) * 2^-24,
//            r = sqrt(-2 ln u1); lanes 0, 1 = r cos(2 pi u2), r sin(2 pi u2) from (x0, x1), lanes 2, 3 the same from (x2, x3);
//            so |z| <= sqrt(48 ln 2) = 5.77
//   draws    0 is x_T, 1 + i the re-noise after evaluation i
//   math     logf, sqrtf and sincospif(2 u2): the full-precision device functions, no fast intrinsics, no fast-math flag.  Every
//            product of the chain is a lone multiplication (nothing for the compiler to contract), so both kernels below and both
//            store forms produce the same bits.
//
// One Philox block per lane = four normals, one 16-byte store when M % 4 == 0 and the tensor is 16-byte aligned (rows of 80
// floats keep that alignment), element stores otherwise.  Grid over (block chunk, utterance, draw): the seed is one load that is
// uniform over the workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "noise_philox.h"
#include "noise_device.h"

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

using noise_dev::U4;
using noise_dev::box_muller;

// One block: frame t (tensor row), quad q of the row.  `row` = the tensor row's first float, `brow` = its first uint32 block word.
template <bool VEC>
__device__ __forceinline__ void emit_block(uint64_t seed, uint32_t draw, uint64_t j, int q, int M, float scale, float* row, uint32_t* brow) {
    const U4 x = noise_dev::noise_block(seed, draw, j);
    if (brow) {
        *reinterpret_cast<uint4*>(brow + 4 * q) = make_uint4(x.x, x.y, x.z, x.w);
        return;
    }
    float z0, z1, z2, z3;
    box_muller(x.x, x.y, scale, z0, z1);
    box_muller(x.z, x.w, scale, z2, z3);
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(row + 4 * q) = make_float4(z0, z1, z2, z3);
    } else {
        const int m = 4 * q;
        row[m] = z0;                      // m < M by construction (q < ceil(M / 4))
        if (m + 1 < M) row[m + 1] = z1;
        if (m + 2 < M) row[m + 2] = z2;
        if (m + 3 < M) row[m + 3] = z3;
    }
}

// grid (ceil(T * Q / 256), B, n_draws), Q = ceil(M / 4)
template <bool VEC>
__global__ __launch_bounds__(256) void noise_fill_kernel(const int64_t* __restrict__ seeds, int B, int T, int M, int Q, int first_draw, int64_t t0,
                                                         float scale, float* __restrict__ out, uint32_t* __restrict__ bits) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;      // T * Q < 2^31 (launcher)
    if (i >= (uint32_t)T * (uint32_t)Q) return;
    const int b = blockIdx.y, d = blockIdx.z;
    const int t = (int)(i / (uint32_t)Q), q = (int)(i - (uint32_t)t * (uint32_t)Q);
    const uint64_t seed = (uint64_t)seeds[b];
    const uint64_t j = ((uint64_t)t0 + (uint64_t)t) * (uint64_t)Q + (uint64_t)q;
    const long rowi = ((long)d * B + b) * T + t;
    emit_block<VEC>(seed, (uint32_t)(first_draw + d), j, q, M, scale, out + rowi * M, bits ? bits + rowi * Q * 4 : nullptr);
}

// grid (sum over groups of B * wg_per_utt, n_draws): a workgroup finds its group in the table (uniform scan), then its utterance
template <bool VEC>
__global__ __launch_bounds__(256) void noise_fill_groups_kernel(NoiseGroupTable tab, int n_groups, int M, int Q, int first_draw) {
    const int wg = blockIdx.x;
    int g = 0;
    while (g + 1 < n_groups && wg >= tab.g[g + 1].wg0) ++g;
    const int32_t B = tab.g[g].B, T = tab.g[g].T, per = tab.g[g].wg_per_utt;
    const int local = wg - tab.g[g].wg0;
    const int b = local / per;
    const uint32_t i = (uint32_t)(local - b * per) * 256u + threadIdx.x;      // T * Q < 2^31 (launcher)
    if (b >= B || i >= (uint32_t)T * (uint32_t)Q) return;
    const int d = blockIdx.y;
    const int t = (int)(i / (uint32_t)Q), q = (int)(i - (uint32_t)t * (uint32_t)Q);
    const uint64_t seed = (uint64_t)tab.g[g].seeds[b];
    const uint64_t j = (uint64_t)t * (uint64_t)Q + (uint64_t)q;
    const long rowi = ((long)d * B + b) * T + t;
    emit_block<VEC>(seed, (uint32_t)(first_draw + d), j, q, M, 1.0f, tab.g[g].out + rowi * M, nullptr);
}

bool vec_ok(const void* p, int M) { return (M & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int cmtts_launch_noise_fill(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, float scale, float* out,
                                       uint32_t* bits, void* stream) {
    const int Q = (M + 3) / 4;
    const dim3 grid(cdiv((long)T * Q, 256), B, n_draws);
    if ((long)T * Q > 0x7fffff00L || grid.y > 65535u || grid.z > 65535u) return -2;
    if (bits || vec_ok(out, M))
        hipLaunchKernelGGL(noise_fill_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, seeds, B, T, M, Q, first_draw, t0, scale, out, bits);
    else
        hipLaunchKernelGGL(noise_fill_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, seeds, B, T, M, Q, first_draw, t0, scale, out, bits);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_noise_fill_groups(const NoiseGroup* groups, int n_groups, int M, int first_draw, int n_draws, void* stream) {
    const int Q = (M + 3) / 4;
    if (n_draws > 65535) return -2;
    for (int g0 = 0; g0 < n_groups; g0 += NOISE_MAX_GROUPS) {
        const int n = n_groups - g0 < NOISE_MAX_GROUPS ? n_groups - g0 : NOISE_MAX_GROUPS;
        NoiseGroupTable tab;
        long wg = 0;
        bool vec = true;
        for (int k = 0; k < NOISE_MAX_GROUPS; ++k) {
            tab.g[k] = k < n ? groups[g0 + k] : NoiseGroup{nullptr, nullptr, 0, 0, 0, 1};
            if (k >= n) continue;
            if ((long)tab.g[k].T * Q > 0x7fffff00L) return -2;
            tab.g[k].wg_per_utt = cdiv((long)tab.g[k].T * Q, 256);
            tab.g[k].wg0 = (int32_t)wg;
            wg += (long)tab.g[k].B * tab.g[k].wg_per_utt;
            vec = vec && vec_ok(tab.g[k].out, M);
        }
        if (wg > 0x7fffffffL) return -2;
        const dim3 grid((unsigned)wg, n_draws);
        if (vec) hipLaunchKernelGGL(noise_fill_groups_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, tab, n, M, Q, first_draw);
        else hipLaunchKernelGGL(noise_fill_groups_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, tab, n, M, Q, first_draw);
        if (hipGetLastError() != hipSuccess) return -3;
    }
    return 0;
}
