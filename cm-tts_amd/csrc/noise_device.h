// Device functions of the seeded sampler noise (the definition: noise_philox.hip's header comment, cmtts_amd/noise.py): the Philox4x32-10
// block and Box-Muller on 24-bit uniforms.  Shared by the units that generate that noise — noise_philox.hip (the fill kernels) and
// retake.hip (the masked sampler's step kernel, which draws its re-noise in place) — so that both produce the same bits: every product
// of the chain is a lone multiplication (nothing for the compiler to contract), logf / sqrtf / sincospif are the full-precision device
// functions.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace noise_dev {

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float scale, float& za, float& zb) {
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;      // (0, 1], exact
    const float u2x2 = (float)(xb >> 8) * 0x1p-23f;           // 2 u2 in [0, 2), exact
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(u2x2, &sn, &cs);
    const float a = r * cs, b = r * sn;
    za = a * scale;      // the expression of scale_kernel (kernels.hip) on the rounded normal: the bits of a fill followed by k_scale
    zb = b * scale;
}

// The block of (seed, draw, j): counter (j mod 2^32, j >> 32, draw, "CMTT"), key = the two halves of the seed
__device__ __forceinline__ U4 noise_block(uint64_t seed, uint32_t draw, uint64_t j) {
    return philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), draw, 0x434D5454u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace noise_dev
