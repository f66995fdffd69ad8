// The Winograd F(4,3) pieces of the denoiser's gated k = 3 conv (points 0, +-1, +-2, inf; denoiser_persist.hip header comment): the
// input transform of one quad, the output transform and the gate on row pairs.  Used by the persistent stack's WINO == 2 instances and
// by the per-layer form of the same conv (resblock_split_w43.hip): one source for both, so every z element of either comes from the
// same operation sequence (tests/test_gpu_batch_invariant.py).
#pragma once
#include <hip/hip_runtime.h>

namespace wino43 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// d0..d5 = u(4q-1 .. 4q+4) as Da = d0..d3, Db = d4, d5 -> V0 = 4 d0 - 5 d2 + d4, V1 = (d4 - 4 d2) + (d3 - 4 d1), V2 = (d4 - 4 d2) - (d3 - 4 d1),
// V3 = (d4 - d2) + 2 (d3 - d1), V4 = (d4 - d2) - 2 (d3 - d1), V5 = 4 d1 - 5 d3 + d5.
// (written on float pairs: the compiler then issues v_pk_fma_f32 / v_pk_add_f32 — 8 VALU operations per k-step instead of 12 + moves;
//  the same fused operations on the same values)
__device__ __forceinline__ void transform(const f32x4& Da, const float2& Db, float (&V)[6]) {
    const f32x2 P01 = {Da[0], Da[1]}, P23 = {Da[2], Da[3]}, P45 = {Db.x, Db.y};
    const f32x2 c4 = {4.f, 4.f}, cm5 = {-5.f, -5.f}, c2 = {2.f, -2.f};
    const f32x2 V05 = __builtin_elementwise_fma(c4, P01, __builtin_elementwise_fma(cm5, P23, P45));
    const float t0 = __builtin_fmaf(-4.f, Da[2], Db.x), t1 = __builtin_fmaf(-4.f, Da[1], Da[3]);
    const float t2 = Db.x - Da[2], t3 = Da[3] - Da[1];
    const f32x2 a0 = {t0, t0}, a1 = {t1, -t1}, b0 = {t2, t2}, b1 = {t3, t3};
    const f32x2 V12 = a0 + a1;
    const f32x2 V34 = __builtin_elementwise_fma(c2, b1, b0);
    V[0] = V05.x; V[1] = V12.x; V[2] = V12.y; V[3] = V34.x; V[4] = V34.y; V[5] = V05.y;
}

// output transform of two adjacent accumulator rows: y0 = m0 + (m1 + m2) + (m3 + m4), y1 = (m1 - m2) + 2 (m3 - m4), y2 = (m1 + m2) + 4 (m3 + m4),
// y3 = (m1 - m2) + 8 (m3 - m4) + m5, each + bias
__device__ __forceinline__ void out_transform(f32x2 m0, f32x2 m1, f32x2 m2, f32x2 m3, f32x2 m4, f32x2 m5, f32x2 bias, f32x2 (&y)[4]) {
    const f32x2 s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
    const f32x2 c2 = {2.f, 2.f}, c4 = {4.f, 4.f}, c8 = {8.f, 8.f};
    y[0] = ((m0 + s12) + s34) + bias;
    y[1] = __builtin_elementwise_fma(c2, d34, d12) + bias;
    y[2] = __builtin_elementwise_fma(c4, s34, s12) + bias;
    y[3] = (__builtin_elementwise_fma(c8, d34, d12) + m5) + bias;
}

// cmtts_gate (gate.h) on two elements: the same multiplies, v_exp / v_rcp, adds and fma per element
__device__ __forceinline__ f32x2 gate2(f32x2 g, f32x2 f) {
    const f32x2 nl2e = {-1.44269504088896340736f, -1.44269504088896340736f}, l2e = {1.44269504088896340736f, 1.44269504088896340736f};
    const f32x2 one = {1.f, 1.f}, m2c = {-2.f, -2.f};
    const f32x2 ag = g * nl2e;
    const f32x2 eg = {__builtin_amdgcn_exp2f(ag.x), __builtin_amdgcn_exp2f(ag.y)};
    const f32x2 dg = one + eg;
    const f32x2 sg = {__builtin_amdgcn_rcpf(dg.x), __builtin_amdgcn_rcpf(dg.y)};
    const f32x2 af = (f + f) * l2e;
    const f32x2 ef = {__builtin_amdgcn_exp2f(af.x), __builtin_amdgcn_exp2f(af.y)};
    const f32x2 df = one + ef;
    const f32x2 rf = {__builtin_amdgcn_rcpf(df.x), __builtin_amdgcn_rcpf(df.y)};
    const f32x2 th = __builtin_elementwise_fma(m2c, rf, one);
    return sg * th;
}

}  // namespace wino43
