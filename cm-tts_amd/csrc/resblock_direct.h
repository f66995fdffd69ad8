// The fp32 DIRECT form of the denoiser residual block, piece by piece — one source for every per-layer kernel that promises the same
// bits: resblock_fused_kernel<32> / <64> (16 waves, one workgroup per tile), the two kernels of resblock_split.hip (the <32> tile cut
// into four workgroups of 4 waves), and — gate bias and x' / skip epilogue only — the 16-bit kernel of resblock_fused_lp.hip.
//
//   u  = cp + (x + dp)                                             stage_u
//   y  = W3 (*) u ; z = gate(y[:C] + b3[:C], y[C:] + b3[C:])       conv_k3, gate
//   o  = Wo * z + bo ; x' = (o[:C] + (x + d)) / sqrt(2) ; skip (+)= o[C:]      project, epilogue
//
// A wave is identified by its m-tile mt in [0, 16): 32 rows of the 512-row output of either contraction (the wave index in the fused
// kernel, blockIdx.z * 4 + wave in the split ones).  Everything a wave computes depends on mt, its lane, the tile (b, t0) and the frames
// per tile FN alone, never on how many waves share its workgroup: that is the bitwise contract between the forms
// (tests/test_gpu_parity.py::test_fused_resblock_bitwise, test_split_resblock_bitwise).  LDS tiles are [C][FN + 4] fp32.
#pragma once
#include <hip/hip_runtime.h>
#include "gate.h"
#include "mfma_lane.h"
#include "resblock_args.h"

namespace resdirect {

constexpr int C = 256;          // residual channels (= encoder hidden)
constexpr int RING = 4;         // register ring depth for the weight stream

// ---- stage u[m][j] = cp + (x + dp) for frames t0-1+j, j in [0, FN+2); zero outside [0,T) (conv padding).  NW waves share the C rows.
// Unconditional clamped loads, selects at LDS-store time, 8 rows in flight per thread; lanes = (row parity, frame) at FN = 32.
template <int FN, int NW>
__device__ __forceinline__ void stage_u(float* u_lds, const float* xin, const float* cp, const float* dp, int t0, int T, int tid) {
    constexpr int U_LD = FN + 4;
    constexpr int RPI = 64 / FN;                 // rows covered by one wave-wide access (2 or 1)
    constexpr int ROWS_PER_WAVE = C / NW;
    const int lane = tid & 63, w = tid >> 6;
    const int n = lane & (FN - 1);
    const int rsub = RPI == 2 ? lane >> 5 : 0;
    const int t = t0 + n;
    const int t_c = min(t, T - 1);
#pragma unroll 1
    for (int i = 0; i < ROWS_PER_WAVE / RPI; i += 8) {
        float xv[8], cv[8], dq[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = w * ROWS_PER_WAVE + (i + q) * RPI + rsub;
            xv[q] = xin[(unsigned)(m * T + t_c)];
            cv[q] = cp[(unsigned)(m * T + t_c)];
            dq[q] = dp[m];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = w * ROWS_PER_WAVE + (i + q) * RPI + rsub;
            const float uv = cv[q] + (xv[q] + dq[q]);
            u_lds[m * U_LD + 1 + n] = t < T ? uv : 0.f;
        }
    }
    for (int i = tid; i < 2 * C; i += 64 * NW) {   // halo columns: (side, row)
        const int m = i & (C - 1);
        const bool right = i >= C;
        const int th = right ? t0 + FN : t0 - 1;
        const int thc = min(max(th, 0), T - 1);
        const float uh = cp[(unsigned)(m * T + thc)] + (xin[(unsigned)(m * T + thc)] + dp[m]);
        u_lds[m * U_LD + (right ? FN + 1 : 0)] = (th >= 0 && th < T) ? uh : 0.f;
    }
}

// ---- the k-group stream.  A fragments of one k-group (8 input channels = 4 k-steps) for m-tile mt: one coalesced 16-byte load per lane
__device__ __forceinline__ void load_a(f32x4& dst, const float* wfrag, int group, int mt, int lane) {
    dst = *reinterpret_cast<const f32x4*>(wfrag + ((long)group * (2 * C / 32) + mt) * 256 + lane * 4);
}
// B operands of one k-group: rows krow0 + 2kk + khalf of the LDS tile at column offset `col`
template <int NT>
__device__ __forceinline__ void load_b(float (&dst)[4][NT], const float* tile, int krow0, int col, int lane) {
    constexpr int U_LD = NT * 32 + 4;
    const float* bs = tile + (krow0 + (lane >> 5)) * U_LD + (lane & 31) + col;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j) dst[kk][j] = bs[2 * kk * U_LD + j * 32];
}
template <int NT>
__device__ __forceinline__ void mma_group(f32x16 (&acc)[NT], const f32x4& af, const float (&bv)[4][NT]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bv[kk][j], acc[j], 0, 0, 0);
}
template <int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
}

// acc = W3 (*) u, K = 3 x 256 in conv_mfma.hip's order: 96 k-groups, (16-channel chunk, tap, 8-half).  A 4-deep register ring keeps three
// weight groups in flight; the B operands run one group ahead of the MFMAs that consume them.
template <int NT>
__device__ __forceinline__ void conv_k3(f32x16 (&acc)[NT], const float* W3f, const float* u_lds, int mt, int lane) {
    zero_acc(acc);
    constexpr int NG = (C / 8) * 3;
    auto kgrp = [&](int it, int& g8, int& tap) {           // iteration -> (k-group of 8 channels, tap)
        it = min(it, NG - 1);
        const int q = it / 6, rr = it - q * 6;
        tap = rr >> 1;
        g8 = 2 * q + (rr & 1);
    };
    f32x4 A[RING];
    float Bv[2][4][NT];
    int g8, tap;
#pragma unroll
    for (int s = 0; s < RING - 1; ++s) {
        kgrp(s, g8, tap);
        load_a(A[s], W3f, tap * (C / 8) + g8, mt, lane);
    }
    kgrp(0, g8, tap);
    load_b(Bv[0], u_lds, g8 * 8, tap, lane);
    for (int it = 0; it < NG; it += RING) {
#pragma unroll
        for (int s = 0; s < RING; ++s) {
            kgrp(it + s + RING - 1, g8, tap);
            load_a(A[(s + RING - 1) % RING], W3f, tap * (C / 8) + g8, mt, lane);
            kgrp(it + s + 1, g8, tap);
            load_b(Bv[(s + 1) & 1], u_lds, g8 * 8, tap, lane);
            __builtin_amdgcn_sched_barrier(0);
            mma_group(acc, A[s], Bv[s & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// acc = Wo * z, K = 256: 32 k-groups in ascending order through the same ring
template <int NT>
__device__ __forceinline__ void project(f32x16 (&acc)[NT], const float* Wof, const float* z_lds, int mt, int lane) {
    zero_acc(acc);
    constexpr int NG = C / 8;
    f32x4 A[RING];
    float Bv[2][4][NT];
#pragma unroll
    for (int s = 0; s < RING - 1; ++s) load_a(A[s], Wof, s, mt, lane);
    load_b(Bv[0], z_lds, 0, 0, lane);
    for (int it = 0; it < NG; it += RING) {
#pragma unroll
        for (int s = 0; s < RING; ++s) {
            load_a(A[(s + RING - 1) % RING], Wof, min(it + s + RING - 1, NG - 1), mt, lane);
            load_b(Bv[(s + 1) & 1], z_lds, min(it + s + 1, NG - 1) * 8, 0, lane);
            __builtin_amdgcn_sched_barrier(0);
            mma_group(acc, A[s], Bv[s & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- gate.  M-tile mt = [16 sigmoid rows | 16 tanh rows] of channels [16 mt, +16): registers r (rows 0-15) and r+8 (rows 16-31) of the
// same lane pair up.  gate_bias fetches the two biases of register pair r; gate hands z of (n-tile j, channel, register pair) to `store`.
__device__ __forceinline__ void gate_bias(float (&bg)[8], float (&bf)[8], const float* b3, int mt, int lane) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int mg = mt * 32 + acc_row(r, lane);
        bg[r] = b3[mg];
        bf[r] = b3[mg + 16];
    }
}
template <int NT, class Store>
__device__ __forceinline__ void gate(const f32x16 (&acc)[NT], const float* b3, int mt, int lane, Store store) {
    float bg[8], bf[8];
    gate_bias(bg, bf, b3, mt, lane);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 8; ++r)
            store(j, mt * 16 + acc_row(r, lane), cmtts_gate(acc[j][r] + bg[r], acc[j][r + 8] + bf[r]));
}

// ---- x' / skip epilogue of m-tile mt over the tile's NT n-tiles: m-tiles 0-7 (rows [0,256) of o) -> x', 8-15 (rows [256,512)) -> skip.
// res_half is wave-uniform.  Per n-tile: all 16 gathers, then all the arithmetic, then the 16 predicated stores.  Two things keep the
// gathers in flight together and the stores back to back in every caller (checked in the assembly of both fused tiles, the split out
// kernel and the 16-bit kernel: no s_waitcnt between the loads, none between the stores):
//  * the gather offset is formed in 32 bits (ldg).  As src[(unsigned)idx] the compiler formed it with a 64-bit multiply-add whose unused
//    high half was the destination of a bias load just issued, and the wait-count pass then put s_waitcnt vmcnt(1) in front of every
//    gather: 16 L2 round trips one after another in resblock_split_out_kernel;
//  * a store issued while gathers are still pending makes the compiler wait for every store before the next one (loads and stores
//    share the counter), so the arithmetic of all 16 registers comes before the first store.
template <int NT>
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[NT], const ResArgs& a, int b, int t0, int mt, int lane) {
    const int T = a.T;
    const float* xin = a.x_in + (long)b * C * T;
    const float* dv = a.d + (long)b * a.vec_stride;
    float* xout = a.x_out + (long)b * C * T;
    float* skip = a.skip + (long)b * C * T;
    const bool res_half = mt < C / 32;
    const float* src = res_half ? xin : skip;
    float* dst = res_half ? xout : skip;
    const bool need_src = res_half || a.accum_skip;
    const int mrow0 = (mt % (C / 32)) * 32;                 // row inside the half
    float bo[16], dd[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bo[r] = a.bo[mt * 32 + acc_row(r, lane)];
        dd[r] = res_half ? dv[mrow0 + acc_row(r, lane)] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int t = t0 + j * 32 + (lane & 31);
        const int t_c = min(t, T - 1);
        float sv[16], v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            sv[r] = need_src ? ldg(src, (unsigned)((mrow0 + acc_row(r, lane)) * T + t_c)) : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float o = acc[j][r] + bo[r];
            if (res_half) v[r] = (o + (sv[r] + dd[r])) * CMTTS_RSQRT2;
            else v[r] = a.accum_skip ? o + sv[r] : o;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (t < T) dst[(unsigned)((mrow0 + acc_row(r, lane)) * T + t)] = v[r];
    }
}

}  // namespace resdirect
