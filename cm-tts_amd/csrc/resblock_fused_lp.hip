// Reduced-precision variant of the fused denoiser residual block (resblock_fused.hip): the two
// contractions run on v_mfma_f32_32x32x16_{bf16,f16} (fp32 accumulate, 16x the fp32 MFMA rate); x, cp,
// x', skip, biases, the gate and the residual arithmetic stay fp32 in HBM and registers.  This is the
// denoiser of BASELINE.json configs[2] (bf16) and configs[4] (fp16); the reference has no reduced-
// precision inference path, so parity is stated against the fp32 oracle with its own
// tolerance (tests/test_gpu_parity.py::test_reduced_precision_denoiser).
//
// Layout differences from the fp32 kernel, all forced by the K=16 MFMA fragment (lane l supplies
// 8 consecutive k of row/column l&31, k half = l>>5):
//  * u and z live in LDS TRANSPOSED and converted: [frame][channel] 16-bit, row stride 520 B, so a
//    B fragment is 16 contiguous bytes (two conflict-free ds_read_b64) and a tap is a row offset;
//  * weights are re-packed per layer as [tap][k-group of 16][m-tile][lane][8 x 16-bit]: one
//    global_load_dwordx4 per MFMA, streamed L2 -> VGPR through a 4-deep register ring.
// At this MFMA rate the kernel is bound by the weight fill (1.05 MB per workgroup) and by the HBM
// bursts, not by the matrix pipe.
// What stays fp32 is the fp32 kernels' own source: the gate's bias fetch and the x' / skip epilogue are resblock_direct.h's.
#include <hip/hip_runtime.h>
#include "cvt16.h"
#include "resblock_direct.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int C = 256;
constexpr int NW = 16;
constexpr int FN = 64;
constexpr int NT = FN / 32;
constexpr int RS = 260;          // 16-bit elements per LDS row (520 B: 8-B aligned rows, bank stride 2 dwords)
constexpr int RING = 4;

template <int MODE>
__global__ __launch_bounds__(64 * NW, 4) void resblock_fused_lp_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned short ut[];   // [FN + 2][RS]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * FN;
    const int T = a.T;
    const int l31 = lane & 31, khalf = lane >> 5;
    const float* xin = a.x_in + (long)b * C * T;
    const float* cp = a.cp + (long)b * a.cp_bstride;
    const float* dp = a.dp + (long)b * a.vec_stride;

    // ---- stage u^T[j][m] = cvt(cp + (x + dp)), j = frame - (t0 - 1); lane = frame, waves over channel pairs
    bool ovf = false;
    {
        const int t = t0 + lane;
        const int t_c = min(t, T - 1);
#pragma unroll 1
        for (int i = 0; i < C / (2 * NW); i += 4) {
            float x0[4], x1[4], c0[4], c1[4], d0[4], d1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = 2 * (w + NW * (i + q));
                x0[q] = xin[(unsigned)(m * T + t_c)];
                x1[q] = xin[(unsigned)((m + 1) * T + t_c)];
                c0[q] = cp[(unsigned)(m * T + t_c)];
                c1[q] = cp[(unsigned)((m + 1) * T + t_c)];
                d0[q] = dp[m];
                d1[q] = dp[m + 1];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = 2 * (w + NW * (i + q));
                const float u0 = c0[q] + (x0[q] + d0[q]);
                const float u1 = c1[q] + (x1[q] + d1[q]);
                const unsigned pk = t < T ? pack16<MODE>(u0, u1) : 0u;
                *reinterpret_cast<unsigned*>(ut + (1 + lane) * RS + m) = pk;
                // fp16: an input beyond the type's range converts to something finite and WRONG — reported (code 3, cmtts_poll_error)
                if (MODE == 2) ovf |= t < T && !(fabsf(u0) <= 65504.0f && fabsf(u1) <= 65504.0f);
            }
        }
        if (MODE == 2 && ovf && a.flag && *(volatile unsigned*)a.flag == 0u) *(volatile unsigned*)a.flag = 3u;
        if (tid < 2 * C) {
            const int m = tid & (C - 1);
            const bool right = tid >= C;
            const int th = right ? t0 + FN : t0 - 1;
            const int thc = min(max(th, 0), T - 1);
            const float uh = cp[(unsigned)(m * T + thc)] + (xin[(unsigned)(m * T + thc)] + dp[m]);
            ut[(right ? FN + 1 : 0) * RS + m] = (th >= 0 && th < T) ? (unsigned short)pack16<MODE>(uh, 0.f) : (unsigned short)0;
        }
    }
    __syncthreads();   // (1) u staged

    f32x16 acc[NT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    };
    auto load_a = [&](u32x4& dst, const void* wfrag, int group) {   // group = tap * 16 + k-group
        dst = *(reinterpret_cast<const u32x4*>(wfrag) + ((long)group * (2 * C / 32) + w) * 64 + lane);
    };
    auto load_b = [&](u32x4 (&dst)[NT], int kg, int row_off) {      // 16 bytes = 8 k-values of one frame
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const unsigned short* p = ut + (j * 32 + l31 + row_off) * RS + kg * 16 + khalf * 8;
            const u32x2 lo = *reinterpret_cast<const u32x2*>(p);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(p + 4);
            dst[j] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
        }
    };

    // =============================================================== phase B: gated k=3 conv, 48 k-groups
    {
        zero_acc();
        constexpr int NG = 3 * (C / 16);
        u32x4 A[RING], Bv[2][NT];
#pragma unroll
        for (int s = 0; s < RING - 1; ++s) load_a(A[s], a.W3f, s);
        load_b(Bv[0], 0, 0);
        for (int it = 0; it < NG; it += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                load_a(A[(s + RING - 1) % RING], a.W3f, min(it + s + RING - 1, NG - 1));
                const int nx = min(it + s + 1, NG - 1);
                load_b(Bv[(s + 1) & 1], nx & 15, nx >> 4);      // group = tap * 16 + kg
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = mma16<MODE>(A[s], Bv[s & 1][j], acc[j]);
            }
        }
    }
    __syncthreads();   // (2) u dead: its buffer becomes z^T
    {
        float bg[8], bf[8];
        resdirect::gate_bias(bg, bf, a.b3, w, lane);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 8; r += 2) {     // registers r, r+1 = adjacent channels (even first)
                const float z0 = cmtts_gate(acc[j][r] + bg[r], acc[j][r + 8] + bf[r]);
                const float z1 = cmtts_gate(acc[j][r + 1] + bg[r + 1], acc[j][r + 9] + bf[r + 1]);
                const int ch = w * 16 + acc_row(r, lane);
                *reinterpret_cast<unsigned*>(ut + (j * 32 + l31) * RS + ch) = pack16<MODE>(z0, z1);
            }
    }
    __syncthreads();   // (3) z complete

    // =============================================================== phase C: output projection, 16 k-groups
    {
        zero_acc();
        constexpr int NG = C / 16;
        u32x4 A[RING], Bv[2][NT];
#pragma unroll
        for (int s = 0; s < RING - 1; ++s) load_a(A[s], a.Wof, s);
        load_b(Bv[0], 0, 0);
        for (int it = 0; it < NG; it += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                load_a(A[(s + RING - 1) % RING], a.Wof, min(it + s + RING - 1, NG - 1));
                load_b(Bv[(s + 1) & 1], min(it + s + 1, NG - 1), 0);
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = mma16<MODE>(A[s], Bv[s & 1][j], acc[j]);
            }
        }
        resdirect::epilogue(acc, a, b, t0, w, lane);     // fp32, the fp32 kernels' x' / skip expressions
    }
}

template <int MODE>
int launch_lp(const ResArgs& a, hipStream_t stream) {
    const size_t lds = (size_t)(FN + 2) * RS * sizeof(unsigned short);
    dim3 grid((a.T + FN - 1) / FN, a.B);
    hipLaunchKernelGGL(resblock_fused_lp_kernel<MODE>, grid, dim3(64 * NW), lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

// mode: 1 = bf16, 2 = fp16 operands.  a->W3f / a->Wof point to the 16-bit fragment-order weights.  -2 not served: any other mode, an empty
// batch, rows beyond the 32-bit element index, x' written over x.
extern "C" int cmtts_launch_resblock_lp(const ResArgs* a, int mode, void* stream) {
    if (mode != 1 && mode != 2) return -2;
    if (a->B <= 0 || a->T <= 0 || (long)C * a->T >= (1L << 31) || a->x_out == a->x_in) return -2;
    ResArgs c = *a;
    c.dbg = nullptr;
    return mode == 1 ? launch_lp<1>(c, (hipStream_t)stream) : launch_lp<2>(c, (hipStream_t)stream);
}
