// Per-layer form of the persistent denoiser stack's Winograd F(4,3) residual block (denoiser_persist.hip, WINO == 2) for SMALL batches.
// The model option "batch_invariant" (denoiser_side.hip) routes every residual layer that would run in the direct form (resblock_fused.hip,
// resblock_split.hip, the three-launch path) through this conv kernel + resblock_split.hip's projection kernel, so that an utterance's mel
// has the same bits whether its batch took the persistent stack (large batches) or the per-layer kernels (small ones).
//
// A 64-frame tile (16 frame quads = one n-tile of v_mfma_f32_16x16x4_f32: the persistent kernel's lane mapping) is cut along the z rows
// into four workgroups of 4 waves.  A wave owns 16 z channels: the sigmoid and the tanh m-tile of one half of a persistent wave's rows.
//   * stage u = cp + (x + d [+ p]) for the tile and its two halo frames, zero outside [0, T) (every workgroup stages all 256 input rows,
//     from L2) — or copy the u that the three-launch path already formed (ResArgs::u);
//   * per k-step (4 channels): the six inputs u(4q-1 .. 4q+4) of the lane's quad, their input transform, 2 m-tiles x 6 transforms = 12 MFMAs;
//   * output transform, gate, z -> HBM scratch [B][256][T].
// Bitwise contract with the persistent instance (tests/test_gpu_batch_invariant.py): the same transformed weights (to_wino43_fragments), the
// same quad inputs with the same zero masking, the same input / output transforms and gate (wino43.h: one source for both kernels), the same
// MFMA over the same k-steps in the same ascending order per accumulator.  Which wave owns which rows changes no arithmetic.
// The projection + x' / skip epilogue is resblock_split.hip's out kernel: the persistent stack's projection and epilogue are those of the
// direct form in every instance (the F(4,3) instance parks x in `xst` between layers and reads back the same bits).
// Per wave 64 k-steps x 12 MFMAs of 32 cycles — the matrix time of one wave of the direct split kernel on a 32-frame tile — for twice the
// frames: half the waves per utterance at the same per-layer latency.
#include <hip/hip_runtime.h>
#include "resblock_direct.h"
#include "wino43.h"

using wino43::f32x2;
using wino43::f32x4;

namespace {

constexpr int C = 256;
constexpr int FN = 64;          // frames per tile: 16 quads
constexpr int NWS = 4;          // waves per workgroup (one per SIMD)
constexpr int MS = 4;           // workgroups per tile: 16 waves x 16 z channels
constexpr int U_LD = FN + 4;    // column f + 1 = frame t0 + f, f in [-1, FN]
constexpr int NS4 = C / 4;      // k-steps of four channels
constexpr int RING = 4;         // k-steps of transformed weights in flight + the one in use
constexpr int PW = 8;           // waves of the persistent instance: the packed layout is [NS4 + 4][PW][6 transforms][64 lanes][4 m-tiles]
constexpr int PAD_ROWS = 4;     // u rows behind the tile: the look-ahead read behind the last k-step lands there (discarded)
static_assert(NS4 % RING == 0, "the k loop runs whole ring rounds");

__global__ __launch_bounds__(64 * NWS) void resblock_w43_conv_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) float u_lds[];     // [C + PAD_ROWS][U_LD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * FN, T = a.T;
    const int zc = blockIdx.z * NWS + w;           // z channels [16 zc, +16): half zc & 1 of persistent wave zc >> 1
    const int pw = zc >> 1, cb = zc & 1;
    const float* uin = a.u ? a.u + (long)b * C * T : nullptr;

    // ---- stage: lanes = frames, 8 rows in flight per thread; the persistent kernel's expressions (layer 0: u = cp + (x + dp); later
    // layers form the same value from x' in registers) — resblock_direct.h's staging at 64 frames and 4 waves — or a copy of a->u
    if (uin) {
        const int t = t0 + lane, t_c = min(t, T - 1);
        constexpr int ROWS_PER_WAVE = C / NWS;       // 64
#pragma unroll 1
        for (int i = 0; i < ROWS_PER_WAVE; i += 8) {
            float uv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) uv[q] = uin[(unsigned)((w * ROWS_PER_WAVE + i + q) * T + t_c)];
#pragma unroll
            for (int q = 0; q < 8; ++q) u_lds[(w * ROWS_PER_WAVE + i + q) * U_LD + 1 + lane] = t < T ? uv[q] : 0.f;
        }
        for (int i = tid; i < 2 * C; i += 64 * NWS) {   // halo columns: (side, row)
            const int m = i & (C - 1);
            const bool right = i >= C;
            const int th = right ? t0 + FN : t0 - 1;
            const int thc = min(max(th, 0), T - 1);
            u_lds[m * U_LD + (right ? FN + 1 : 0)] = (th >= 0 && th < T) ? uin[(unsigned)(m * T + thc)] : 0.f;
        }
    } else {
        resdirect::stage_u<FN, NWS>(u_lds, a.x_in + (long)b * C * T, a.cp + (long)b * a.cp_bstride, a.dp + (long)b * a.vec_stride, t0, T, tid);
    }
    __syncthreads();

    // ---- gated k = 3 conv as F(4,3): lane (q = l & 15, k = l >> 4) holds quad q's six inputs in channel 4 ks + k; accumulator [i][p] =
    // m-tile 2 cb + i (sigmoid rows, then tanh rows) of persistent wave pw, transform p
    f32x4 acc[2][6];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[i][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        constexpr int KS_BYTES = PW * 6 * 64 * 16;      // one k-step of the packed array
        // (buffer loads: out-of-range k-steps read zeros; the packer pads every layer's array by 4 k-steps anyway)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.W3f), 0, (NS4 + 4) * KS_BYTES, 0x00020000);
        const int voff = (pw * 6 * 64 + lane) * 16 + cb * 8;      // elements 2 cb, 2 cb + 1 of the lane's fragment = this wave's two m-tiles
        f32x2 A[RING][6];
        auto load_a = [&](f32x2 (&dst)[6], int ks) {
#pragma unroll
            for (int p = 0; p < 6; ++p) dst[p] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff + p * 1024, ks * KS_BYTES, 0));
        };
        f32x4 Da;
        float2 Db;
        float V[6];
        auto load_d = [&](int ks) {
            const float* rr = u_lds + (4 * ks + (lane >> 4)) * U_LD + 4 * (lane & 15);
            Da = *reinterpret_cast<const f32x4*>(rr);
            Db = *reinterpret_cast<const float2*>(rr + 4);
        };
#pragma unroll
        for (int s = 0; s < RING - 1; ++s) load_a(A[s], s);
        load_d(0);
#pragma unroll 1
        for (int s0 = 0; s0 < NS4; s0 += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                const int ks = s0 + s;
                wino43::transform(Da, Db, V);
                __builtin_amdgcn_sched_barrier(0);
                load_a(A[(s + RING - 1) % RING], ks + RING - 1);
                load_d(ks + 1);
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[i][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s][p][i], V[p], acc[i][p], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // ---- output transform + gate on row pairs (accumulator registers 2 h, 2 h + 1 = rows 4 rb + 2 h, + 1 of the m-tile); lane q4 holds
    // output frames 4 q4 .. 4 q4 + 3 of the tile
    const int q4 = lane & 15, rb = lane >> 4;
    float bg[4], bf[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bg[r] = a.b3[64 * pw + 32 * cb + 4 * rb + r];
        bf[r] = a.b3[64 * pw + 32 * cb + 16 + 4 * rb + r];
    }
    float* zb = a.z + (long)b * C * T;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        auto P = [&](int i, int p) { return f32x2{acc[i][p][2 * h], acc[i][p][2 * h + 1]}; };
        f32x2 yg[4], yf[4];
        wino43::out_transform(P(0, 0), P(0, 1), P(0, 2), P(0, 3), P(0, 4), P(0, 5), f32x2{bg[2 * h], bg[2 * h + 1]}, yg);
        wino43::out_transform(P(1, 0), P(1, 1), P(1, 2), P(1, 3), P(1, 4), P(1, 5), f32x2{bf[2 * h], bf[2 * h + 1]}, yf);
        const int zr = 16 * zc + 4 * rb + 2 * h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x2 zz = wino43::gate2(yg[e], yf[e]);
            const int t = t0 + 4 * q4 + e;
            if (t < T) {
                zb[(unsigned)(zr * T + t)] = zz.x;
                zb[(unsigned)((zr + 1) * T + t)] = zz.y;
            }
        }
    }
}

}  // namespace

// ResidualBlock.forward in the F(4,3) form as two launches (this conv kernel, resblock_split.hip's projection kernel); needs a->z (scratch
// [B][256][T]) and a->W3f = the layer's F(4,3) fragments (to_wino43_fragments).  0 ok, -2 not served (no scratch / shape / x' written over x), -3 HIP error.
extern "C" int cmtts_launch_resblock_w43(const ResArgs* ap, void* stream_) {
    const ResArgs& a = *ap;
    hipStream_t stream = (hipStream_t)stream_;
    if (!a.z || !a.W3f || a.B <= 0 || a.B > 65535 || a.T <= 0 || (long)C * a.T >= (1L << 31) || a.x_out == a.x_in) return -2;
    const size_t lds = (size_t)(C + PAD_ROWS) * U_LD * sizeof(float);     // 70.7 KB: two workgroups per CU
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(resblock_w43_conv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -3;
        attr_set = true;
    }
    dim3 grid((a.T + FN - 1) / FN, a.B, MS);
    hipLaunchKernelGGL(resblock_w43_conv_kernel, grid, dim3(64 * NWS), lds, stream, a);
    if (hipGetLastError() != hipSuccess) return -3;
    return cmtts_launch_resblock_split_out(ap, stream_);
}
