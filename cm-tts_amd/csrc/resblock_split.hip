// Low-latency form of the denoiser residual block for SMALL batches (a few utterances): the same arithmetic as
// resblock_fused.hip, spread over four times as many CUs.
//
// resblock_fused_kernel<32> gives a 32-frame tile to ONE workgroup of 16 waves: all 16 output m-tiles of the gated conv
// (K = 768) and of the output projection (K = 256) run on one CU, ~55 us of matrix pipe per layer whatever the batch
// (83 us measured) — one 150-frame utterance keeps 5 of 256 CUs busy for 20 x 83 us per evaluation.  Here a tile is cut
// along the OUTPUT ROWS into four workgroups of 4 waves (one wave per SIMD, one m-tile per wave):
//   kernel 1 (conv):  stage u = cp + (x + d [+ p]) for the tile (every workgroup stages all 256 input rows, from L2),
//                     gated k=3 conv for its 4 m-tiles, z -> HBM scratch [B][256][T];
//   kernel 2 (out):   stage z, output projection for its 4 m-tiles, x' / skip epilogue.
// Every wave evaluates the same expressions in the same order as its counterpart in the fused kernel (same fragment
// stream, same (16-channel chunk, tap, k) order, same epilogue expressions; how the compiler schedules them may differ): BITWISE equal
// (tests/test_gpu_parity.py::test_split_resblock_bitwise).  Two launches of ~20 and ~12 us replace one of 83.
// The staging of u, the k-group stream, the gate and the epilogue ARE the fused kernel's: both call resblock_direct.h with the same m-tile
// index.  What is particular to this file is the grid cut, the z staging of the second kernel and the launchers.
#include <hip/hip_runtime.h>
#include "resblock_direct.h"

namespace {

using resdirect::C;
constexpr int FN = 32;          // frames per tile
constexpr int NWS = 4;          // waves per workgroup
constexpr int MS = 4;           // workgroups per tile (4 m-tiles each: 16 m-tiles of 32 rows)
constexpr int U_LD = FN + 4;

__global__ __launch_bounds__(64 * NWS) void resblock_split_conv_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) float u_lds[];     // [C][U_LD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int mt = blockIdx.z * NWS + (tid >> 6);  // this wave's m-tile = wave index of the fused kernel
    const int b = blockIdx.y, t0 = blockIdx.x * FN, T = a.T;
    resdirect::stage_u<FN, NWS>(u_lds, a.x_in + (long)b * C * T, a.cp + (long)b * a.cp_bstride, a.dp + (long)b * a.vec_stride, t0, T, tid);
    __syncthreads();

    f32x16 acc[1];
    resdirect::conv_k3(acc, a.W3f, u_lds, mt, lane);
    float* zb = a.z + (long)b * C * T;
    const int t = t0 + (lane & 31);
    resdirect::gate(acc, a.b3, mt, lane, [&](int, int ch, float zv) {
        if (t < T) zb[(unsigned)(ch * T + t)] = zv;
    });
}

__global__ __launch_bounds__(64 * NWS) void resblock_split_out_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) float z_lds[];     // [C][U_LD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int mt = blockIdx.z * NWS + w;
    const int b = blockIdx.y, t0 = blockIdx.x * FN, T = a.T;
    const int l31 = lane & 31, khalf = lane >> 5;
    const float* zb = a.z + (long)b * C * T;
    {   // stage z[m][n]: columns beyond T are never stored by the epilogue, any finite value will do
        const int t_c = min(t0 + l31, T - 1);
        constexpr int ROWS_PER_WAVE = C / NWS;
#pragma unroll 1
        for (int i = 0; i < ROWS_PER_WAVE / 2; i += 8) {
            float zv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) zv[q] = zb[(unsigned)((w * ROWS_PER_WAVE + (i + q) * 2 + khalf) * T + t_c)];
#pragma unroll
            for (int q = 0; q < 8; ++q) z_lds[(w * ROWS_PER_WAVE + (i + q) * 2 + khalf) * U_LD + l31] = zv[q];
        }
    }
    __syncthreads();

    f32x16 acc[1];
    resdirect::project(acc, a.Wof, z_lds, mt, lane);
    resdirect::epilogue(acc, a, b, t0, mt, lane);
}

}  // namespace

// ResidualBlock.forward as two launches for small batches; needs a->z (scratch [B][256][T]).  0 ok, -2 not served
// (no scratch / shape / x' written over x), -3 HIP error.  The caller decides WHEN (denoiser_side.hip: few 32-frame tiles).
extern "C" int cmtts_launch_resblock_split(const ResArgs* ap, void* stream_) {
    const ResArgs& a = *ap;
    hipStream_t stream = (hipStream_t)stream_;
    if (!a.z || a.B <= 0 || a.T <= 0 || (long)C * a.T >= (1L << 31) || a.x_out == a.x_in) return -2;
    const size_t lds = (size_t)C * U_LD * sizeof(float);
    dim3 grid((a.T + FN - 1) / FN, a.B, MS);
    hipLaunchKernelGGL(resblock_split_conv_kernel, grid, dim3(64 * NWS), lds, stream, a);
    hipLaunchKernelGGL(resblock_split_out_kernel, grid, dim3(64 * NWS), lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The second launch alone, behind another producer of a->z (resblock_split_w43.hip: the persistent stack's F(4,3) conv).
extern "C" int cmtts_launch_resblock_split_out(const ResArgs* ap, void* stream_) {
    const ResArgs& a = *ap;
    hipStream_t stream = (hipStream_t)stream_;
    if (!a.z || a.B <= 0 || a.T <= 0 || (long)C * a.T >= (1L << 31)) return -2;
    const size_t lds = (size_t)C * U_LD * sizeof(float);
    dim3 grid((a.T + FN - 1) / FN, a.B, MS);
    hipLaunchKernelGGL(resblock_split_out_kernel, grid, dim3(64 * NWS), lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
