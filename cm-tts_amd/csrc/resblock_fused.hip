// Fused denoiser residual block for gfx950 — ResidualBlock.forward (model/blocks.py:667-686) of the
// CM-TTS consistency denoiser as ONE kernel per layer:
//
//   u  = (x + d [+ p]) + cp            cp = conditioner_projection(cond) + bias, precomputed for all 20
//                                      layers by ONE stacked GEMM (it does not depend on the step)
//   y  = W3 (*) u + b3 ; z = sigmoid(y[:C]) * tanh(y[C:])      conv_layer k=3 pad 1 + gate   (phase B)
//   o  = Wo * z + bo ; x' = (o[:C] + (x + d)) / sqrt(2) ; skip (+)= o[C:]                    (phase C)
//
// One workgroup (16 wave64) owns FN = 64 frames of one utterance; u (with its +-1 frame Conv1D halo)
// and z never leave LDS (z re-uses u's buffer): per layer HBM sees x, cp in and x', skip in/out.
// Both contractions run on v_mfma_f32_32x32x2_f32 (exact fp32) in the same (16-channel chunk, tap, k)
// order as conv_mfma.hip, so the result is BITWISE equal to the three-launch form
// (tests/test_gpu_parity.py::test_fused_resblock_bitwise).
//
// Operand delivery (the part that decides the MFMA duty cycle):
//  * WEIGHTS never touch LDS.  Wave w owns ONE 32-row MFMA tile of the output (rows [32w, +32)) over
//    all 64 frames, and no other wave needs those rows, so they are streamed global/L2 -> VGPR already
//    in MFMA A-fragment order: cmtts_finalize() re-packs each layer as [k-group of 8][m-tile][lane][4]
//    so that ONE coalesced global_load_dwordx4 (1 KB per wave) delivers the A operands of four
//    k-steps = 8 MFMAs.  The measured wall (tools/mfma_probe.hip, profiles/) is the per-CU L2->CU fill
//    rate, ~12 B/clk: a 32-frame tile needs 256 B of weights per MFMA and caps the kernel at ~75 % of
//    the MFMA peak whatever the schedule; 64 frames per workgroup halve that.  A 4-deep register ring
//    keeps three groups in flight; there is no ds_write / wave barrier / LDS double buffering.
//  * The gate needs sigmoid and tanh operands in the same lane: each 32-row tile is packed as
//    [16 sigmoid rows | 16 tanh rows] of the same 16 channels, which the 32x32 C layout puts in
//    registers r and r+8 of one lane.
//  * ACTIVATIONS (u, then z) are read from LDS with conflict-free ds_read_b32 (32 consecutive frames
//    per half-wave), one k-group ahead of the MFMAs that consume them.
//  * 16 waves = 4 per SIMD keep the matrix pipe fed while other waves wait on loads (70 KB LDS,
//    <= 128 VGPRs per wave).
// Three s_barriers per workgroup in total (u staged, u dead, z complete).
#include <hip/hip_runtime.h>
#include "resblock_direct.h"

// The pieces — staging, the k-group stream, gate, epilogue — are resblock_direct.h's, shared with resblock_split.hip and (gate bias,
// epilogue) resblock_fused_lp.hip; this file is their order, the barriers between them and the launcher.
namespace {

using resdirect::C;
constexpr int NW = 16;          // waves per workgroup (one 32-row MFMA tile each)

template <int FN>
__global__ __launch_bounds__(64 * NW, 4) void resblock_fused_kernel(const ResArgs a) {
    static_assert(64 * NW == 1024, "1024-thread workgroups");
    constexpr int NT = FN / 32;         // 32-frame MFMA column tiles per wave
    constexpr int U_LD = FN + 4;        // LDS row stride of u / z (FN + 2 columns used by u)
    extern __shared__ __attribute__((aligned(16))) float u_lds[];   // [C][U_LD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;     // w = this wave's m-tile
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * FN;
    const int T = a.T;

    const int bid_dbg = blockIdx.x + gridDim.x * blockIdx.y;
    auto stamp = [&](int slot) {
        if (a.dbg && tid == 0) a.dbg[(long)bid_dbg * 8 + slot] = (long long)__builtin_readcyclecounter();
    };
    stamp(0);
    resdirect::stage_u<FN, NW>(u_lds, a.x_in + (long)b * C * T, a.cp + (long)b * a.cp_bstride, a.dp + (long)b * a.vec_stride, t0, T, tid);
    __syncthreads();   // (1) u staged
    stamp(1);

    f32x16 acc[NT];
    resdirect::conv_k3(acc, a.W3f, u_lds, w, lane);     // phase B: gated k=3 conv
    stamp(2);
    __syncthreads();   // (2) every wave is done reading u: its buffer becomes z
    stamp(3);
    resdirect::gate(acc, a.b3, w, lane, [&](int j, int ch, float zv) { u_lds[ch * U_LD + j * 32 + (lane & 31)] = zv; });
    __syncthreads();   // (3) z complete
    stamp(4);

    resdirect::project(acc, a.Wof, u_lds, w, lane);     // phase C: output projection
    stamp(5);
    resdirect::epilogue(acc, a, b, t0, w, lane);
    stamp(6);
}

long long* g_dbg = nullptr;
int g_force_fn = 0;

template <int FN>
int launch_fn(const ResArgs& a, hipStream_t stream) {
    static bool attr_set = false;
    const size_t lds = (size_t)(C * (FN + 4)) * sizeof(float);
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(resblock_fused_kernel<FN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -3;
        attr_set = true;
    }
    dim3 grid((a.T + FN - 1) / FN, a.B);
    hipLaunchKernelGGL(resblock_fused_kernel<FN>, grid, dim3(64 * NW), lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" void cmtts_resblock_set_debug(long long* dbg) { g_dbg = dbg; }
extern "C" void cmtts_resblock_set_tile(int frames) { g_force_fn = frames; }

extern "C" int cmtts_launch_resblock(const ResArgs* a_in, void* stream) {
    ResArgs a = *a_in;
    a.dbg = g_dbg;
    // -2 not served: an empty batch, rows beyond the 32-bit element index, x' written over x (neighbouring tiles read its halo)
    if (a.B <= 0 || a.T <= 0 || (long)C * a.T >= (1L << 31) || a.x_out == a.x_in) return -2;
    // 64-frame tiles halve the weight bytes per MFMA (the measured wall); 32-frame tiles only when 64-frame
    // tiles could not even give every CU one workgroup
    const long tiles64 = (long)((a.T + 63) / 64) * a.B;
    const bool use32 = g_force_fn ? g_force_fn == 32 : tiles64 < 256;
    return use32 ? launch_fn<32>(a, (hipStream_t)stream) : launch_fn<64>(a, (hipStream_t)stream);
}
