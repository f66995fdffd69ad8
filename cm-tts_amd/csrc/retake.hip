// Re-taking spans of an utterance: the masked consistency sampler on frame windows (include/cmtts_hip.h: cmtts_retake; DESIGN.md
// §3.6e; cmtts_amd/retake.py is the same definition in numpy).
//
// The sampler is cmtts_sample's loop on a batch of windows [N][Tw] with the KNOWN frames put back after every evaluation:
//   x   = sigma_max * z(draw 0)                                                  every frame of the window   (RETAKE_INIT)
//   x0  = denoise(x, sigma_i); v = regen ? x0 : known;  x = v + (z(1 + i) * nstd_i) * 0.85f              (RETAKE_MID)
//   last evaluation: mel[b][start + t] = x0 (+ the same term when nstd_i >= 0) where regen, nothing else  (RETAKE_LAST)
// The denoiser's kernels are unchanged (its tail writes x0 = c_out F + c_skip x); the three forms above are ONE kernel between
// evaluations, retake_step_kernel.  Its z is the seeded normal at (seed of the row's utterance, draw, start_n + t, m), drawn in
// the kernel with the device functions noise_philox.hip uses (noise_device.h) — a window draws exactly the noise the whole
// utterance would, and no noise tensor is written or read.
//
// This unit is compiled with FP contraction off: v + (z * nstd) * 0.85f is the definition's three roundings.
// Latency / HBM bound: one Philox block = four mel bins per lane, the bin axis on consecutive lanes, 16-byte
// loads and stores when n_mels % 4 == 0 and the tensors are 16-byte aligned, element accesses otherwise.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "retake.h"
#include "noise_device.h"

#pragma clang fp contract(off)

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// grid (chunks, N): the workgroups of one window walk its known rows (one contiguous block of Tw * M floats), its mask bytes, its
// speaker vector and its seed
__global__ __launch_bounds__(256) void retake_gather_kernel(const float* __restrict__ mel, const uint8_t* __restrict__ regen,
                                                            const float* __restrict__ spk, const int64_t* __restrict__ seeds,
                                                            const StreamWindow* __restrict__ win, int T, int Tw, int M, int H,
                                                            float* __restrict__ known_w, uint8_t* __restrict__ regen_w,
                                                            float* __restrict__ spk_w, int64_t* __restrict__ seeds_w) {
    const int n = blockIdx.y;
    const StreamWindow wd = win[n];
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const float* src = mel + ((long)wd.b * T + wd.start) * M;
    float* dst = known_w + (long)n * Tw * M;
    const long nel = (long)Tw * M;
    long i = tid;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const long n4 = nel >> 2;
        for (long q = tid; q < n4; q += stride) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
        i = (n4 << 2) + tid;
    }
    for (; i < nel; i += stride) dst[i] = src[i];
    for (long t = tid; t < Tw; t += stride) {
        const bool core = t >= wd.core_off && t < wd.core_off + wd.core_len;
        regen_w[(long)n * Tw + t] = core && regen[(long)wd.b * T + wd.start + t] ? 1 : 0;
    }
    if (spk)
        for (long h = tid; h < H; h += stride) spk_w[(long)n * H + h] = spk[(long)wd.b * H + h];
    if (tid == 0) seeds_w[n] = seeds[wd.b];
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p, int m, int M) {
    if constexpr (VEC) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], m + 1 < M ? p[1] : 0.f, m + 2 < M ? p[2] : 0.f, m + 3 < M ? p[3] : 0.f);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, float4 v, int m, int M) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x;                       // m < M by construction (q < ceil(M / 4))
        if (m + 1 < M) p[1] = v.y;
        if (m + 2 < M) p[2] = v.z;
        if (m + 3 < M) p[3] = v.w;
    }
}

// grid (ceil(Tw * Q / 256), N), Q = ceil(M / 4): lane = one Philox block = mel bins [4 q, 4 q + 4) of frame t of window n
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void retake_step_kernel(RetakeStepArgs a, int Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;      // Tw * Q < 2^31 (launcher)
    if (i >= (uint32_t)a.Tw * (uint32_t)Q) return;
    const int n = blockIdx.y;
    const int t = (int)(i / (uint32_t)Q), q = (int)(i - (uint32_t)t * (uint32_t)Q);
    const int m = 4 * q, M = a.M;
    const long row = (long)n * a.Tw + t;
    bool regen = false;
    if constexpr (MODE != RETAKE_INIT) {
        regen = a.regen[row] != 0;
        if (MODE == RETAKE_LAST && !regen) return;      // kept frames stay as they are: nothing is added to them
    }
    const StreamWindow wd = a.win[n];
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool draw = MODE != RETAKE_LAST || a.scale >= 0.0f;
    if (draw) {
        const uint64_t j = ((uint64_t)wd.start + (uint64_t)t) * (uint64_t)Q + (uint64_t)q;
        const noise_dev::U4 x = noise_dev::noise_block((uint64_t)a.seeds[n], (uint32_t)a.draw, j);
        const float s = MODE == RETAKE_INIT ? a.scale : 1.0f;      // INIT: the fill kernel's z * sigma_max; else z itself (z * 1.0f)
        noise_dev::box_muller(x.x, x.y, s, z.x, z.y);
        noise_dev::box_muller(x.z, x.w, s, z.z, z.w);
    }
    if constexpr (MODE == RETAKE_INIT) {
        store4<VEC>(a.out + row * M + m, z, m, M);
        return;
    } else {
        const float* src = (MODE == RETAKE_LAST || regen) ? a.x0 : a.known;
        float4 v = load4<VEC>(src + row * M + m, m, M);
        if (draw) {
            const float nstd = a.scale;
            v.x = v.x + (z.x * nstd) * 0.85f;
            v.y = v.y + (z.y * nstd) * 0.85f;
            v.z = v.z + (z.z * nstd) * 0.85f;
            v.w = v.w + (z.w * nstd) * 0.85f;
        }
        float* dst = MODE == RETAKE_LAST ? a.out + ((long)wd.b * a.T + wd.start + t) * M + m : a.out + row * M + m;
        store4<VEC>(dst, v, m, M);
    }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MODE>
void launch_step(const RetakeStepArgs& a, int Q, bool vec, hipStream_t s) {
    const dim3 grid(cdiv((long)a.Tw * Q, 256), a.N);
    if (vec) hipLaunchKernelGGL((retake_step_kernel<true, MODE>), grid, dim3(256), 0, s, a, Q);
    else hipLaunchKernelGGL((retake_step_kernel<false, MODE>), grid, dim3(256), 0, s, a, Q);
}

}  // namespace

extern "C" int cmtts_launch_retake_gather(const float* mel, const uint8_t* regen, const float* spk, const int64_t* seeds, const StreamWindow* win,
                                          int N, int T, int Tw, int M, int H, float* known_w, uint8_t* regen_w, float* spk_w, int64_t* seeds_w,
                                          void* stream) {
    if (N <= 0 || Tw <= 0 || M <= 0) return 0;
    if (N > 65535) return -2;
    const long n4 = ((long)Tw * M + 3) / 4;
    const int chunks = n4 > 256L * 64 ? 64 : cdiv(n4, 256);      // up to 64 workgroups per window; they stride over the rest
    hipLaunchKernelGGL(retake_gather_kernel, dim3(chunks, N), dim3(256), 0, (hipStream_t)stream, mel, regen, spk, seeds, win, T, Tw, M, H, known_w,
                       regen_w, spk_w, seeds_w);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_retake_step(const RetakeStepArgs* a, void* stream) {
    const int Q = (a->M + 3) / 4;
    if (a->N <= 0 || a->Tw <= 0 || a->M <= 0) return 0;
    if (a->N > 65535 || (long)a->Tw * Q > 0x7fffff00L) return -2;
    bool vec = (a->M & 3) == 0 && al16(a->out);
    if (a->mode != RETAKE_INIT) vec = vec && al16(a->x0) && (a->mode == RETAKE_LAST || al16(a->known));
    hipStream_t s = (hipStream_t)stream;
    if (a->mode == RETAKE_INIT) launch_step<RETAKE_INIT>(*a, Q, vec, s);
    else if (a->mode == RETAKE_MID) launch_step<RETAKE_MID>(*a, Q, vec, s);
    else launch_step<RETAKE_LAST>(*a, Q, vec, s);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
