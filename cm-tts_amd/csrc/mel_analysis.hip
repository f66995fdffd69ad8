// Recorded speech in (include/cmtts_hip.h: cmtts_analysis_*, cmtts_mel_analysis, cmtts_phoneme_energy, cmtts_pcm_crossfade; DESIGN.md §3.5i;
// definition: cmtts_amd/analysis.py).
//
//   mel      STFT + mel + energy in ONE launch, fp32.  A workgroup of four waves owns four consecutive frames of one row.  Frames overlap by 75 %,
//            so the 1792 samples they cover are staged once — converted (int16 / 32768, or float clipped to [-1, 1]) through the reflect index —
//            and each wave then windows ITS frame into LDS as 512 complex points z[n] = x[2n] + i x[2n+1] at bit-reversed positions, runs a
//            512-point radix-2 FFT there (twiddles from the host's table, made in double) and unpicks the real 1024-point spectrum with the split
//            step X[k] = E[k] + W^k O[k], X[512 - k] = conj(E[k] - W^k O[k]).  Magnitudes go to LDS; the energy is a lane-strided sum (bins
//            ascending per lane) closed by a fixed shuffle tree; the filterbank is applied as sparse triangles, one lane per filter, bins ascending
//            (a bin feeds at most two filters: 1026 weights against 41040 of the dense product).  No atomics.  A frame's arithmetic depends on its
//            samples alone: not on the wave that ran it, its row or the launch.
//   energy   per row an exclusive scan of the durations (integer), per phoneme the mean of its frames, frames ascending, in double, then
//            (e - mean) / std rounded to float once.
//   fade     one thread per sample of a vocoded window row: the core is the vocoded sample, the X margin frames a linear fade between the
//            recording and it, every other sample the recording's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "launch.h"
#include "mel_analysis.h"
#include "model.h"

namespace {

constexpr int MEL_THREADS = 64 * MEL_FPB;
constexpr int MEL_STAGE = MEL_NFFT + (MEL_FPB - 1) * MEL_HOP;        // samples four consecutive frames cover
constexpr int MEL_HALF = MEL_NFFT / 2;                               // points of the complex FFT
constexpr int MEL_MAG_LD = MEL_BINS + 3;
constexpr float MEL_FLOOR = 1e-5f;
constexpr float MEL_LOG_FLOOR = -11.512925464970229f;                // log(1e-5), rounded once: what a clamped cell holds

__device__ __forceinline__ int mel_frames_of(int n, int pad, int T) {
    if (n <= pad) return 0;
    const int f = pad == MEL_NFFT / 2 ? 1 + n / MEL_HOP : n / MEL_HOP;
    return min(f, T);
}

template <bool I16>
__global__ __launch_bounds__(MEL_THREADS) void mel_analysis_kernel(const MelTables t, const void* __restrict__ wav, long ld,
                                                                   const int32_t* __restrict__ n_valid, int pad, int T, int layout,
                                                                   float* __restrict__ mel, float* __restrict__ energy, int32_t* __restrict__ frames) {
    __shared__ float smp[MEL_STAGE];
    __shared__ float2 z[MEL_FPB][MEL_HALF];
    __shared__ float mag[MEL_FPB][MEL_MAG_LD];
    __shared__ float2 tw[MEL_HALF];
    __shared__ float pk[MEL_NNZ_MAX];
    __shared__ int32_t ftab[3 * MEL_CH];
    __shared__ float melo[MEL_FPB][MEL_CH];
    __shared__ float en[MEL_FPB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.y, f0 = blockIdx.x * MEL_FPB;
    const long nv = n_valid[row];
    const int n = (int)(nv < 0 ? 0 : (nv > ld ? ld : nv));
    const int F = mel_frames_of(n, pad, T);
    if (blockIdx.x == 0 && tid == 0) frames[row] = F;

    if (f0 < F) {                                             // uniform per workgroup
        for (int j = tid; j < MEL_STAGE; j += MEL_THREADS) {
            int i = f0 * MEL_HOP + j - pad;
            if (i < 0) i = -i;
            if (i >= n) i = 2 * (n - 1) - i;
            i = min(max(i, 0), n - 1);                        // a frame at or beyond F of this group: its samples are staged, never used
            float v;
            if (I16) v = (float)reinterpret_cast<const int16_t*>(wav)[row * ld + i] * (1.0f / 32768.0f);
            else v = fminf(fmaxf(reinterpret_cast<const float*>(wav)[row * ld + i], -1.0f), 1.0f);
            smp[j] = v;
        }
        for (int j = tid; j < MEL_HALF; j += MEL_THREADS) tw[j] = reinterpret_cast<const float2*>(t.twiddle)[j];
        for (int j = tid; j < t.nnz; j += MEL_THREADS) pk[j] = t.pack[j];
        for (int j = tid; j < 3 * MEL_CH; j += MEL_THREADS) ftab[j] = t.tab[j];
        __syncthreads();

        // this wave's frame, windowed, at bit-reversed positions
        const float* s = smp + w * MEL_HOP;
        float2* zz = z[w];
        for (int k = lane; k < MEL_HALF; k += 64) {
            const float2 wn = reinterpret_cast<const float2*>(t.window)[k];
            zz[__brev((unsigned)k) >> 23] = make_float2(wn.x * s[2 * k], wn.y * s[2 * k + 1]);
        }
        __syncthreads();
        for (int half = 1; half < MEL_HALF; half <<= 1) {
            const int tstep = MEL_NFFT / 2 / half;            // W_512^(pos * 256 / half) = tw[pos * 512 / half]
            for (int b = lane; b < MEL_HALF / 2; b += 64) {
                const int pos = b & (half - 1);
                const int i0 = ((b - pos) << 1) + pos, i1 = i0 + half;
                const float2 c = tw[pos * tstep];
                const float2 x = zz[i1], a = zz[i0];
                const float tr = c.x * x.x - c.y * x.y, ti = c.x * x.y + c.y * x.x;
                zz[i0] = make_float2(a.x + tr, a.y + ti);
                zz[i1] = make_float2(a.x - tr, a.y - ti);
            }
            __syncthreads();
        }
        // split step: bins k and 512 - k from Z[k] and Z[512 - k] (Z[512] = Z[0])
        for (int k = lane; k <= MEL_HALF / 2; k += 64) {
            const float2 a = zz[k], b = zz[(MEL_HALF - k) & (MEL_HALF - 1)];
            const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);          // E = (A + conj B) / 2
            const float orr = 0.5f * (a.y + b.y), oi = 0.5f * (b.x - a.x);         // O = -i (A - conj B) / 2
            const float2 c = tw[k];
            const float pr = c.x * orr - c.y * oi, pi = c.x * oi + c.y * orr;      // W^k O
            const float xr = er + pr, xi = ei + pi, yr = er - pr, yi = ei - pi;
            mag[w][k] = sqrtf(xr * xr + xi * xi);
            mag[w][MEL_HALF - k] = sqrtf(yr * yr + yi * yi);
        }
        __syncthreads();
        {
            float e = 0.f;
            for (int k = lane; k < MEL_HALF; k += 64) e += mag[w][k] * mag[w][k];
            if (lane == 0) e += mag[w][MEL_HALF] * mag[w][MEL_HALF];
            for (int d = 32; d; d >>= 1) e += __shfl_down(e, d);
            if (lane == 0) en[w] = sqrtf(e);
        }
        for (int m = lane; m < MEL_CH; m += 64) {
            const int off = ftab[3 * m], lo = ftab[3 * m + 1], cnt = ftab[3 * m + 2];
            float acc = 0.f;
            for (int i = 0; i < cnt; ++i) acc = fmaf(pk[off + i], mag[w][lo + i], acc);
            melo[w][m] = acc > MEL_FLOOR ? logf(acc) : MEL_LOG_FLOOR;
        }
        __syncthreads();
    }

    // the group's cells: what was computed for frames below F, zeros from there on
    for (int idx = tid; idx < MEL_FPB * MEL_CH; idx += MEL_THREADS) {
        const int fw = layout == 0 ? idx / MEL_CH : idx % MEL_FPB, m = layout == 0 ? idx % MEL_CH : idx / MEL_FPB;
        const int f = f0 + fw;
        if (f >= T) continue;
        const float v = f < F ? melo[fw][m] : 0.f;
        if (layout == 0) mel[((long)row * T + f) * MEL_CH + m] = v;
        else mel[((long)row * MEL_CH + m) * T + f] = v;
    }
    if (tid < MEL_FPB && f0 + tid < T) energy[(long)row * T + f0 + tid] = f0 + tid < F ? en[tid] : 0.f;
}

// ---- phoneme energy --------------------------------------------------------------------------------------------------------------------
constexpr int PE_THREADS = 256;

__global__ __launch_bounds__(PE_THREADS) void phoneme_energy_kernel(const float* __restrict__ energy, int T, const int32_t* __restrict__ durations,
                                                                    int L, double mean, double std, float* __restrict__ out) {
    __shared__ long long tot[PE_THREADS];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int32_t* d = durations + (long)row * L;
    const int run = (L + PE_THREADS - 1) / PE_THREADS;
    const int l0 = min(tid * run, L), l1 = min(l0 + run, L);
    long long s = 0;
    for (int l = l0; l < l1; ++l) s += max(d[l], 0);
    tot[tid] = s;
    __syncthreads();
    for (int step = 1; step < PE_THREADS; step <<= 1) {       // inclusive scan of the runs' totals (integers: any order)
        const long long add = tid >= step ? tot[tid - step] : 0;
        __syncthreads();
        tot[tid] += add;
        __syncthreads();
    }
    long long pos = tot[tid] - s;
    const float* e = energy + (long)row * T;
    for (int l = l0; l < l1; ++l) {
        const int n = max(d[l], 0);
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const long long fr = pos + i;
            if (fr >= T) break;                               // frames at or beyond T count as zero
            acc += (double)e[fr];
        }
        const double m = n > 0 ? acc / (double)n : 0.0;
        out[(long)row * L + l] = (float)((m - mean) / std);
        pos += n;
    }
}

// ---- crossfade -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int16_t to_pcm16(float v) { return (int16_t)(int)fminf(fmaxf(rintf(v), -32768.0f), 32767.0f); }

__global__ __launch_bounds__(256) void pcm_crossfade_kernel(const float* __restrict__ wav_rows, const int16_t* __restrict__ rec_rows,
                                                            const int32_t* __restrict__ table, int core, int X, int hop,
                                                            int16_t* __restrict__ out_rows) {
    const int n = blockIdx.y;
    const long rowlen = (long)(core + 2 * X) * hop;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= rowlen) return;
    const int lead = min(max(table[4 * n], 0), X), len = min(max(table[4 * n + 1], 0), core), trail = min(max(table[4 * n + 2], 0), X);
    const int fades = table[4 * n + 3];
    const long o = n * rowlen + j;
    const int16_t r = rec_rows[o];
    const float v = wav_rows[o] * 32768.0f, rf = (float)r;
    const long a = (long)lead * hop, b = a + (long)len * hop, c = b + (long)trail * hop;
    const float span = (float)((long)X * hop);
    int16_t y = r;
    if (j < a) {
        if ((fades & 1) && lead == X) y = to_pcm16(rf + (((float)j + 0.5f) / span) * (v - rf));
    } else if (j < b) {
        y = to_pcm16(v);
    } else if (j < c) {
        if ((fades & 2) && trail == X) y = to_pcm16(rf + (((float)(c - 1 - j) + 0.5f) / span) * (v - rf));
    }
    out_rows[o] = y;
}

}  // namespace

extern "C" int cmtts_launch_mel_analysis(const MelTables* t, const void* wav, int is_int16, long ld, int rows, const int32_t* n_valid, int pad, int T,
                                         int layout, float* mel, float* energy, int32_t* frames, void* stream) {
    if (rows < 1 || rows > 65535 || ld < 1 || ld > INT32_MAX / 2 || T < 1 || T > (1 << 22) || (pad != MEL_NFFT / 2 && pad != (MEL_NFFT - MEL_HOP) / 2) ||
        (layout != 0 && layout != 1) || t->nnz < 0 || t->nnz > MEL_NNZ_MAX)
        return -2;
    const dim3 grid((T + MEL_FPB - 1) / MEL_FPB, rows);
    if (is_int16)
        hipLaunchKernelGGL(mel_analysis_kernel<true>, grid, dim3(MEL_THREADS), 0, (hipStream_t)stream, *t, wav, ld, n_valid, pad, T, layout, mel, energy, frames);
    else
        hipLaunchKernelGGL(mel_analysis_kernel<false>, grid, dim3(MEL_THREADS), 0, (hipStream_t)stream, *t, wav, ld, n_valid, pad, T, layout, mel, energy, frames);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_phoneme_energy(const float* energy, int B, int T, const int32_t* durations, int L, double mean, double std, float* out,
                                           void* stream) {
    if (B < 1 || B > 65535 || T < 1 || L < 1) return -2;
    hipLaunchKernelGGL(phoneme_energy_kernel, dim3(B), dim3(PE_THREADS), 0, (hipStream_t)stream, energy, T, durations, L, mean, std, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_pcm_crossfade(const float* wav_rows, const int16_t* rec_rows, const int32_t* table, int N, int core, int X, int hop,
                                          int16_t* out_rows, void* stream) {
    if (N < 1 || N > 65535 || core < 1 || X < 0 || hop < 1 || (long)(core + 2L * X) * hop > INT32_MAX) return -2;
    const long rowlen = (long)(core + 2 * X) * hop;
    hipLaunchKernelGGL(pcm_crossfade_kernel, dim3((unsigned)((rowlen + 255) / 256), N), dim3(256), 0, (hipStream_t)stream, wav_rows, rec_rows, table,
                       core, X, hop, out_rows);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the handle and the C ABI ------------------------------------------------------------------------------------------------------------
struct cmtts_analysis {
    Allocs al;
    MelTables t{};
};

extern "C" {

int cmtts_mel_basis(int fs, int n_fft, int n_mels, double fmin, double fmax, float* out) {
    if (n_fft % 2 || mel_basis(fs, n_fft, n_mels, fmin, fmax, out) != 0)       // the entry point stays even-only; mel_basis() itself takes the GE2E front end's odd 551
        return fail(CMTTS_E_INVALID, "cmtts_mel_basis: null out, or outside fs >= 1, even 2 <= n_fft <= 65536, 1 <= n_mels <= 1024, 0 <= fmin < fmax <= fs / 2");
    return 0;
}

static int analysis_geometry(const std::string& who, int fs, int filter_length, int hop_length, int win_length, int n_mels, double fmin, double fmax) {
    if (filter_length != MEL_NFFT || hop_length != MEL_HOP || win_length != MEL_NFFT || n_mels != MEL_CH)
        return fail(CMTTS_E_INVALID, who + ": unsupported geometry (only filter_length = win_length = 1024, hop_length = 256, 80 mel channels)");
    if (fs < MEL_MIN_RATE || fs > MEL_MAX_RATE || !(fmin >= 0.0) || !(fmin < fmax) || !(fmax <= fs / 2.0))
        return fail(CMTTS_E_INVALID, who + ": 8000 <= fs <= 48000 and 0 <= fmin < fmax <= fs / 2");
    return 0;
}

int cmtts_analysis_create(int fs, int filter_length, int hop_length, int win_length, int n_mels, double fmin, double fmax, cmtts_analysis** out) {
    const std::string who = "cmtts_analysis_create";
    if (!out) return fail(CMTTS_E_INVALID, who + ": null argument");
    CHK(analysis_geometry(who, fs, filter_length, hop_length, win_length, n_mels, fmin, fmax));
    std::vector<float> basis((size_t)MEL_CH * MEL_BINS), pack(MEL_NNZ_MAX), window(MEL_NFFT), twiddle(MEL_NFFT);
    std::vector<int32_t> tab(3 * MEL_CH);
    if (mel_basis(fs, MEL_NFFT, MEL_CH, fmin, fmax, basis.data()) != 0) return fail(CMTTS_E_INVALID, who + ": no filterbank for these arguments");
    const int nnz = mel_sparse_rows(basis.data(), pack.data(), tab.data());
    if (nnz < 0) return fail(CMTTS_E_INVALID, who + ": the filterbank does not fit the sparse form");
    mel_window(window.data());
    mel_twiddles(twiddle.data());
    cmtts_analysis* a = new cmtts_analysis();
    auto up = [&](const void* h, size_t bytes, const void** dst) { return a->al.upload_bytes(h, bytes, (void**)dst); };
    int rc = up(window.data(), window.size() * sizeof(float), (const void**)&a->t.window);
    if (rc == 0) rc = up(twiddle.data(), twiddle.size() * sizeof(float), (const void**)&a->t.twiddle);
    if (rc == 0) rc = up(pack.data(), pack.size() * sizeof(float), (const void**)&a->t.pack);
    if (rc == 0) rc = up(tab.data(), tab.size() * sizeof(int32_t), (const void**)&a->t.tab);
    if (rc != 0) {
        a->al.release();
        delete a;
        return rc;
    }
    a->t.nnz = nnz;
    *out = a;
    return 0;
}

void cmtts_analysis_destroy(cmtts_analysis* a) {
    if (!a) return;
    a->al.release();
    delete a;
}

size_t cmtts_analysis_workspace_bytes(int rows, int T) {
    if (rows < 1 || rows > 65535 || T < 1 || T > (1 << 22)) return 0;
    return 256;          // the one-launch form keeps everything in LDS: one slice, reserved, so that callers have one protocol
}

int cmtts_mel_analysis(cmtts_analysis* a, const void* wav, int is_int16, int rows, int64_t ld, const int32_t* n_valid, int pad_mode, int T, int layout,
                       float* mel, float* energy, int32_t* frames, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_mel_analysis";
    if (!a || !wav || !n_valid || !mel || !energy || !frames) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (rows < 1 || rows > 65535 || ld < 1 || ld > INT32_MAX / 2) return fail(CMTTS_E_INVALID, who + ": 1 <= rows <= 65535 and 1 <= ld < 2^30");
    if (T < 1 || T > (1 << 22)) return fail(CMTTS_E_INVALID, who + ": 1 <= T <= 2^22");
    if (pad_mode != CMTTS_PAD_REFERENCE && pad_mode != CMTTS_PAD_VOCODER) return fail(CMTTS_E_INVALID, who + ": pad_mode must be CMTTS_PAD_REFERENCE or CMTTS_PAD_VOCODER");
    if (layout != CMTTS_MEL_TC && layout != CMTTS_MEL_CT) return fail(CMTTS_E_INVALID, who + ": layout must be CMTTS_MEL_TC or CMTTS_MEL_CT");
    if (!ws || ws_bytes < cmtts_analysis_workspace_bytes(rows, T)) return fail(CMTTS_E_WORKSPACE, who + ": workspace too small");
    const int pad = pad_mode == CMTTS_PAD_REFERENCE ? MEL_NFFT / 2 : (MEL_NFFT - MEL_HOP) / 2;
    if (cmtts_launch_mel_analysis(&a->t, wav, is_int16 != 0, (long)ld, rows, n_valid, pad, T, layout, mel, energy, frames, stream) != 0)
        return fail(CMTTS_E_HIP, "mel analysis launch failed");
    return 0;
}

int cmtts_phoneme_energy(const float* energy, int B, int T, const int32_t* durations, int L, double mean, double std, float* out, void* stream) {
    const std::string who = "cmtts_phoneme_energy";
    if (!energy || !durations || !out) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (B < 1 || B > 65535 || T < 1 || L < 1) return fail(CMTTS_E_INVALID, who + ": 1 <= B <= 65535, T >= 1, L >= 1");
    if (!(std > 0.0) || !(mean == mean)) return fail(CMTTS_E_INVALID, who + ": std must be positive, mean a number");
    if (cmtts_launch_phoneme_energy(energy, B, T, durations, L, mean, std, out, stream) != 0) return fail(CMTTS_E_HIP, "phoneme energy launch failed");
    return 0;
}

int cmtts_pcm_crossfade(const float* wav_rows, const int16_t* rec_rows, const int32_t* table, int N, int core, int xfade_frames, int hop, int16_t* out_rows,
                        void* stream) {
    const std::string who = "cmtts_pcm_crossfade";
    if (!wav_rows || !rec_rows || !table || !out_rows) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (N < 1 || N > 65535 || core < 1 || xfade_frames < 0 || hop < 1 || (core + 2L * xfade_frames) * hop > INT32_MAX)
        return fail(CMTTS_E_INVALID, who + ": 1 <= N <= 65535, core >= 1, xfade_frames >= 0, hop >= 1, (core + 2 xfade_frames) hop < 2^31");
    if (cmtts_launch_pcm_crossfade(wav_rows, rec_rows, table, N, core, xfade_frames, hop, out_rows, stream) != 0)
        return fail(CMTTS_E_HIP, "pcm crossfade launch failed");
    return 0;
}

}  // extern "C"
