// GE2E speaker embeddings from reference audio (include/cmtts_hip.h: cmtts_ge2e_*; definition: cmtts_amd/ge2e.py).
//
//   mel      one workgroup per (window slot, 16 frames): the frames gathered with numpy's reflect rule into LDS, the 551-point DFT as a contraction
//            on v_mfma_f32_16x16x4_f32 — A = the windowed cos / sin table (16 bins x 4 samples, made in double on the host, L2 resident),
//            B = the frames (4 samples x 16 frames) — so a lane's cos and sin results are the same (bin, frame): power in the lane, then the 40
//            sparse triangle sums, bins ascending.  551 = 19 x 29 has no radix-2 form; the contraction is exact and 0.6 MFLOP per frame.
//   inproj   pre [N T][1024] = x W_ih^T + (b_ih + b_hh): A = W_ih fragments over PACKED gate rows, B = 16 frames; a lane stores four consecutive
//            packed rows of one frame.
//   lstm     one workgroup of 16 waves owns a tile of 16 windows from frame 0 to the last; no workgroup waits on another.  Wave g owns
//            hidden units 16 g .. 16 g + 15: its four 16-row MFMA tiles are their i, f, g, o rows (weight_pack.h: to_lstm_fragments), so the
//            cell runs in the lane that holds the gates; c and h live in registers, h of the tile in LDS as the next step's B operand.  W_hh
//            (1 MB) streams from L2 every step through a four-chunk register ring that runs on across steps.  The accumulators start at
//            pre[t], k ascends: the order is a function of the shape alone.  Cell: 1 / (1 + expf(-x)) and tanhf, the accurate library forms.
//   tail     Linear 256 -> 256 + ReLU + x / (norm + 1e-5) per window; mean of a row's windows in window order / its norm (no epsilon).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "ge2e.h"
#include "internal_hooks.h"
#include "launch.h"
#include "mel_analysis.h"
#include "model.h"
#include "weight_pack.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- mel ----------------------------------------------------------------------------------------------------------------------------
constexpr int FE_THREADS = 256;
constexpr int FE_FRAMES = 16;                                 // frames per workgroup: one MFMA column tile
constexpr int FE_KPAD = GE2E_KCHUNKS * 16;                    // 560
constexpr int FE_STRIDE = FE_KPAD + 4;                        // LDS row stride of a frame (floats)
constexpr int FE_BSTRIDE = GE2E_PAIRS * 16 + 4;               // LDS row stride of a frame's power spectrum

__global__ __launch_bounds__(FE_THREADS) void ge2e_mel_kernel(const float* __restrict__ wav, long ld, const int32_t* __restrict__ n_valid, int mode,
                                                              int max_windows, int T, const Ge2eTables tb, float* __restrict__ windows,
                                                              int32_t* __restrict__ win_lens, int32_t* __restrict__ info) {
    __shared__ float fr[FE_FRAMES][FE_STRIDE];
    __shared__ float pw[FE_FRAMES][FE_BSTRIDE];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, tile = blockIdx.x;
    const int row = blockIdx.y / max_windows, j = blockIdx.y - row * max_windows;
    auto valid = [&](int r) {
        const long nv = n_valid[r];
        return (int)(nv < 0 ? 0 : (nv > ld ? ld : nv));
    };
    const int n = valid(row);
    const Ge2eCounts cnt = ge2e_counts(n, mode, max_windows);
    if (tile == 0 && j == 0 && tid == 0) {
        info[4 * row] = n;
        info[4 * row + 1] = cnt.n_eff;
        info[4 * row + 2] = cnt.frames;
        info[4 * row + 3] = cnt.nwin;
    }
    if (j >= cnt.nwin) return;                                // uniform per workgroup
    // windows of the rows before this one (integer sum: any order)
    if (tid == 0) base_s = 0;
    __syncthreads();
    int before = 0;
    for (int r = tid; r < row; r += FE_THREADS) before += ge2e_counts(valid(r), mode, max_windows).nwin;
    if (before) atomicAdd(&base_s, before);
    __syncthreads();
    const int w = base_s + j;
    const int Tw = mode == 1 ? GE2E_FRAMES : T;
    const int wl = mode == 1 ? GE2E_FRAMES : min(cnt.frames, T);
    const int f0 = mode == 1 ? GE2E_WHOP * j : 0;
    if (tile == 0 && tid == 0) win_lens[w] = wl;

    // the frames: sample s = 220 f - 275 + u of the zero-padded row, reflected about 0 and n_eff - 1 as numpy.pad does (repeatedly for a short row)
    const float* x = wav + (long)row * ld;
    const long period = 2L * (cnt.n_eff - 1);
    for (int idx = tid; idx < FE_FRAMES * FE_KPAD; idx += FE_THREADS) {
        const int i = idx / FE_KPAD, u = idx - i * FE_KPAD;
        const int t = FE_FRAMES * tile + i;
        float v = 0.f;
        if (u < GE2E_NFFT && t < wl) {
            long s = (long)(f0 + t) * GE2E_HOP - GE2E_PAD + u;
            if (period > 0) {
                s %= period;
                if (s < 0) s += period;
                if (s >= cnt.n_eff) s = period - s;
            } else {
                s = 0;
            }
            if (s < n) v = x[s];                              // [n, n_eff): the zero padding; what the row holds there is not read
        }
        fr[i][u] = v;
    }
    __syncthreads();

    // re, im of 16 bins x 16 frames per tile pair; two accumulation chains each (even and odd chunks)
    const int pl = lane & 15, kk = lane >> 4;
    const f32x4* dft = reinterpret_cast<const f32x4*>(tb.dft);
    for (int p = wid; p < GE2E_PAIRS; p += FE_THREADS / 64) {
        f32x4 re[2], im[2];
        re[0] = re[1] = im[0] = im[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4* a = dft + (long)p * GE2E_KCHUNKS * 2 * 64 + lane;
#pragma unroll 2
        for (int c = 0; c < GE2E_KCHUNKS - 1; c += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 ac = a[(c + h) * 128], as = a[(c + h) * 128 + 64];
                const f32x4 b = *reinterpret_cast<const f32x4*>(&fr[pl][16 * (c + h) + 4 * kk]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    re[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[q], b[q], re[h], 0, 0, 0);
                    im[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[q], b[q], im[h], 0, 0, 0);
                }
            }
        }
        {
            constexpr int c = GE2E_KCHUNKS - 1;
            const f32x4 ac = a[c * 128], as = a[c * 128 + 64];
            const f32x4 b = *reinterpret_cast<const f32x4*>(&fr[pl][16 * c + 4 * kk]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                re[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[q], b[q], re[0], 0, 0, 0);
                im[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[q], b[q], im[0], 0, 0, 0);
            }
        }
        // lane: frame pl, bins 16 p + 4 kk .. + 3
        f32x4 pwv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a_re = re[0][r] + re[1][r], a_im = im[0][r] + im[1][r];
            pwv[r] = a_re * a_re + a_im * a_im;
        }
        *reinterpret_cast<f32x4*>(&pw[pl][16 * p + 4 * kk]) = pwv;
    }
    __syncthreads();

    float* out = windows + ((long)w * Tw + FE_FRAMES * tile) * GE2E_MELS;
    for (int o = tid; o < FE_FRAMES * GE2E_MELS; o += FE_THREADS) {
        const int i = o / GE2E_MELS, m = o - i * GE2E_MELS;
        if (FE_FRAMES * tile + i >= Tw) break;
        const int off = tb.tab[3 * m], lo = tb.tab[3 * m + 1], nb = tb.tab[3 * m + 2];
        float acc = 0.f;
        for (int q = 0; q < nb; ++q) acc = fmaf(tb.pack[off + q], pw[i][lo + q], acc);
        out[o] = acc;                                         // frames at and beyond wl were staged as zeros
    }
}

// ---- inproj -------------------------------------------------------------------------------------------------------------------------
// grid (ceil(R / 32), 4): wave = 64 packed gate rows (4 row tiles) x 32 frames (2 column tiles)
__global__ __launch_bounds__(256) void ge2e_inproj_kernel(const float* __restrict__ x, long R, int K, const float* __restrict__ wf,
                                                          const float* __restrict__ bias, float* __restrict__ pre) {
    constexpr int MT = 4, NT = 2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int pl = lane & 15, kk = lane >> 4;
    const int g = blockIdx.y * 4 + wid;                       // 16 groups of 64 packed rows
    const long r0 = (long)blockIdx.x * (16 * NT);
    const int nchunk = (K + 15) / 16;
    const f32x4* wfrag = reinterpret_cast<const f32x4*>(wf) + (long)(MT * g) * 64 + lane;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(bias + 64 * g + 16 * mi + 4 * kk);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = b;
    }
    f32x4 wv[2][MT], xv[2][NT];
    // loads are unconditional from a clamped, always valid address; the select follows (k beyond K: zero, whatever the next row holds)
    auto load = [&](int c, f32x4* w, f32x4* xx) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) w[mi] = wfrag[((long)c * 64 + mi) * 64];
        const int k0 = 16 * c + 4 * kk;
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            const long r = r0 + 16 * ni + pl;
            const bool ok = r < R && k0 < K;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (ok ? r * K + k0 : 0));
            xx[ni] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    load(0, wv[0], xv[0]);
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) load(c + 1, wv[cur ^ 1], xv[cur ^ 1]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[cur][mi][q], xv[cur][ni][q], acc[mi][ni], 0, 0, 0);
    }
    // lane: frame r0 + 16 ni + pl, packed rows 64 g + 16 mi + 4 kk .. + 3
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        const long r = r0 + 16 * ni + pl;
        if (r >= R) continue;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) *reinterpret_cast<f32x4*>(pre + r * GE2E_GATES + 64 * g + 16 * mi + 4 * kk) = acc[mi][ni];
    }
}

// ---- lstm ---------------------------------------------------------------------------------------------------------------------------
constexpr int LSTM_THREADS = 1024;                            // 16 waves: one per 16 hidden units
constexpr int LSTM_HSTRIDE = GE2E_HID + 4;                    // LDS row stride of a window's h
constexpr int LSTM_RING = 4, LSTM_CHUNKS = GE2E_HID / 16;     // 16 chunks of 16 k

__device__ __forceinline__ float sigmoid_acc(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int NT>
__global__ __launch_bounds__(LSTM_THREADS) void ge2e_lstm_kernel(const float* __restrict__ pre, const float* __restrict__ whf,
                                                                 const int32_t* __restrict__ lens, int N, int T, float* __restrict__ hseq,
                                                                 float* __restrict__ hlast) {
    __shared__ float hs[16 * NT][LSTM_HSTRIDE];
    const int tid = threadIdx.x, lane = tid & 63, ug = tid >> 6;
    const int pl = lane & 15, kk = lane >> 4;
    const int w0 = blockIdx.x * 16 * NT;

    // this lane's windows, their lengths, and the tile's longest
    int len[NT];
    long wbase[NT];
    bool wv_ok[NT];
    int tmax = 0;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        const int w = w0 + 16 * ni + pl;
        wv_ok[ni] = w < N;
        const int l = wv_ok[ni] ? (lens ? min(max(lens[w], 0), T) : T) : 0;
        len[ni] = l;
        wbase[ni] = (long)(wv_ok[ni] ? w : N - 1) * T;         // a clamped, always valid address for the loads
    }
    for (int i = 0; i < 16 * NT; ++i) {
        const int w = w0 + i;
        if (w < N) tmax = max(tmax, lens ? min(max(lens[w], 0), T) : T);
    }
    for (int i = tid; i < 16 * NT * LSTM_HSTRIDE; i += LSTM_THREADS) (&hs[0][0])[i] = 0.f;

    f32x4 c[NT], h[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) c[ni] = h[ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    // W_hh: chunk ch, row tiles 4 ug .. 4 ug + 3; the ring runs on across steps (chunk 16 = chunk 0 of the next step)
    const f32x4* wfrag = reinterpret_cast<const f32x4*>(whf) + (long)(4 * ug) * 64 + lane;
    f32x4 ring[LSTM_RING][4];
    auto wload = [&](int ch, f32x4* dst) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) dst[mi] = wfrag[((long)ch * 64 + mi) * 64];
    };
    const int col = 64 * ug + 4 * kk;                        // + 16 gate: this lane's packed rows
    auto pload = [&](int t, f32x4 (*dst)[NT]) {
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) dst[mi][ni] = *reinterpret_cast<const f32x4*>(pre + (wbase[ni] + t) * GE2E_GATES + col + 16 * mi);
    };
    f32x4 acc[4][NT], nxt[4][NT];
    if (tmax > 0) {
        pload(0, nxt);
#pragma unroll
        for (int s = 0; s < LSTM_RING - 1; ++s) wload(s, ring[s]);
    }
    __syncthreads();

    for (int t = 0; t < tmax; ++t) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = nxt[mi][ni];
        if (t + 1 < tmax) pload(t + 1, nxt);
        // rolled over groups of LSTM_RING chunks (the ring slots stay compile-time registers; unrolled further, the loads of all 16 chunks are
        // hoisted and spill)
#pragma unroll 1
        for (int c0 = 0; c0 < LSTM_CHUNKS; c0 += LSTM_RING) {
#pragma unroll
            for (int sl = 0; sl < LSTM_RING; ++sl) {
                const int ch = c0 + sl;
                wload((ch + LSTM_RING - 1) % LSTM_CHUNKS, ring[(sl + LSTM_RING - 1) % LSTM_RING]);
                f32x4 hv[NT];
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) hv[ni] = *reinterpret_cast<const f32x4*>(&hs[16 * ni + pl][16 * ch + 4 * kk]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NT; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(ring[sl][mi][q], hv[ni][q], acc[mi][ni], 0, 0, 0);
            }
        }
        __syncthreads();                                      // every wave has read h[t - 1]
        // the cell, in the lane that holds i, f, g, o of (units 16 ug + 4 kk .. + 3, window pl)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            const bool live = t < len[ni];                    // beyond its length a window keeps its state: a select, so what pre holds there does not matter
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ig = sigmoid_acc(acc[0][ni][r]), fg = sigmoid_acc(acc[1][ni][r]);
                const float gg = tanhf(acc[2][ni][r]), og = sigmoid_acc(acc[3][ni][r]);
                const float cn = fg * c[ni][r] + ig * gg;
                const float hn = og * tanhf(cn);
                c[ni][r] = live ? cn : c[ni][r];
                h[ni][r] = live ? hn : h[ni][r];
            }
            *reinterpret_cast<f32x4*>(&hs[16 * ni + pl][16 * ug + 4 * kk]) = h[ni];
            if (wv_ok[ni]) *reinterpret_cast<f32x4*>(hseq + (wbase[ni] + t) * GE2E_HID + 16 * ug + 4 * kk) = h[ni];
        }
        __syncthreads();
    }
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
        if (wv_ok[ni]) *reinterpret_cast<f32x4*>(hlast + (long)(w0 + 16 * ni + pl) * GE2E_HID + 16 * ug + 4 * kk) = h[ni];
}

// ---- tail ---------------------------------------------------------------------------------------------------------------------------
constexpr int TAIL_THREADS = GE2E_EMB;

// every lane returns the sum of the workgroup's values, combined in a fixed tree
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int d = TAIL_THREADS / 2; d; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    const float s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(TAIL_THREADS) void ge2e_proj_kernel(const float* __restrict__ hlast, const float* __restrict__ lin_t,
                                                                 const float* __restrict__ lin_b, float* __restrict__ emb_w) {
    __shared__ float v[GE2E_HID];
    __shared__ float red[TAIL_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    v[tid] = hlast[(long)w * GE2E_HID + tid];
    __syncthreads();
    float acc = 0.f;
    for (int k = 0; k < GE2E_HID; ++k) acc = fmaf(v[k], lin_t[(long)k * GE2E_EMB + tid], acc);
    acc = fmaxf(acc + lin_b[tid], 0.f);
    const float ss = block_sum(acc * acc, red);
    emb_w[(long)w * GE2E_EMB + tid] = acc / (sqrtf(ss) + 1e-5f);
}

__global__ __launch_bounds__(TAIL_THREADS) void ge2e_rows_kernel(const float* __restrict__ emb_w, int W, const int32_t* __restrict__ row_map,
                                                                 float* __restrict__ emb) {
    __shared__ float red[TAIL_THREADS];
    const int row = blockIdx.x, tid = threadIdx.x;
    float acc = 0.f;
    int cnt = 0;
    for (int w = 0; w < W; ++w)
        if (row_map[w] == row) {                              // uniform per workgroup
            acc += emb_w[(long)w * GE2E_EMB + tid];
            ++cnt;
        }
    float out = 0.f;
    if (cnt > 0) {
        const float mean = acc / (float)cnt;
        const float ss = block_sum(mean * mean, red);
        out = mean / sqrtf(ss);                               // no epsilon, as the reference
    }
    emb[(long)row * GE2E_EMB + tid] = out;
}

}  // namespace

int ge2e_host_tables(float* dft, float* pack, int32_t* tab) {
    const double pi = 3.14159265358979323846;
    std::vector<double> win(GE2E_NFFT);
    for (int u = 0; u < GE2E_NFFT; ++u) win[u] = 0.5 - 0.5 * cos(2.0 * pi * u / GE2E_NFFT);
    float* o = dft;
    for (int p = 0; p < GE2E_PAIRS; ++p)
        for (int c = 0; c < GE2E_KCHUNKS; ++c)
            for (int cs = 0; cs < 2; ++cs)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int bin = 16 * p + (lane & 15), u = 16 * c + 4 * (lane >> 4) + j;
                        double v = 0.0;
                        if (bin < GE2E_BINS && u < GE2E_NFFT) {
                            const double a = 2.0 * pi * (double)((bin * u) % GE2E_NFFT) / GE2E_NFFT;
                            v = win[u] * (cs ? sin(a) : cos(a));
                        }
                        *o++ = (float)v;
                    }
    std::vector<float> basis((size_t)GE2E_MELS * GE2E_BINS);
    if (mel_basis(GE2E_RATE, GE2E_NFFT, GE2E_MELS, 0.0, GE2E_RATE / 2.0, basis.data()) != 0) return -1;
    int nnz = 0;
    for (int m = 0; m < GE2E_MELS; ++m) {
        const float* row = basis.data() + (size_t)m * GE2E_BINS;
        int lo = 0, hi = GE2E_BINS;
        while (lo < GE2E_BINS && row[lo] == 0.f) ++lo;
        while (hi > lo && row[hi - 1] == 0.f) --hi;
        if (nnz + (hi - lo) > GE2E_NNZ_MAX) return -1;
        tab[3 * m] = nnz;
        tab[3 * m + 1] = lo;
        tab[3 * m + 2] = hi - lo;
        for (int k = lo; k < hi; ++k) pack[nnz++] = row[k];
    }
    return nnz;
}

extern "C" int cmtts_launch_ge2e_mel(const float* wav, long ld, int rows, const int32_t* n_valid, int mode, int max_windows, int T, const Ge2eTables* tb,
                                     float* windows, int32_t* win_lens, int32_t* info, void* stream) {
    if (rows <= 0) return 0;
    if (ld < 1 || ld >= (1L << 30) || (mode != 0 && mode != 1) || max_windows < 1 || (mode == 0 && (max_windows != 1 || T < 1)) ||
        (long)rows * max_windows > 65535)
        return -2;
    const int Tw = mode == 1 ? GE2E_FRAMES : T;
    hipLaunchKernelGGL(ge2e_mel_kernel, dim3((Tw + FE_FRAMES - 1) / FE_FRAMES, rows * max_windows), dim3(FE_THREADS), 0, (hipStream_t)stream, wav, ld,
                       n_valid, mode, max_windows, T, *tb, windows, win_lens, info);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_ge2e_layer(const float* x, int N, int T, int K, const float* wih, const float* whh, const float* bias, const int32_t* lens,
                                       int tile, float* pre, float* hseq, float* hlast, void* stream) {
    if (N <= 0) return 0;
    if (T < 1 || (K != GE2E_MELS && K != GE2E_HID) || tile != GE2E_TILE || (long)N * T > (1L << 31) - 64) return -2;
    const long R = (long)N * T;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ge2e_inproj_kernel, dim3((unsigned)((R + 31) / 32), 4), dim3(256), 0, s, x, R, K, wih, bias, pre);
    // NT = 2 (32 windows per workgroup) was built and measured: 87 spilled VGPRs, 23.7 ms against 11.3 ms per forward (profiles/ge2e.md); it left the build
    hipLaunchKernelGGL((ge2e_lstm_kernel<1>), dim3((N + 15) / 16), dim3(LSTM_THREADS), 0, s, pre, whh, lens, N, T, hseq, hlast);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_ge2e_tail(const float* hlast, int W, const float* lin_t, const float* lin_b, float* emb_w, const int32_t* row_map, int rows,
                                      float* emb, void* stream) {
    if (W > 0) hipLaunchKernelGGL(ge2e_proj_kernel, dim3(W), dim3(TAIL_THREADS), 0, (hipStream_t)stream, hlast, lin_t, lin_b, emb_w);
    if (row_map && rows > 0) hipLaunchKernelGGL(ge2e_rows_kernel, dim3(rows), dim3(TAIL_THREADS), 0, (hipStream_t)stream, emb_w, W, row_map, emb);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the handle and the C ABI ---------------------------------------------------------------------------------------------------------
struct Ge2eLayer {
    float *wih = nullptr, *whh = nullptr, *bias = nullptr;
};

struct cmtts_ge2e {
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    Allocs al;
    Ge2eLayer layers[GE2E_LAYERS];
    float *lin_t = nullptr, *lin_b = nullptr;
    Ge2eTables tb{};
};

// [M][K] row-major -> the fragment stream of its k-major form
static std::vector<float> lstm_stream(const std::vector<float>& w, int K) {
    std::vector<float> km((size_t)K * GE2E_GATES);
    for (int r = 0; r < GE2E_GATES; ++r)
        for (int k = 0; k < K; ++k) km[(size_t)k * GE2E_GATES + r] = w[(size_t)r * K + k];
    return to_lstm_fragments(km, K, GE2E_GATES);
}

static int upload_tables(Allocs& al, Ge2eTables* tb) {
    std::vector<float> dft(GE2E_DFT_FLOATS), pack(GE2E_NNZ_MAX, 0.f);
    std::vector<int32_t> tab(3 * GE2E_MELS);
    if (ge2e_host_tables(dft.data(), pack.data(), tab.data()) < 0) return fail(CMTTS_E_INVALID, "ge2e: the filterbank's rows are not single runs");
    float *d = nullptr, *p = nullptr;
    void* t = nullptr;
    CHK(al.upload(dft, &d));
    CHK(al.upload(pack, &p));
    CHK(al.upload_bytes(tab.data(), tab.size() * sizeof(int32_t), &t));
    tb->dft = d;
    tb->pack = p;
    tb->tab = (const int32_t*)t;
    return 0;
}

static size_t ge2e_forward_bytes(long W, long T) {
    return (size_t)(W * T * (GE2E_GATES + GE2E_HID) + 2 * W * GE2E_EMB) * sizeof(float) + (size_t)W * sizeof(int32_t) + 5 * 256;
}

extern "C" {

int cmtts_ge2e_create(cmtts_ge2e** out) {
    if (!out) return fail(CMTTS_E_INVALID, "cmtts_ge2e_create: null argument");
    *out = new cmtts_ge2e();
    return 0;
}

int cmtts_ge2e_set_tensor(cmtts_ge2e* e, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!e || !name) return fail(CMTTS_E_INVALID, "cmtts_ge2e_set_tensor: null argument");
    if (e->finalized) return fail(CMTTS_E_INVALID, "cmtts_ge2e_set_tensor: already finalized");
    return set_tensor(e->host, name, data, shape, ndim);
}

static int ge2e_finalize(cmtts_ge2e* e) {
    auto want = [&](const std::string& n, std::initializer_list<int64_t> shape, const HostTensor** t) {
        auto it = e->host.find(n);
        if (it == e->host.end()) return fail(CMTTS_E_INVALID, "cmtts_ge2e_finalize: missing tensor " + n);
        size_t i = 0;
        if (it->second.shape.size() != shape.size()) return fail(CMTTS_E_INVALID, "cmtts_ge2e_finalize: bad rank of " + n);
        for (int64_t d : shape)
            if (it->second.shape[i++] != d) return fail(CMTTS_E_INVALID, "cmtts_ge2e_finalize: bad shape of " + n);
        *t = &it->second;
        return 0;
    };
    for (int l = 0; l < GE2E_LAYERS; ++l) {
        const std::string sfx = "_l" + std::to_string(l);
        const int K = l == 0 ? GE2E_MELS : GE2E_HID;
        const HostTensor *wih, *whh, *bih, *bhh;
        CHK(want("lstm.weight_ih" + sfx, {GE2E_GATES, K}, &wih));
        CHK(want("lstm.weight_hh" + sfx, {GE2E_GATES, GE2E_HID}, &whh));
        CHK(want("lstm.bias_ih" + sfx, {GE2E_GATES}, &bih));
        CHK(want("lstm.bias_hh" + sfx, {GE2E_GATES}, &bhh));
        std::vector<float> bias(GE2E_GATES);
        for (int q = 0; q < GE2E_GATES; ++q) bias[q] = bih->data[lstm_packed_row(q)] + bhh->data[lstm_packed_row(q)];
        CHK(e->al.upload(lstm_stream(wih->data, K), &e->layers[l].wih));
        CHK(e->al.upload(lstm_stream(whh->data, GE2E_HID), &e->layers[l].whh));
        CHK(e->al.upload(bias, &e->layers[l].bias));
    }
    const HostTensor *lw, *lb;
    CHK(want("linear.weight", {GE2E_EMB, GE2E_HID}, &lw));
    CHK(want("linear.bias", {GE2E_EMB}, &lb));
    std::vector<float> lt((size_t)GE2E_HID * GE2E_EMB);
    for (int o = 0; o < GE2E_EMB; ++o)
        for (int k = 0; k < GE2E_HID; ++k) lt[(size_t)k * GE2E_EMB + o] = lw->data[(size_t)o * GE2E_HID + k];
    CHK(e->al.upload(lt, &e->lin_t));
    CHK(e->al.upload(lb->data, &e->lin_b));
    return upload_tables(e->al, &e->tb);
}

int cmtts_ge2e_finalize(cmtts_ge2e* e) {
    if (!e) return fail(CMTTS_E_INVALID, "cmtts_ge2e_finalize: null handle");
    if (e->finalized) return 0;
    const int rc = ge2e_finalize(e);
    if (rc != 0) {
        e->al.release();
        return rc;
    }
    e->finalized = true;
    e->host.clear();
    return 0;
}

void cmtts_ge2e_destroy(cmtts_ge2e* e) {
    if (!e) return;
    e->al.release();
    delete e;
}

size_t cmtts_ge2e_workspace_bytes(int W, int T) {
    if (W < 1 || W > 65535 || T < 1 || (long)W * T > (1L << 31) - 64) return 0;
    return ge2e_forward_bytes(W, T);
}

int cmtts_ge2e_features(cmtts_ge2e* e, const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, int mode, int max_windows, int T,
                        float* windows, int32_t* win_lens, int32_t* info, void* stream) {
    const std::string who = "cmtts_ge2e_features";
    if (!e || !wav || !n_valid || !windows || !win_lens || !info) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!e->finalized) return fail(CMTTS_E_INVALID, who + ": call cmtts_ge2e_finalize first");
    if (fs != GE2E_RATE) return fail(CMTTS_E_INVALID, who + ": the audio must be at 22050 Hz (the one rate the GE2E front end is defined at)");
    if (rows < 1 || ld < 1 || ld >= (1L << 30)) return fail(CMTTS_E_INVALID, who + ": rows and ld must be >= 1 (ld < 2^30)");
    if (mode != 0 && mode != 1) return fail(CMTTS_E_INVALID, who + ": mode must be 0 (whole utterance) or 1 (partials)");
    if (max_windows < 1 || (long)rows * max_windows > 65535 || (mode == 0 && (max_windows != 1 || T < 1)))
        return fail(CMTTS_E_INVALID, who + ": max_windows >= 1 (1 and T >= 1 for mode 0), rows * max_windows <= 65535");
    const int rc = cmtts_launch_ge2e_mel(wav, (long)ld, rows, n_valid, mode, max_windows, T, &e->tb, windows, win_lens, info, stream);
    return rc != 0 ? fail(CMTTS_E_HIP, "ge2e mel launch failed") : 0;
}

int cmtts_ge2e_forward(cmtts_ge2e* e, const float* windows, int W, int T, const int32_t* lengths, const int32_t* row_map, int rows, float* emb, void* ws,
                       size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_ge2e_forward";
    if (!e || !emb || (W > 0 && (!windows || !ws))) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!e->finalized) return fail(CMTTS_E_INVALID, who + ": call cmtts_ge2e_finalize first");
    if (rows < 1 || W < 0 || W > 65535 || T < 1 || (long)W * T > (1L << 31) - 64)
        return fail(CMTTS_E_INVALID, who + ": rows, T must be >= 1, 0 <= W <= 65535, W * T < 2^31");
    if (!row_map && rows != W) return fail(CMTTS_E_INVALID, who + ": without a row_map every window is a row (rows == W)");
    if (row_map)
        for (int w = 0; w < W; ++w)
            if (row_map[w] < 0 || row_map[w] >= rows) return fail(CMTTS_E_INVALID, who + ": row_map entry outside [0, rows)");
    if (W > 0 && ws_bytes < ge2e_forward_bytes(W, T)) return fail(CMTTS_E_INVALID, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws);
    float *pre = nullptr, *hseq = nullptr, *hlast = nullptr, *emb_w = nullptr;
    int32_t* rm = nullptr;
    if (W > 0) {
        pre = cv.take<float>((size_t)W * T * GE2E_GATES);
        hseq = cv.take<float>((size_t)W * T * GE2E_HID);
        hlast = cv.take<float>((size_t)W * GE2E_HID);
        emb_w = row_map ? cv.take<float>((size_t)W * GE2E_EMB) : emb;
        rm = cv.take<int32_t>((size_t)W);
        if (row_map) HIPCHK(hipMemcpyAsync(rm, row_map, (size_t)W * sizeof(int32_t), hipMemcpyHostToDevice, s));
        const float* x = windows;
        for (int l = 0; l < GE2E_LAYERS; ++l) {
            const Ge2eLayer& L = e->layers[l];
            // layer l + 1 reads hseq only through its projection, which has finished before its recurrence overwrites hseq
            if (cmtts_launch_ge2e_layer(x, W, T, l == 0 ? GE2E_MELS : GE2E_HID, L.wih, L.whh, L.bias, lengths, GE2E_TILE, pre, hseq, hlast, stream) != 0)
                return fail(CMTTS_E_HIP, "ge2e layer launch failed");
            x = hseq;
        }
    }
    if (W == 0) {                                             // rows without windows: zeros
        HIPCHK(hipMemsetAsync(emb, 0, (size_t)rows * GE2E_EMB * sizeof(float), s));
        return 0;
    }
    if (cmtts_launch_ge2e_tail(hlast, W, e->lin_t, e->lin_b, emb_w, row_map ? rm : nullptr, rows, emb, stream) != 0)
        return fail(CMTTS_E_HIP, "ge2e tail launch failed");
    return 0;
}

int cmtts_internal_ge2e_mel_basis(float* out) {
    return out ? mel_basis(GE2E_RATE, GE2E_NFFT, GE2E_MELS, 0.0, GE2E_RATE / 2.0, out) : CMTTS_E_INVALID;
}

int cmtts_internal_ge2e_mel(const float* wav, int rows, int64_t ld, const int32_t* n_valid, int mode, int max_windows, int T, float* windows,
                            int32_t* win_lens, int32_t* info, void* stream) {
    if (!wav || !n_valid || !windows || !win_lens || !info || rows < 1) return fail(CMTTS_E_INVALID, "cmtts_internal_ge2e_mel: invalid argument");
    Allocs al;
    Ge2eTables tb{};
    int rc = upload_tables(al, &tb);
    if (rc == 0) {
        rc = cmtts_launch_ge2e_mel(wav, (long)ld, rows, n_valid, mode, max_windows, T, &tb, windows, win_lens, info, stream);
        (void)hipStreamSynchronize((hipStream_t)stream);
        if (rc != 0) rc = fail(CMTTS_E_INVALID, "cmtts_internal_ge2e_mel: launch refused");
    }
    al.release();
    return rc;
}

}  // extern "C"
