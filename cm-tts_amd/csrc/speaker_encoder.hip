// Speaker embeddings from reference audio (include/cmtts_hip.h: cmtts_spkenc_*; definition: cmtts_amd/speaker.py).
//
//   trim     one workgroup per row.  |x| >= 0 orders as its uint32 bit pattern, so the two order statistics of the 95th percentile are an exact
//            radix select (four 8-bit digits, LDS histogram); the threshold is formed in double with separately rounded operations, the first
//            and last index above it are integer min / max reductions: nothing depends on the order lanes arrive in.
//   fbank    one workgroup per (window slot, frame): pre-emphasis while staging the frame bit-reversed into LDS, a 1024-point radix-2 FFT in
//            LDS, power, the 64 sparse triangle sums (one lane per filter, bins ascending), the per-frame normalisation on one wave, the
//            write into the window layout [W][160][64] — zero rows behind the utterance's end included.  All of it in DOUBLE, rounded to
//            float once at the store: the features are divided by a per-frame deviation, and a float32 FFT left a frame's 64 values up to
//            2.6 ulp off (4.08 x the float32 numpy definition on a one-frame signal); the work is 1/1000 of the net's.
//   conv2d   NHWC implicit GEMM on v_mfma_f32_16x16x4_f32: A = weights (16 output channels x 4 k), B = activations (4 k x 16 output pixels),
//            so a lane's four results are four consecutive channels of one pixel: one 16-byte store, bias and residual loads alike.  k runs over
//            (tap, input channel) in chunks of 16; a lane's chunk operand is ONE 16-byte load on either side (weight_pack.h: to_conv2d_fragments).
//            A wave owns 64 output channels x NT 16-pixel tiles.  Instances: KS = 1, the workgroup's four waves own four pixel groups; KS = 4, they
//            split the chunks of ONE tile four ways and wave 0 adds the partial sums in wave order — the instance is chosen by (cin, cout)
//            alone, so a pixel's bits do not depend on the batch.  Epilogue: bias, clip(0, 20), optional residual, clip.
//   tail     time mean -> dense 2048 -> 512 -> L2 norm per window; mean of a row's windows in window order -> L2 norm.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "internal_hooks.h"
#include "launch.h"
#include "model.h"
#include "speaker_encoder.h"
#include "weight_pack.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float SPK_CLIP = 20.0f;

// ---- trim ---------------------------------------------------------------------------------------------------------------------------
constexpr int TRIM_THREADS = 1024;

// the key of rank `rank` (0-based, ascending) among the |x| bit patterns of x[0:n); every lane returns it
__device__ uint32_t select_rank(const float* __restrict__ x, int n, int rank, int* hist, int* pick) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += TRIM_THREADS) {
            const uint32_t key = __float_as_uint(x[i]) & 0x7fffffffu;
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int r = rank, d = 0;
            for (; d < 255; ++d) {
                if (r < hist[d]) break;
                r -= hist[d];
            }
            pick[0] = d;
            pick[1] = r;
        }
        __syncthreads();
        prefix |= (uint32_t)pick[0] << shift;
        mask |= 255u << shift;
        rank = pick[1];
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(TRIM_THREADS) void spk_trim_kernel(const float* __restrict__ wav, long ld, const int32_t* __restrict__ n_valid,
                                                                int32_t* __restrict__ info) {
    __shared__ int hist[256];
    __shared__ int pick[2];
    __shared__ int lo, hi;
    const int row = blockIdx.x, tid = threadIdx.x;
    const long nv = n_valid[row];
    const int n = (int)(nv < 0 ? 0 : (nv > ld ? ld : nv));
    const float* x = wav + (long)row * ld;
    int first = -1, last = -1;
    if (n > 0) {                                              // uniform per workgroup
        const double p = __dmul_rn(0.95, (double)(n - 1));
        const int k = (int)floor(p);
        const double ek = (double)__uint_as_float(select_rank(x, n, k, hist, pick));
        const double ek1 = k + 1 < n ? (double)__uint_as_float(select_rank(x, n, k + 1, hist, pick)) : ek;
        const double thr = __dadd_rn(ek, __dmul_rn(__dsub_rn(p, (double)k), __dsub_rn(ek1, ek)));
        if (tid == 0) {
            lo = n;
            hi = -1;
        }
        __syncthreads();
        int mn = n, mx = -1;
        for (int i = tid; i < n; i += TRIM_THREADS)
            if ((double)fabsf(x[i]) > thr) {
                mn = min(mn, i);
                mx = max(mx, i);
            }
        if (mx >= 0) {
            atomicMin(&lo, mn);
            atomicMax(&hi, mx);
        }
        __syncthreads();
        if (hi > lo) {                                        // hi == lo: the kept span x[first:last] is empty
            first = lo;
            last = hi;
        }
    }
    if (tid == 0) {
        info[4 * row] = first;
        info[4 * row + 1] = last;
    }
}

// ---- fbank --------------------------------------------------------------------------------------------------------------------------
constexpr int FB_THREADS = 256;

// lane 0 receives the sum over the wave's 64 lanes, combined in a fixed tree
__device__ __forceinline__ double wave_sum(double v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// frames and windows of a row from its kept span
__device__ __forceinline__ void spk_counts(int first, int last, const SpkPlan& p, int mode, int max_windows, int* F, int* nwin) {
    const int m = first < 0 ? 0 : last - first;
    const int f = m <= 0 ? 0 : (m > p.frame_len ? 1 + (m - p.frame_len + p.frame_step - 1) / p.frame_step : 1);
    int w = f > 0 ? 1 : 0;
    if (mode == 1 && f > SPK_FRAMES) w = min((f - SPK_FRAMES + SPK_HOP - 1) / SPK_HOP + 1, max_windows);
    *F = f;
    *nwin = w;
}

__global__ __launch_bounds__(FB_THREADS) void spk_fbank_kernel(const float* __restrict__ wav, long ld, int32_t* __restrict__ info, const SpkPlan p,
                                                               int mode, const int32_t* __restrict__ offsets, int max_windows,
                                                               const double* __restrict__ twiddle, float* __restrict__ windows) {
    __shared__ double re[SPK_NFFT], im[SPK_NFFT];
    __shared__ double pw[SPK_NFFT / 2 + 1];
    __shared__ int base_s;
    const int tid = threadIdx.x, t = blockIdx.x;
    const int row = blockIdx.y / max_windows, j = blockIdx.y - row * max_windows;
    const int first = info[4 * row], last = info[4 * row + 1];
    int F, nwin;
    spk_counts(first, last, p, mode, max_windows, &F, &nwin);
    if (t == 0 && j == 0 && tid == 0) {
        info[4 * row + 2] = F;
        info[4 * row + 3] = nwin;
    }
    if (j >= nwin) return;                                    // uniform per workgroup
    // windows of the rows before this one (integer sum: any order)
    if (tid == 0) base_s = 0;
    __syncthreads();
    int before = 0;
    for (int r = tid; r < row; r += FB_THREADS) {
        int f2, w2;
        spk_counts(info[4 * r], info[4 * r + 1], p, mode, max_windows, &f2, &w2);
        before += w2;
    }
    if (before) atomicAdd(&base_s, before);
    __syncthreads();
    const int room = max(F - SPK_FRAMES, 0);
    int off;
    if (mode == 0) off = room / 2;
    else if (mode == 2) off = min(max(offsets[row], 0), room);
    else off = j < (room + SPK_HOP - 1) / SPK_HOP ? SPK_HOP * j : room;
    float* out = windows + ((long)(base_s + j) * SPK_FRAMES + t) * SPK_FBANKS;
    const int f = off + t;
    if (f >= F) {                                             // zero rows behind the utterance's end
        if (tid < SPK_FBANKS) out[tid] = 0.f;
        return;
    }
    // the frame, pre-emphasised, at bit-reversed positions
    const float* s = wav + (long)row * ld + first;
    const int m = last - first;
    for (int u = tid; u < SPK_NFFT; u += FB_THREADS) {
        const int i = f * p.frame_step + u;
        double v = 0.0;
        if (u < p.frame_len && i < m) v = i == 0 ? (double)s[0] : __dsub_rn((double)s[i], __dmul_rn(0.97, (double)s[i - 1]));
        const int br = (int)(__brev((unsigned)u) >> 22);
        re[br] = v;
        im[br] = 0.0;
    }
    __syncthreads();
    for (int half = 1; half < SPK_NFFT; half <<= 1) {
        const int tstep = (SPK_NFFT / 2) / half;
        for (int b = tid; b < SPK_NFFT / 2; b += FB_THREADS) {
            const int pos = b & (half - 1);
            const int i0 = ((b - pos) << 1) + pos, i1 = i0 + half;
            const double wr = twiddle[2 * pos * tstep], wi = twiddle[2 * pos * tstep + 1];
            const double xr = re[i1], xi = im[i1];
            const double tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
            const double ar = re[i0], ai = im[i0];
            re[i0] = ar + tr;
            im[i0] = ai + ti;
            re[i1] = ar - tr;
            im[i1] = ai - ti;
        }
        __syncthreads();
    }
    for (int k = tid; k <= SPK_NFFT / 2; k += FB_THREADS) pw[k] = (re[k] * re[k] + im[k] * im[k]) * (1.0 / SPK_NFFT);
    __syncthreads();
    if (tid >= SPK_FBANKS) return;                            // wave 0 finishes
    const int b0 = p.bins[tid], b1 = p.bins[tid + 1], b2 = p.bins[tid + 2];
    double acc = 0.0;
    for (int i = b0; i < b1; ++i) acc += pw[i] * ((double)(i - b0) / (double)(b1 - b0));
    for (int i = b1; i < b2; ++i) acc += pw[i] * ((double)(b2 - i) / (double)(b2 - b1));
    if (acc == 0.0) acc = 2.220446049250313e-16;
    const double mean = __shfl(wave_sum(acc), 0) * (1.0 / SPK_FBANKS);
    const double d = acc - mean;
    const double sd = sqrt(__shfl(wave_sum(d * d), 0) * (1.0 / SPK_FBANKS));
    out[tid] = (float)(d / fmax(sd, 1e-12));
}

// ---- conv2d -------------------------------------------------------------------------------------------------------------------------
struct ConvGeom {
    int Ho, Wo, pad_t, pad_l, P, nchunk, cpt_shift;          // P = B Ho Wo output pixels; cpt = cin / 16 chunks per tap = 1 << cpt_shift
};

__device__ __forceinline__ f32x4 clip4(f32x4 v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fminf(fmaxf(v[r], 0.f), SPK_CLIP);
    return v;
}

template <int NT, int KS, bool CIN1>
__global__ __launch_bounds__(256) void conv2d_mfma_kernel(const SpkConvArgs a, const ConvGeom g) {
    constexpr int MT = 4;                                     // 64 output channels per wave
    __shared__ float red[KS == 4 ? 3 * MT * NT * 4 * 64 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int pl = lane & 15, kk = lane >> 4;
    const int m0 = blockIdx.y * 64;
    const int p0 = (blockIdx.x * (KS == 1 ? 4 : 1) + (KS == 1 ? wid : 0)) * NT * 16;
    const int c_begin = KS == 4 ? wid * (g.nchunk / 4) : 0, c_end = KS == 4 ? c_begin + g.nchunk / 4 : g.nchunk;

    // this lane's pixel of every n-tile
    int iy0[NT], ix0[NT];
    long xb[NT];
    bool pv[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int pix = p0 + 16 * i + pl;
        pv[i] = pix < g.P;
        const int pc = pv[i] ? pix : 0;
        const int b = pc / (g.Ho * g.Wo), r = pc - b * (g.Ho * g.Wo);
        const int oy = r / g.Wo, ox = r - oy * g.Wo;
        iy0[i] = oy * a.stride - g.pad_t;
        ix0[i] = ox * a.stride - g.pad_l;
        xb[i] = (long)b * a.H * a.W;
    }
    const f32x4* wfrag = reinterpret_cast<const f32x4*>(a.wf) + (long)(m0 / 16) * 64 + lane;
    const long wchunk = (long)(a.cout / 16) * 64;            // f32x4 per chunk

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 wv[2][MT], xv[2][NT];
    // loads are unconditional from a clamped, always valid address; the select follows
    auto load = [&](int c, f32x4* w, f32x4* x) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) w[mi] = wfrag[c * wchunk + mi * 64];
        if (CIN1) {
#pragma unroll
            for (int ni = 0; ni < NT; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int tap = 16 * c + 4 * kk + j;
                    const int ty = tap / a.ks, tx = tap - ty * a.ks;
                    const int iy = iy0[ni] + ty, ix = ix0[ni] + tx;
                    const bool ok = pv[ni] && tap < a.ks * a.ks && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                    const float v = a.x[ok ? xb[ni] + (long)iy * a.W + ix : 0];
                    x[ni][j] = ok ? v : 0.f;
                }
        } else {
            const int tap = c >> g.cpt_shift;
            const int cin0 = ((c - (tap << g.cpt_shift)) << 4) + 4 * kk;
            const int ty = tap / a.ks, tx = tap - ty * a.ks;
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) {
                const int iy = iy0[ni] + ty, ix = ix0[ni] + tx;
                const bool ok = pv[ni] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (ok ? (xb[ni] + (long)iy * a.W + ix) * a.cin + cin0 : 0));
                x[ni] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    if (c_begin < c_end) load(c_begin, wv[0], xv[0]);
    for (int c = c_begin; c < c_end; ++c) {
        const int cur = (c - c_begin) & 1;
        if (c + 1 < c_end) load(c + 1, wv[cur ^ 1], xv[cur ^ 1]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[cur][mi][j], xv[cur][ni][j], acc[mi][ni], 0, 0, 0);
    }

    if (KS == 4) {                                            // partial sums of waves 1 .. 3 -> wave 0, added in wave order
        if (wid > 0) {
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[(((wid - 1) * MT * NT + mi * NT + ni) * 4 + r) * 64 + lane] = acc[mi][ni][r];
        }
        __syncthreads();
        if (wid > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[mi][ni][r] += red[((w * MT * NT + mi * NT + ni) * 4 + r) * 64 + lane];
    }

    // lane: pixel pl of the n-tile, output channels m0 + 16 mi + 4 kk .. + 3
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        const int pix = p0 + 16 * ni + pl;
        if (pix >= g.P) continue;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
            const long o = (long)pix * a.cout + m0 + 16 * mi + 4 * kk;
            f32x4 v = clip4(acc[mi][ni] + *reinterpret_cast<const f32x4*>(a.bias + m0 + 16 * mi + 4 * kk));
            if (a.res) v = clip4(v + *reinterpret_cast<const f32x4*>(a.res + o));
            *reinterpret_cast<f32x4*>(a.y + o) = v;
        }
    }
}

// ---- tail ---------------------------------------------------------------------------------------------------------------------------
constexpr int TAIL_THREADS = SPK_EMB;

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

__global__ __launch_bounds__(TAIL_THREADS) void spk_dense_kernel(const float* __restrict__ feat, const float* __restrict__ dense,
                                                                 const float* __restrict__ bias, float* __restrict__ emb_w) {
    __shared__ float v[SPK_DENSE_IN];
    __shared__ float red[TAIL_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    const float* f = feat + (long)w * 10 * SPK_DENSE_IN;
    for (int i = tid; i < SPK_DENSE_IN; i += TAIL_THREADS) {
        float s = f[i];
        for (int h = 1; h < 10; ++h) s += f[h * SPK_DENSE_IN + i];
        v[i] = s / 10.0f;
    }
    __syncthreads();
    float acc = 0.f;
    for (int k = 0; k < SPK_DENSE_IN; ++k) acc = fmaf(v[k], dense[(long)k * SPK_EMB + tid], acc);
    acc += bias[tid];
    const float ss = block_sum(acc * acc, red);
    emb_w[(long)w * SPK_EMB + tid] = acc / sqrtf(fmaxf(ss, 1e-12f));
}

__global__ __launch_bounds__(TAIL_THREADS) void spk_rows_kernel(const float* __restrict__ emb_w, int W, const int32_t* __restrict__ row_map,
                                                                float* __restrict__ emb) {
    __shared__ float red[TAIL_THREADS];
    const int row = blockIdx.x, tid = threadIdx.x;
    float acc = 0.f;
    int cnt = 0;
    for (int w = 0; w < W; ++w)
        if (row_map[w] == row) {                              // uniform per workgroup
            acc += emb_w[(long)w * SPK_EMB + tid];
            ++cnt;
        }
    float out = 0.f;
    if (cnt > 0) {
        const float mean = acc / (float)cnt;
        const float ss = block_sum(mean * mean, red);
        out = mean / sqrtf(fmaxf(ss, 1e-12f));
    }
    emb[(long)row * SPK_EMB + tid] = out;
}

int same_pad_before(int n, int k, int s, int* out) {
    *out = (n + s - 1) / s;
    const int total = (*out - 1) * s + k - n;
    return total > 0 ? total / 2 : 0;
}

}  // namespace

int speaker_plan(int fs, int win_length, SpkPlan* plan) {
    if (fs < SPK_MIN_RATE || fs > SPK_MAX_RATE || win_length <= SPK_NFFT / 2 || win_length > SPK_NFFT) return -1;
    plan->frame_len = (int)floor(0.025 * fs + 0.5);
    plan->frame_step = (int)floor(0.01 * fs + 0.5);
    const double hi = 2595.0 * log10(1.0 + (fs / 2.0) / 700.0);
    for (int i = 0; i < SPK_FBANKS + 2; ++i) {
        // numpy.linspace(0, hi, 66): i * step with step = hi / 65; the last point is hi itself
        const double mel = i == SPK_FBANKS + 1 ? hi : i * (hi / (SPK_FBANKS + 1));
        const double hz = 700.0 * (pow(10.0, mel / 2595.0) - 1.0);
        plan->bins[i] = (int)floor((SPK_NFFT + 1) * hz / fs);
        if (plan->bins[i] > SPK_NFFT / 2) plan->bins[i] = SPK_NFFT / 2;
    }
    return 0;
}

extern "C" int cmtts_launch_spk_trim(const float* wav, long ld, int rows, const int32_t* n_valid, int32_t* info, void* stream) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(spk_trim_kernel, dim3(rows), dim3(TRIM_THREADS), 0, (hipStream_t)stream, wav, ld, n_valid, info);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_spk_fbank(const float* wav, long ld, int rows, int32_t* info, const SpkPlan* plan, int mode, const int32_t* offsets,
                                      int max_windows, const double* twiddle, float* windows, void* stream) {
    if (rows <= 0) return 0;
    if (max_windows < 1 || max_windows > SPK_MAX_WINDOWS || (long)rows * max_windows > 65535 || mode < 0 || mode > 2 || (mode == 2 && !offsets))
        return -2;
    hipLaunchKernelGGL(spk_fbank_kernel, dim3(SPK_FRAMES, rows * max_windows), dim3(FB_THREADS), 0, (hipStream_t)stream, wav, ld, info, *plan, mode,
                       offsets, max_windows, twiddle, windows);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_spk_conv2d(const SpkConvArgs* a, void* stream) {
    const bool cin1 = a->cin == 1;
    if (a->B < 1 || a->H < 1 || a->W < 1 || (a->ks != 3 && a->ks != 5) || (a->stride != 1 && a->stride != 2)) return -2;
    if (cin1 ? a->cout != 64 : (a->cin % 64 != 0 || a->cin > 512)) return -2;
    if (a->cout != 64 && a->cout != 128 && a->cout != 256 && a->cout != 512) return -2;
    ConvGeom g;
    g.pad_t = same_pad_before(a->H, a->ks, a->stride, &g.Ho);
    g.pad_l = same_pad_before(a->W, a->ks, a->stride, &g.Wo);
    const long P = (long)a->B * g.Ho * g.Wo;
    if (P > (1L << 30) || (long)a->B * a->H * a->W * a->cin > (1L << 40)) return -2;
    g.P = (int)P;
    g.nchunk = (a->ks * a->ks * a->cin + 15) / 16;
    g.cpt_shift = 0;
    while (!cin1 && (16 << g.cpt_shift) < a->cin) ++g.cpt_shift;
    if (!cin1 && (16 << g.cpt_shift) != a->cin) return -2;   // cin / 16 must be a power of two: 64, 128, 256, 512
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(256);
    auto tiles = [&](int per) { return (unsigned)((P + per - 1) / per); };
    if (cin1) hipLaunchKernelGGL((conv2d_mfma_kernel<2, 1, true>), dim3(tiles(128), 1), blk, 0, s, *a, g);
    else if (a->cout == 64) hipLaunchKernelGGL((conv2d_mfma_kernel<2, 1, false>), dim3(tiles(128), 1), blk, 0, s, *a, g);
    // cout >= 128: the four-way K split.  NT never enters a pixel's summation order, so it could follow the launch size; NT = 4 / 2 from 256 workgroups
    // on was built and measured SLOWER (W = 32: 5.84 ms against 4.79 ms, 352 VGPRs at NT = 4): these launches wait on their operand loads, not on L2 bandwidth
    else if (a->cout == 128) hipLaunchKernelGGL((conv2d_mfma_kernel<2, 4, false>), dim3(tiles(32), 2), blk, 0, s, *a, g);
    else hipLaunchKernelGGL((conv2d_mfma_kernel<1, 4, false>), dim3(tiles(16), a->cout / 64), blk, 0, s, *a, g);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_spk_tail(const float* feat, int W, const float* dense, const float* bias, float* emb_w, const int32_t* row_map,
                                     int rows, float* emb, void* stream) {
    if (W > 0) hipLaunchKernelGGL(spk_dense_kernel, dim3(W), dim3(TAIL_THREADS), 0, (hipStream_t)stream, feat, dense, bias, emb_w);
    if (rows > 0) hipLaunchKernelGGL(spk_rows_kernel, dim3(rows), dim3(TAIL_THREADS), 0, (hipStream_t)stream, emb_w, W, row_map, emb);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the handle and the C ABI ---------------------------------------------------------------------------------------------------------
struct SpkLayer {
    std::string name;
    int ks, stride, cin, cout;
    float *wf = nullptr, *bias = nullptr;
};

struct cmtts_spkenc {
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    Allocs al;
    std::vector<SpkLayer> layers;
    float *dense = nullptr, *dense_b = nullptr;
    double* twiddle = nullptr;
};

static const int SPK_STAGES[4] = {64, 128, 256, 512};
constexpr long SPK_ACT_FLOATS = 80L * 32 * 64;              // the largest activation of a window (stage 1: 80 x 32 x 64; later stages halve it)

static std::vector<double> spk_twiddles() {
    std::vector<double> t(SPK_NFFT);
    for (int k = 0; k < SPK_NFFT / 2; ++k) {
        const double a = -2.0 * M_PI * k / SPK_NFFT;
        t[2 * k] = cos(a);
        t[2 * k + 1] = sin(a);
    }
    return t;
}

static size_t spk_forward_bytes(long W) { return (size_t)(2 * W * SPK_ACT_FLOATS + W * SPK_EMB) * sizeof(float) + 3 * 256; }

extern "C" {

int cmtts_spkenc_create(cmtts_spkenc** out) {
    if (!out) return fail(CMTTS_E_INVALID, "cmtts_spkenc_create: null argument");
    *out = new cmtts_spkenc();
    return 0;
}

int cmtts_spkenc_set_tensor(cmtts_spkenc* e, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!e || !name) return fail(CMTTS_E_INVALID, "cmtts_spkenc_set_tensor: null argument");
    if (e->finalized) return fail(CMTTS_E_INVALID, "cmtts_spkenc_set_tensor: already finalized");
    std::string n = name;
    if (n.size() > 2 && n.compare(n.size() - 2, 2, ":0") == 0) n.resize(n.size() - 2);      // a saved Keras variable's suffix
    return set_tensor(e->host, n.c_str(), data, shape, ndim);
}

static int spk_finalize(cmtts_spkenc* e) {
    auto want = [&](const std::string& n, std::initializer_list<int64_t> shape, const HostTensor** t) {
        auto it = e->host.find(n);
        if (it == e->host.end()) return fail(CMTTS_E_INVALID, "cmtts_spkenc_finalize: missing tensor " + n);
        size_t i = 0;
        if (it->second.shape.size() != shape.size()) return fail(CMTTS_E_INVALID, "cmtts_spkenc_finalize: bad rank of " + n);
        for (int64_t d : shape)
            if (it->second.shape[i++] != d) return fail(CMTTS_E_INVALID, "cmtts_spkenc_finalize: bad shape of " + n);
        *t = &it->second;
        return 0;
    };
    e->layers.clear();
    int cin = 1;
    for (int s = 0; s < 4; ++s) {
        const int c = SPK_STAGES[s];
        e->layers.push_back({"conv" + std::to_string(c) + "-s", 5, 2, cin, c});
        for (int b = 0; b < 3; ++b)
            for (const char* ab : {"_2a", "_2b"})
                e->layers.push_back({"res" + std::to_string(s + 1) + "_" + std::to_string(b) + "_branch" + ab, 3, 1, c, c});
        cin = c;
    }
    for (SpkLayer& L : e->layers) {
        const HostTensor *k, *b, *bn[4];
        CHK(want(L.name + "/kernel", {L.ks, L.ks, L.cin, L.cout}, &k));
        CHK(want(L.name + "/bias", {L.cout}, &b));
        const char* part[4] = {"gamma", "beta", "moving_mean", "moving_variance"};
        std::vector<float> bnv;
        for (int i = 0; i < 4; ++i) {
            CHK(want(L.name + "_bn/" + part[i], {L.cout}, &bn[i]));
            bnv.insert(bnv.end(), bn[i]->data.begin(), bn[i]->data.end());
        }
        std::vector<float> bias;
        const std::vector<float> f = pack_conv2d_bn(k->data, L.ks * L.ks, L.cin, L.cout, b->data.data(), bnv.data(), &bias);
        if (f.empty()) return fail(CMTTS_E_INVALID, "cmtts_spkenc_finalize: no packer for " + L.name);
        CHK(e->al.upload(f, &L.wf));
        CHK(e->al.upload(bias, &L.bias));
    }
    const HostTensor *dk, *db;
    CHK(want("affine/kernel", {SPK_DENSE_IN, SPK_EMB}, &dk));
    CHK(want("affine/bias", {SPK_EMB}, &db));
    CHK(e->al.upload(dk->data, &e->dense));
    CHK(e->al.upload(db->data, &e->dense_b));
    const std::vector<double> tw = spk_twiddles();
    CHK(e->al.upload_bytes(tw.data(), tw.size() * sizeof(double), (void**)&e->twiddle));
    return 0;
}

int cmtts_spkenc_finalize(cmtts_spkenc* e) {
    if (!e) return fail(CMTTS_E_INVALID, "cmtts_spkenc_finalize: null handle");
    if (e->finalized) return 0;
    const int rc = spk_finalize(e);
    if (rc != 0) {
        e->al.release();
        return rc;
    }
    e->finalized = true;
    e->host.clear();
    return 0;
}

void cmtts_spkenc_destroy(cmtts_spkenc* e) {
    if (!e) return;
    e->al.release();
    delete e;
}

size_t cmtts_spkenc_workspace_bytes(int rows, int64_t ld, int max_windows) {
    if (rows < 1 || ld < 1 || max_windows < 1 || max_windows > SPK_MAX_WINDOWS) return 0;
    return spk_forward_bytes((long)rows * max_windows);
}

int cmtts_spkenc_features(cmtts_spkenc* e, const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, int win_length, int mode,
                          const int32_t* offsets, int max_windows, float* windows, int32_t* info, void* stream) {
    const std::string who = "cmtts_spkenc_features";
    if (!e || !wav || !n_valid || !windows || !info) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!e->finalized) return fail(CMTTS_E_INVALID, who + ": call cmtts_spkenc_finalize first");
    if (rows < 1 || ld < 1 || ld > INT32_MAX) return fail(CMTTS_E_INVALID, who + ": rows and ld must be >= 1 (ld < 2^31)");
    if (mode < 0 || mode > 2 || (mode == 2 && !offsets)) return fail(CMTTS_E_INVALID, who + ": mode must be 0, 1 or 2 (2 with offsets)");
    if (max_windows < 1 || max_windows > SPK_MAX_WINDOWS || (long)rows * max_windows > 65535 || (mode != 1 && max_windows != 1))
        return fail(CMTTS_E_INVALID, who + ": max_windows must be 1 (in 1 .. 64 for mode 1), rows * max_windows <= 65535");
    SpkPlan plan;
    if (speaker_plan(fs, win_length, &plan) != 0)
        return fail(CMTTS_E_INVALID, who + ": unsupported fs / win_length (8000 <= fs <= 40000, 512 < win_length <= 1024)");
    if (cmtts_launch_spk_trim(wav, (long)ld, rows, n_valid, info, stream) != 0) return fail(CMTTS_E_HIP, "speaker trim launch failed");
    if (cmtts_launch_spk_fbank(wav, (long)ld, rows, info, &plan, mode, offsets, max_windows, e->twiddle, windows, stream) != 0)
        return fail(CMTTS_E_HIP, "speaker fbank launch failed");
    return 0;
}

int cmtts_spkenc_forward(cmtts_spkenc* e, const float* windows, int W, const int32_t* row_map, int rows, float* emb, void* ws, size_t ws_bytes,
                         void* stream) {
    const std::string who = "cmtts_spkenc_forward";
    if (!e || !emb || !row_map || (W > 0 && (!windows || !ws))) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!e->finalized) return fail(CMTTS_E_INVALID, who + ": call cmtts_spkenc_finalize first");
    if (rows < 1 || W < 0 || W > 65535) return fail(CMTTS_E_INVALID, who + ": rows must be >= 1, 0 <= W <= 65535");
    if (W > 0 && ws_bytes < spk_forward_bytes(W)) return fail(CMTTS_E_INVALID, who + ": workspace too small");
    Carver cv(ws);
    float* act[2] = {nullptr, nullptr};
    float* emb_w = nullptr;
    if (W > 0) {
        act[0] = cv.take<float>((size_t)W * SPK_ACT_FLOATS);
        act[1] = cv.take<float>((size_t)W * SPK_ACT_FLOATS);
        emb_w = cv.take<float>((size_t)W * SPK_EMB);
        const float* x = windows;
        int H = SPK_FRAMES, Wd = SPK_FBANKS, cur = 0;       // act[cur]: where the next strided conv writes
        for (size_t i = 0; i < e->layers.size(); i += 7) {
            SpkConvArgs a{x, e->layers[i].wf, e->layers[i].bias, nullptr, act[cur], W, H, Wd, e->layers[i].cin, e->layers[i].cout, 5, 2};
            if (cmtts_launch_spk_conv2d(&a, stream) != 0) return fail(CMTTS_E_HIP, "speaker conv launch failed: " + e->layers[i].name);
            H = (H + 1) / 2;
            Wd = (Wd + 1) / 2;
            const int c = e->layers[i].cout;
            for (int b = 0; b < 3; ++b) {
                const SpkLayer &la = e->layers[i + 1 + 2 * b], &lb = e->layers[i + 2 + 2 * b];
                SpkConvArgs a1{act[cur], la.wf, la.bias, nullptr, act[cur ^ 1], W, H, Wd, c, c, 3, 1};
                SpkConvArgs a2{act[cur ^ 1], lb.wf, lb.bias, act[cur], act[cur], W, H, Wd, c, c, 3, 1};
                if (cmtts_launch_spk_conv2d(&a1, stream) != 0 || cmtts_launch_spk_conv2d(&a2, stream) != 0)
                    return fail(CMTTS_E_HIP, "speaker conv launch failed: " + la.name);
            }
            x = act[cur];
            cur ^= 1;
        }
        if (cmtts_launch_spk_tail(x, W, e->dense, e->dense_b, emb_w, row_map, rows, emb, stream) != 0)
            return fail(CMTTS_E_HIP, "speaker tail launch failed");
    } else if (cmtts_launch_spk_tail(nullptr, 0, e->dense, e->dense_b, nullptr, row_map, rows, emb, stream) != 0) {
        return fail(CMTTS_E_HIP, "speaker tail launch failed");
    }
    return 0;
}

int cmtts_internal_spkenc_conv(const float* x, const float* frag, const float* bias, const float* res, int B, int H, int W, int cin, int cout, int ks,
                               int stride, float* y, void* stream) {
    if (!x || !frag || !bias || !y) return fail(CMTTS_E_INVALID, "cmtts_internal_spkenc_conv: null argument");
    SpkConvArgs a{x, frag, bias, res, y, B, H, W, cin, cout, ks, stride};
    const int rc = cmtts_launch_spk_conv2d(&a, stream);
    if (rc == -2) return fail(CMTTS_E_INVALID, "cmtts_internal_spkenc_conv: no instance for this shape");
    return rc != 0 ? fail(CMTTS_E_HIP, "speaker conv launch failed") : 0;
}

int cmtts_internal_spkenc_fbank(const float* wav, int rows, int64_t ld, int fs, int win_length, int mode, const int32_t* offsets, int max_windows,
                                float* windows, int32_t* info, void* stream) {
    SpkPlan plan;
    if (!wav || !windows || !info || rows < 1 || ld < 1 || ld > INT32_MAX || speaker_plan(fs, win_length, &plan) != 0)
        return fail(CMTTS_E_INVALID, "cmtts_internal_spkenc_fbank: invalid argument");
    const std::vector<double> t = spk_twiddles();
    double* tw = nullptr;
    HIPCHK(hipMalloc((void**)&tw, t.size() * sizeof(double)));
    HIPCHK(hipMemcpy(tw, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    const int rc = cmtts_launch_spk_fbank(wav, (long)ld, rows, info, &plan, mode, offsets, max_windows, tw, windows, stream);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipFree(tw));
    return rc != 0 ? fail(CMTTS_E_INVALID, "cmtts_internal_spkenc_fbank: launch refused") : 0;
}

}  // extern "C"
