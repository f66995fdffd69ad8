// Objective metrics of a rendering against the recording it was made from (include/cmtts_hip.h: cmtts_metric_*; definition:
// cmtts_amd/metrics.py).
//
//   cepstra    c[t][k] = sum_n mel[t][n] D[n][k], the orthonormal DCT-II of the 80-channel log-mel.  A workgroup owns 32 frames of one row, stages
//              them and the float32 table in LDS; a thread's output is one fused chain of 80 terms.
//   cost       c[i][j] = sqrt(sum_k (cx[i][k] - cy[j][k])^2) over coefficients k_lo .. k_hi, in the difference form on the VALU: the shape of
//              align_cost_kernel — a 64 x 64 tile of one pair per workgroup, both sides' K columns in LDS, a 4 x 4 micro-tile per thread, one
//              fused chain of K terms per cell, then a correctly rounded square root.  The DTW of align.hip takes the matrix as it lies.
//   diagonal   align="frame": the float32 sum of c[j][j], j ascending, over min(x_len, y_len) frames.
//   f0         one wave per pair over the recording's frames j with the rendering's frame row[j]: integer counts, then double sums in the
//              definition's order (lane l takes frames l, l + 64, ...; the lanes are joined by halving, xor 32 .. 1), two passes.
//   prepare    one workgroup per pair: per side and column the L2 norm over the frames (double, four interleaved partial sums joined
//              (0 + 1) + (2 + 3), as align_means_kernel), then every value over its norm, rounded once; the pair's min and max.
//   ssim       one workgroup per (pair, 8 window rows): 18 frames of both images in LDS, the five moment maps filtered along time, then along
//              the coefficients, in double, taps ascending; the tile's sum of the index goes to the workspace, a second launch joins a pair's
//              tiles in a fixed order.  The tiles depend on the pair's own length alone: a pair's bits do not depend on its batch.
// No atomics, vector stores only.  Frames, cells and rows at or beyond a pair's lengths are neither read nor written.  Built without FMA
// contraction (Makefile): every operation that the definition rounds once is rounded once here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "metrics.h"
#include "model.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ double wave_sum(double v) {      // joined by halving: lane l takes l ^ 32, then 16, .. 1; every lane ends with the sum
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// ---- cepstra ---------------------------------------------------------------------------------------------------------------------------
constexpr int MC_FRAMES = 32, MC_THREADS = 256, MC_LD = MT_CH + 1;

__global__ __launch_bounds__(MC_THREADS) void metric_cepstra_kernel(const float* __restrict__ mel, const int32_t* __restrict__ lens,
                                                                     const float* __restrict__ table, int T, int n_cep, float* __restrict__ cep) {
    __shared__ float ms[MC_FRAMES * MC_LD];
    __shared__ float ds[MT_CH * MT_CH];                     // [n][k], leading dimension n_cep
    const int b = blockIdx.y, t0 = blockIdx.x * MC_FRAMES, tid = threadIdx.x;
    const int n = clampi(lens[b], 0, T);
    if (t0 >= n) return;
    const int rows = min(MC_FRAMES, n - t0);
    for (int e = tid; e < MT_CH * n_cep; e += MC_THREADS) ds[e] = table[e];
    const float* mb = mel + ((size_t)b * T + t0) * MT_CH;
    for (int e = tid; e < rows * MT_CH; e += MC_THREADS) {
        const int r = e / MT_CH, k = e - r * MT_CH;
        ms[r * MC_LD + k] = mb[e];
    }
    __syncthreads();
    float* cb = cep + ((size_t)b * T + t0) * n_cep;
    for (int e = tid; e < rows * n_cep; e += MC_THREADS) {
        const int r = e / n_cep, k = e - r * n_cep;
        float s = 0.f;
#pragma unroll 8
        for (int c = 0; c < MT_CH; ++c) s = fmaf(ms[r * MC_LD + c], ds[c * n_cep + k], s);
        cb[e] = s;
    }
}

// ---- cost ------------------------------------------------------------------------------------------------------------------------------
constexpr int MK_TILE = 64, MK_LD = MT_CH + 1, MK_THREADS = 256;

__global__ __launch_bounds__(MK_THREADS) void metric_cost_kernel(const float* __restrict__ cx, const float* __restrict__ cy,
                                                                  const int32_t* __restrict__ x_len, const int32_t* __restrict__ y_len, int Ts, int Tr,
                                                                  int n_cep, int k_lo, int K, float* __restrict__ cost) {
    __shared__ float xs[MK_TILE * MK_LD], ys[MK_TILE * MK_LD];
    const int b = blockIdx.z, i0 = blockIdx.y * MK_TILE, j0 = blockIdx.x * MK_TILE;
    const int xl = clampi(x_len[b], 1, Ts), yl = clampi(y_len[b], 1, Tr);
    if (i0 >= xl || j0 >= yl) return;
    const int tid = threadIdx.x;
    const float* xb = cx + (size_t)b * Ts * n_cep + k_lo;
    const float* yb = cy + (size_t)b * Tr * n_cep + k_lo;
    for (int e = tid; e < MK_TILE * K; e += MK_THREADS) {
        const int r = e / K, k = e - r * K;
        const int gi = i0 + r, gj = j0 + r;
        xs[r * MK_LD + k] = gi < xl ? xb[(size_t)gi * n_cep + k] : 0.f;
        ys[r * MK_LD + k] = gj < yl ? yb[(size_t)gj * n_cep + k] : 0.f;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    for (int k = 0; k < K; ++k) {
        float xa[4], yc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            xa[a] = xs[(ty + 16 * a) * MK_LD + k];
            yc[a] = ys[(tx + 16 * a) * MK_LD + k];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = xa[a] - yc[c];
                acc[a][c] = fmaf(d, d, acc[a][c]);
            }
    }
    float* cb = cost + (size_t)b * Ts * Tr;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
            if (i < xl && j < yl) cb[(size_t)i * Tr + j] = sqrtf(acc[a][c]);      // correctly rounded: hipcc's default for fp32 sqrt
        }
}

// ---- the diagonal (align="frame") --------------------------------------------------------------------------------------------------------
constexpr int MD_THREADS = 256;

__global__ __launch_bounds__(MD_THREADS) void metric_diagonal_kernel(const float* __restrict__ cost, const int32_t* __restrict__ x_len,
                                                                      const int32_t* __restrict__ y_len, int Ts, int Tr, float* __restrict__ total,
                                                                      int32_t* __restrict__ path_len) {
    __shared__ float dg[MT_MAX_SIDE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(clampi(x_len[b], 1, Ts), clampi(y_len[b], 1, Tr));
    const float* c = cost + (size_t)b * Ts * Tr;
    for (int j = tid; j < n; j += MD_THREADS) dg[j] = c[(size_t)j * Tr + j];
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int j = 0; j < n; ++j) s += dg[j];
        total[b] = s;
        path_len[b] = n;
    }
}

// ---- F0 statistics -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void metric_f0_kernel(const float* __restrict__ f0_syn, const float* __restrict__ f0_rec,
                                                        const int32_t* __restrict__ row, const int32_t* __restrict__ x_len,
                                                        const int32_t* __restrict__ y_len, int Ts, int Tr, int32_t* __restrict__ counts,
                                                        float* __restrict__ vals) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int xl = clampi(x_len[b], 1, Ts), yl = clampi(y_len[b], 1, Tr);
    const float* fs = f0_syn + (size_t)b * Ts;
    const float* fr = f0_rec + (size_t)b * Tr;
    const int32_t* rw = row ? row + (size_t)b * Tr : nullptr;
    int n_vv = 0, n_gpe = 0, n_vde = 0;
    double sx = 0.0, sy = 0.0;
    for (int j = lane; j < yl; j += 64) {
        const int i = rw ? clampi(rw[j], 0, xl - 1) : min(j, xl - 1);
        const float a = fs[i], r = fr[j];
        const bool va = a != 0.f, vr = r != 0.f;
        n_vde += va != vr;
        if (va && vr) {
            ++n_vv;
            const float d = a - r, lim = 0.2f * r;          // one subtract, one multiply, one compare
            n_gpe += fabsf(d) > lim;
            sx += (double)a;
            sy += (double)r;
        }
    }
    n_vv = wave_sum(n_vv);
    n_gpe = wave_sum(n_gpe);
    n_vde = wave_sum(n_vde);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    if (lane == 0) {
        int32_t* c = counts + (size_t)b * 4;
        c[0] = yl;
        c[1] = n_vv;
        c[2] = n_gpe;
        c[3] = n_vde;
    }
    float* out = vals + (size_t)b * 3;
    if (n_vv == 0) {
        if (lane < 3) out[lane] = __int_as_float(0x7fc00000);
        return;
    }
    const double mx = sx / (double)n_vv, my = sy / (double)n_vv;
    double se2 = 0.0, sae = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int j = lane; j < yl; j += 64) {
        const int i = rw ? clampi(rw[j], 0, xl - 1) : min(j, xl - 1);
        const float a = fs[i], r = fr[j];
        if (a != 0.f && r != 0.f) {
            const double x = (double)a, y = (double)r;
            const double e = 1200.0 * log2(x / y);
            const double dx = x - mx, dy = y - my;
            se2 += e * e;
            sae += fabs(e);
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
        }
    }
    se2 = wave_sum(se2);
    sae = wave_sum(sae);
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
    sxy = wave_sum(sxy);
    if (lane == 0) {
        out[0] = (float)sqrt(se2 / (double)n_vv);
        out[1] = (float)(sae / (double)n_vv);
        out[2] = sxx > 0.0 && syy > 0.0 ? (float)(sxy / sqrt(sxx * syy)) : __int_as_float(0x7fc00000);
    }
}

// ---- the column-normalised images ------------------------------------------------------------------------------------------------------
constexpr int MP_GROUPS = 4, MP_THREADS = MP_GROUPS * MT_CH;

__global__ __launch_bounds__(MP_THREADS) void metric_prepare_kernel(const float* __restrict__ cx, const float* __restrict__ cy,
                                                                     const int32_t* __restrict__ row, const int32_t* __restrict__ x_len,
                                                                     const int32_t* __restrict__ y_len, int Ts, int Tr, int n_cep, int C,
                                                                     float* __restrict__ u, float* __restrict__ v, float* __restrict__ minmax) {
    __shared__ double part[2][MP_GROUPS][MT_CH];
    __shared__ double norm[2][MT_CH];
    __shared__ float lo_s[MP_THREADS], hi_s[MP_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, k = tid % MT_CH, g = tid / MT_CH;
    const int xl = clampi(x_len[b], 1, Ts), yl = clampi(y_len[b], 1, Tr);
    const float* xb = cx + (size_t)b * Ts * n_cep;
    const float* yb = cy + (size_t)b * Tr * n_cep;
    const int32_t* rw = row ? row + (size_t)b * Tr : nullptr;
    if (k < C) {
        double sa = 0.0, sb = 0.0;
        for (int j = g; j < yl; j += MP_GROUPS) {
            const int i = rw ? clampi(rw[j], 0, xl - 1) : min(j, xl - 1);
            const double a = (double)xb[(size_t)i * n_cep + k], r = (double)yb[(size_t)j * n_cep + k];
            sa += a * a;
            sb += r * r;
        }
        part[0][g][k] = sa;
        part[1][g][k] = sb;
    }
    __syncthreads();
    if (g < 2 && k < C) norm[g][k] = sqrt((part[g][0][k] + part[g][1][k]) + (part[g][2][k] + part[g][3][k]));
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    float* ub = u + (size_t)b * Tr * C;
    float* vb = v + (size_t)b * Tr * C;
    for (int e = tid; e < yl * C; e += MP_THREADS) {
        const int j = e / C, c = e - j * C;
        const int i = rw ? clampi(rw[j], 0, xl - 1) : min(j, xl - 1);
        const double na = norm[0][c], nr = norm[1][c];
        const float qa = na > 0.0 ? (float)((double)xb[(size_t)i * n_cep + c] / na) : 0.f;
        const float qr = nr > 0.0 ? (float)((double)yb[(size_t)j * n_cep + c] / nr) : 0.f;
        ub[e] = qa;
        vb[e] = qr;
        lo = fminf(lo, fminf(qa, qr));
        hi = fmaxf(hi, fmaxf(qa, qr));
    }
    lo_s[tid] = lo;
    hi_s[tid] = hi;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < MP_THREADS; ++t) {
            lo = fminf(lo, lo_s[t]);
            hi = fmaxf(hi, hi_s[t]);
        }
        minmax[(size_t)b * 2] = lo;
        minmax[(size_t)b * 2 + 1] = hi;
    }
}

// ---- structural similarity -----------------------------------------------------------------------------------------------------------------
constexpr int MS_THREADS = 256, MS_IN = MT_SSIM_ROWS + MT_WIN - 1, MS_LD = MT_CH + 1;

struct SsimWindow {
    double g[MT_WIN];
};

__global__ __launch_bounds__(MS_THREADS) void metric_ssim_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  const int32_t* __restrict__ y_len, int Tr, int C, const float* __restrict__ range,
                                                                  SsimWindow win, int ntiles, double* __restrict__ partial) {
    __shared__ float us[MS_IN * MS_LD], vs[MS_IN * MS_LD];
    __shared__ double mom[5][MT_SSIM_ROWS * MS_LD];
    __shared__ double red[MS_THREADS];
    const int b = blockIdx.y, ti = blockIdx.x, tid = threadIdx.x;
    const int yl = clampi(y_len[b], 1, Tr);
    const int nwr = yl - (MT_WIN - 1), r0 = ti * MT_SSIM_ROWS;      // window rows of the pair, the first of this tile
    if (C < MT_WIN || r0 >= nwr) return;
    const int rows = min(MT_SSIM_ROWS, nwr - r0), in_rows = rows + MT_WIN - 1;      // r0 + in_rows <= yl
    const float* ub = u + ((size_t)b * Tr + r0) * C;
    const float* vb = v + ((size_t)b * Tr + r0) * C;
    for (int e = tid; e < in_rows * C; e += MS_THREADS) {
        const int r = e / C, c = e - r * C;
        us[r * MS_LD + c] = ub[e];
        vs[r * MS_LD + c] = vb[e];
    }
    __syncthreads();
    for (int e = tid; e < rows * C; e += MS_THREADS) {
        const int r = e / C, c = e - r * C;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int t = 0; t < MT_WIN; ++t) {
            const double a = (double)us[(r + t) * MS_LD + c], q = (double)vs[(r + t) * MS_LD + c], w = win.g[t];
            m0 += w * a;
            m1 += w * q;
            m2 += w * (a * a);
            m3 += w * (q * q);
            m4 += w * (a * q);
        }
        mom[0][r * MS_LD + c] = m0;
        mom[1][r * MS_LD + c] = m1;
        mom[2][r * MS_LD + c] = m2;
        mom[3][r * MS_LD + c] = m3;
        mom[4][r * MS_LD + c] = m4;
    }
    __syncthreads();
    const double L = (double)range[0];
    const double k1 = 0.01 * L, k2 = 0.03 * L;
    const double c1 = k1 * k1, c2 = k2 * k2;
    const int wc = C - (MT_WIN - 1);
    double acc = 0.0;
    for (int e = tid; e < rows * wc; e += MS_THREADS) {
        const int r = e / wc, c = e - r * wc;
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < MT_WIN; ++t) s += win.g[t] * mom[q][r * MS_LD + c + t];
            m[q] = s;
        }
        const double mxy = m[0] * m[1], mxx = m[0] * m[0], myy = m[1] * m[1];
        const double num = (2.0 * mxy + c1) * (2.0 * (m[4] - mxy) + c2);
        const double den = (mxx + myy + c1) * ((m[2] - mxx) + (m[3] - myy) + c2);
        acc += num / den;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = MS_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)b * ntiles + ti] = red[0];
}

__global__ __launch_bounds__(64) void metric_ssim_join_kernel(const double* __restrict__ partial, const int32_t* __restrict__ y_len, int Tr, int C,
                                                               int ntiles, float* __restrict__ ssim) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nwr = clampi(y_len[b], 1, Tr) - (MT_WIN - 1);
    if (C < MT_WIN || nwr < 1) {
        if (lane == 0) ssim[b] = __int_as_float(0x7fc00000);
        return;
    }
    const int nt = (nwr + MT_SSIM_ROWS - 1) / MT_SSIM_ROWS;      // <= ntiles: nwr <= Tr - 10
    double s = 0.0;
    for (int t = lane; t < nt; t += 64) s += partial[(size_t)b * ntiles + t];
    s = wave_sum(s);
    if (lane == 0) ssim[b] = (float)(s / ((double)nwr * (double)(C - (MT_WIN - 1))));
}

bool metric_sides(int B, int Ts, int Tr) { return B >= 1 && B <= MT_MAX_B && Ts >= 1 && Ts <= MT_MAX_SIDE && Tr >= 1 && Tr <= MT_MAX_SIDE; }

int launched(const std::string& who) { return hipGetLastError() == hipSuccess ? 0 : fail(CMTTS_E_HIP, who + ": launch failed"); }

const char* const kSides = ": 1 <= B <= 65535 and 1 <= Ts, Tr <= 4096";

}  // namespace

// ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int cmtts_metric_dct_table(int n_mels, int n_cep, float* table) {
    const std::string who = "cmtts_metric_dct_table";
    if (!table) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (n_mels != MT_CH) return fail(CMTTS_E_INVALID, who + ": n_mels must be 80");
    if (n_cep < 1 || n_cep > MT_CH) return fail(CMTTS_E_INVALID, who + ": 1 <= n_cep <= 80");
    const double N = (double)n_mels, pi = 3.141592653589793;
    const double s0 = sqrt(1.0 / N), s = sqrt(2.0 / N);
    for (int n = 0; n < n_mels; ++n)
        for (int k = 0; k < n_cep; ++k) {
            const double arg = pi * ((double)n + 0.5) * (double)k / N;
            table[(size_t)n * n_cep + k] = k == 0 ? (float)s0 : (float)(s * cos(arg));
        }
    return 0;
}

size_t cmtts_metric_workspace_bytes(int B, int Tr, int C) {
    if (B < 1 || B > MT_MAX_B || Tr < 1 || Tr > MT_MAX_SIDE || C < 1 || C > MT_CH) return 0;
    return ((size_t)B * metric_ssim_tiles(Tr) * sizeof(double) + 255) & ~(size_t)255;
}

int cmtts_metric_cepstra(const float* mel, const int32_t* lens, const float* table, int B, int T, int n_mels, int n_cep, float* cepstra,
                         void* stream) {
    const std::string who = "cmtts_metric_cepstra";
    if (!mel || !lens || !table || !cepstra) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (n_mels != MT_CH) return fail(CMTTS_E_INVALID, who + ": n_mels must be 80");
    if (n_cep < 1 || n_cep > MT_CH) return fail(CMTTS_E_INVALID, who + ": 1 <= n_cep <= 80");
    if (B < 1 || B > MT_MAX_B || T < 1 || T > MT_MAX_SIDE) return fail(CMTTS_E_INVALID, who + ": 1 <= B <= 65535 and 1 <= T <= 4096");
    hipLaunchKernelGGL(metric_cepstra_kernel, dim3((T + MC_FRAMES - 1) / MC_FRAMES, B), dim3(MC_THREADS), 0, (hipStream_t)stream, mel, lens, table, T,
                       n_cep, cepstra);
    return launched(who);
}

int cmtts_metric_cost(const float* cx, const int32_t* x_len, int Ts, const float* cy, const int32_t* y_len, int Tr, int B, int n_cep, int k_lo,
                      int k_hi, float* cost, void* stream) {
    const std::string who = "cmtts_metric_cost";
    if (!cx || !x_len || !cy || !y_len || !cost) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!metric_sides(B, Ts, Tr)) return fail(CMTTS_E_INVALID, who + kSides);
    if (n_cep < 1 || n_cep > MT_CH || k_lo < 0 || k_lo > k_hi || k_hi >= n_cep) return fail(CMTTS_E_INVALID, who + ": 1 <= n_cep <= 80 and 0 <= k_lo <= k_hi < n_cep");
    hipLaunchKernelGGL(metric_cost_kernel, dim3((Tr + MK_TILE - 1) / MK_TILE, (Ts + MK_TILE - 1) / MK_TILE, B), dim3(MK_THREADS), 0, (hipStream_t)stream,
                       cx, cy, x_len, y_len, Ts, Tr, n_cep, k_lo, k_hi - k_lo + 1, cost);
    return launched(who);
}

int cmtts_metric_diagonal(const float* cost, const int32_t* x_len, const int32_t* y_len, int B, int Ts, int Tr, float* total, int32_t* path_len,
                          void* stream) {
    const std::string who = "cmtts_metric_diagonal";
    if (!cost || !x_len || !y_len || !total || !path_len) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!metric_sides(B, Ts, Tr)) return fail(CMTTS_E_INVALID, who + kSides);
    hipLaunchKernelGGL(metric_diagonal_kernel, dim3(B), dim3(MD_THREADS), 0, (hipStream_t)stream, cost, x_len, y_len, Ts, Tr, total, path_len);
    return launched(who);
}

int cmtts_metric_f0(const float* f0_syn, const int32_t* x_len, int Ts, const float* f0_rec, const int32_t* y_len, int Tr, const int32_t* row, int B,
                    int32_t* counts, float* vals, void* stream) {
    const std::string who = "cmtts_metric_f0";
    if (!f0_syn || !x_len || !f0_rec || !y_len || !counts || !vals) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!metric_sides(B, Ts, Tr)) return fail(CMTTS_E_INVALID, who + kSides);
    hipLaunchKernelGGL(metric_f0_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, f0_syn, f0_rec, row, x_len, y_len, Ts, Tr, counts, vals);
    return launched(who);
}

int cmtts_metric_ssim_prepare(const float* cx, const int32_t* x_len, int Ts, const float* cy, const int32_t* y_len, int Tr, const int32_t* row, int B,
                              int n_cep, int C, float* u, float* v, float* minmax, void* stream) {
    const std::string who = "cmtts_metric_ssim_prepare";
    if (!cx || !x_len || !cy || !y_len || !u || !v || !minmax) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!metric_sides(B, Ts, Tr)) return fail(CMTTS_E_INVALID, who + kSides);
    if (n_cep < 1 || n_cep > MT_CH || C < 1 || C > n_cep) return fail(CMTTS_E_INVALID, who + ": 1 <= C <= n_cep <= 80");
    hipLaunchKernelGGL(metric_prepare_kernel, dim3(B), dim3(MP_THREADS), 0, (hipStream_t)stream, cx, cy, row, x_len, y_len, Ts, Tr, n_cep, C, u, v, minmax);
    return launched(who);
}

int cmtts_metric_ssim(const float* u, const float* v, const int32_t* y_len, int B, int Tr, int C, const float* range, float* ssim, void* ws,
                      size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_metric_ssim";
    if (!u || !v || !y_len || !range || !ssim) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (B < 1 || B > MT_MAX_B || Tr < 1 || Tr > MT_MAX_SIDE) return fail(CMTTS_E_INVALID, who + ": 1 <= B <= 65535 and 1 <= Tr <= 4096");
    if (C < 1 || C > MT_CH) return fail(CMTTS_E_INVALID, who + ": 1 <= C <= 80");
    if (!ws || ws_bytes < cmtts_metric_workspace_bytes(B, Tr, C)) return fail(CMTTS_E_WORKSPACE, who + ": workspace too small");
    SsimWindow win;
    double sum = 0.0;
    for (int t = 0; t < MT_WIN; ++t) {
        const double d = (double)(t - MT_WIN / 2);
        win.g[t] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += win.g[t];
    }
    for (int t = 0; t < MT_WIN; ++t) win.g[t] /= sum;
    const int ntiles = metric_ssim_tiles(Tr);
    double* partial = (double*)ws;
    hipLaunchKernelGGL(metric_ssim_kernel, dim3(ntiles, B), dim3(MS_THREADS), 0, (hipStream_t)stream, u, v, y_len, Tr, C, range, win, ntiles, partial);
    hipLaunchKernelGGL(metric_ssim_join_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)partial, y_len, Tr, C, ntiles, ssim);
    return launched(who);
}

}  // extern "C"
