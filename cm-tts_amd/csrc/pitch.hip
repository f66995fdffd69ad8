// Pitch of a recording (include/cmtts_hip.h: cmtts_pitch_*; definition: cmtts_amd/pitch.py).
//
//   nacf       a workgroup owns PT_FPB consecutive frames of one row and stages their W + (PT_FPB - 1) hop samples once (zeros outside the
//              clip); a wave owns one frame: mean in double (lane-strided partial sums, xor butterfly), pk, the windowed samples into the
//              wave's own LDS row, zeros behind them.  The autocorrelation in the direct form: lane l owns the LPL consecutive lags
//              LPL l .. LPL l + LPL - 1 and walks the samples eight at a time — x[i .. i + 7] is a broadcast read, the lane's window
//              x[i + LPL l .. i + LPL l + LPL + 6] is read at a stride of LPL floats across the lanes — 20 LDS reads for 8 LPL products.
//              Eight products are one fused float chain; the chains are added up in double in ascending order: no atomics, a frame's
//              bits depend on its own samples alone.
//   candidates a wave per frame: lane l looks at lags l, l + 64, ..; NC rounds of a wave arg-max on (strength, smaller lag), the winner's
//              lane retiring it; the winners ranked by lag.
//   viterbi    one wave per row, lane c is state c.  A step reads the previous D and lg of states 0 .. 8 by v_readlane (constant lanes:
//              scalars, no LDS on the dependent chain) in ascending order; the frames' candidates (strength and lg, as the candidates launch
//              left them) are loaded eight frames ahead, state 0's strengths are made by all lanes before the chain starts.
//              Back-pointers: one byte per state and frame in LDS (36 KiB); the walk back runs on them in the same launch,
//              exactly n - 1 steps whatever r holds, then every lane writes lag and f0 of its frames.
//   targets    a workgroup per (row, scale); each recomputes the row's cheap prologue in the same fixed order (voiced neighbours by two
//              scans, fill and interpolation, log, mean and std in double by a fixed tree), then the direct circular form against the
//              table of the row's own N in LDS: chains of eight float products added up in double.
// Vector stores only.  Contraction is off for the whole unit: the tracker's float operations are the definition's, one rounding each;
// where a fused multiply-add is meant it is written as fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "launch.h"
#include "model.h"
#include "pitch.h"

#pragma clang fp contract(off)

namespace {

constexpr float PT_VT = 0.6f, PT_ST = 0.03f, PT_OC = 0.01f, PT_OJC = 0.35f, PT_VUC = 0.14f;
constexpr float PT_K = (1.0f + PT_VT) / PT_ST;                // float arithmetic, as the definition's

__device__ __forceinline__ int pt_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float pt_readlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// ---- nacf ------------------------------------------------------------------------------------------------------------------------------
constexpr int PN_THREADS = 64 * PT_FPB;

__host__ __device__ inline int pn_wp(int W) { return (W + 7) & ~7; }
__host__ __device__ inline int pn_stage(const PitchGeometry& g) { return (g.W + (PT_FPB - 1) * g.hop + 3) & ~3; }
template <int LPL>
__host__ __device__ inline int pn_row(int W) { return pn_wp(W) + 64 * LPL; }

template <bool I16, int LPL>
__global__ __launch_bounds__(PN_THREADS) void pitch_nacf_kernel(const PitchTables t, const void* __restrict__ wav, long ld,
                                                                const int32_t* __restrict__ n_valid, int T, float* __restrict__ r,
                                                                float* __restrict__ pk, int32_t* __restrict__ frames) {
    extern __shared__ float sm[];
    const int W = t.g.W, hop = t.g.hop, L2 = t.g.lmax + 2, Wp = pn_wp(W), XL = pn_row<LPL>(W);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.y, fb = blockIdx.x * PT_FPB;
    const long nv = n_valid[row];
    const int n = (int)(nv < 0 ? 0 : (nv > ld ? ld : nv));
    const int F = min(1 + n / hop, T);
    if (blockIdx.x == 0 && tid == 0) frames[row] = F;
    float* stage = sm;
    float* xs = sm + pn_stage(t.g) + w * XL;
    const int f = fb + w;

    if (fb < F) {                                             // uniform per workgroup
        const int SL = W + (PT_FPB - 1) * hop;
        const long g0 = (long)fb * hop - W / 2;
        for (int j = tid; j < SL; j += PN_THREADS) {
            const long gi = g0 + j;
            float v = 0.f;
            if (gi >= 0 && gi < n) {
                if (I16) v = (float)reinterpret_cast<const int16_t*>(wav)[row * ld + gi] * (1.0f / 32768.0f);
                else v = fminf(fmaxf(reinterpret_cast<const float*>(wav)[row * ld + gi], -1.0f), 1.0f);
            }
            stage[j] = v;
        }
        __syncthreads();
        // this wave's frame (a frame at or beyond F: computed on what was staged, never stored)
        const float* s = stage + w * hop;
        double sum = 0.0;
        for (int i = lane; i < W; i += 64) sum += (double)s[i];
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
        const double mean = sum / (double)W;
        double mx = 0.0;
        for (int i = lane; i < W; i += 64) {
            const double xd = (double)s[i] - mean;
            mx = fmax(mx, fabs(xd));
            xs[i] = (float)(xd * (double)t.window[i]);
        }
        for (int i = W + lane; i < XL; i += 64) xs[i] = 0.f;
        for (int d = 32; d; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
        __syncthreads();

        double acc[LPL];
#pragma unroll
        for (int l = 0; l < LPL; ++l) acc[l] = 0.0;
        const float* xw = xs + LPL * lane;
        for (int i0 = 0; i0 < Wp; i0 += 8) {
            const float4 a = *reinterpret_cast<const float4*>(xs + i0), b = *reinterpret_cast<const float4*>(xs + i0 + 4);
            const float xi[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            float wv[LPL + 7];
#pragma unroll
            for (int k = 0; k < LPL + 7; ++k) wv[k] = xw[i0 + k];
#pragma unroll
            for (int l = 0; l < LPL; ++l) {
                float p = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) p = fmaf(xi[k], wv[k + l], p);
                acc[l] += (double)p;
            }
        }
        const double a0 = __shfl(acc[0], 0);
        if (f < F) {
            float* out = r + ((long)row * T + f) * L2;
#pragma unroll
            for (int l = 0; l < LPL; ++l) {
                const int tau = LPL * lane + l;
                if (tau < L2) out[tau] = a0 > 0.0 ? (float)(acc[l] / a0 / t.rw[tau]) : 0.f;
            }
            if (lane == 0) pk[(long)row * T + f] = (float)mx;
        }
    }
    // the group's frames at and beyond F: zeros
    for (int fw = 0; fw < PT_FPB; ++fw) {
        const int ff = fb + fw;
        if (ff < F || ff >= T) continue;
        for (int j = tid; j < L2; j += PN_THREADS) r[((long)row * T + ff) * L2 + j] = 0.f;
        if (tid == 0) pk[(long)row * T + ff] = 0.f;
    }
}

// ---- candidates --------------------------------------------------------------------------------------------------------------------------
constexpr int PC_FPB = 4;
constexpr int PC_KPL = PT_MAX_LAGS / 64;                      // lags a lane looks at

__global__ __launch_bounds__(64 * PC_FPB) void pitch_candidates_kernel(const PitchTables t, const float* __restrict__ r,
                                                                      const int32_t* __restrict__ frames, int T, int32_t* __restrict__ cand_lag,
                                                                      float* __restrict__ cand_str, float* __restrict__ cand_lg) {
    const int lane = threadIdx.x & 63, b = blockIdx.y, f = blockIdx.x * PC_FPB + (threadIdx.x >> 6);
    const int n = pt_clampi(frames[b], 0, T);
    if (f >= n) return;                                       // uniform per wave; no barrier below
    const int L2 = t.g.lmax + 2;
    const float* rr = r + ((long)b * T + f) * L2;
    const float ninf = -INFINITY;
    float s[PC_KPL];
#pragma unroll
    for (int k = 0; k < PC_KPL; ++k) {
        const int tau = lane + 64 * k;
        s[k] = ninf;
        if (tau >= t.g.lmin && tau <= t.g.lmax) {
            const float c = rr[tau], lo = rr[tau - 1], hi = rr[tau + 1];
            if (c > lo && c >= hi && c > 0.f) {
                const float d = t.lg[tau] - t.lg_floor;
                const float oc = PT_OC * d;
                s[k] = c - oc;
            }
        }
    }
    float sel_s[PT_NC];
    int sel_l[PT_NC];
    int cnt = 0;
#pragma unroll
    for (int rd = 0; rd < PT_NC; ++rd) {
        float bs = ninf;
        int bl = INT32_MAX;
#pragma unroll
        for (int k = 0; k < PC_KPL; ++k)
            if (s[k] > bs) { bs = s[k]; bl = lane + 64 * k; }
        for (int d = 32; d; d >>= 1) {
            const float os = __shfl_xor(bs, d);
            const int ol = __shfl_xor(bl, d);
            if (os > bs || (os == bs && ol < bl)) { bs = os; bl = ol; }
        }
        sel_s[rd] = bs;
        sel_l[rd] = bl;
        if (bl != INT32_MAX) {
            ++cnt;
#pragma unroll
            for (int k = 0; k < PC_KPL; ++k)
                if (bl == lane + 64 * k) s[k] = ninf;
        }
    }
    // lane j < 8: winner j goes to the slot of its rank by lag; the slots from cnt on hold (0, -inf)
    if (lane < PT_NC) {
        float ms = ninf;
        int ml = INT32_MAX;
#pragma unroll
        for (int i = 0; i < PT_NC; ++i)
            if (i == lane) { ms = sel_s[i]; ml = sel_l[i]; }
        int rank = 0;
#pragma unroll
        for (int i = 0; i < PT_NC; ++i) rank += sel_l[i] < ml ? 1 : 0;
        const int slot = lane < cnt ? rank : lane;
        const long o = ((long)b * T + f) * PT_NC + slot;
        cand_lag[o] = lane < cnt ? ml : 0;
        cand_str[o] = lane < cnt ? ms : ninf;
        cand_lg[o] = t.lg[lane < cnt ? ml : 0];                // lg[0] = 0
    }
}

// ---- viterbi ---------------------------------------------------------------------------------------------------------------------------
constexpr int PV_AHEAD = 8;

__global__ __launch_bounds__(64) void pitch_viterbi_kernel(const PitchTables t, const float* __restrict__ r, const float* __restrict__ pk,
                                                           const int32_t* __restrict__ frames, int T, const int32_t* __restrict__ cand_lag,
                                                           const float* __restrict__ cand_str, const float* __restrict__ cand_lg,
                                                           int32_t* __restrict__ lag_out,
                                                           float* __restrict__ f0_out) {
    __shared__ uint8_t bp[PT_MAX_T * PT_STATES];
    __shared__ uint8_t st[PT_MAX_T];
    __shared__ float us[PT_MAX_T];                            // state 0's strength per frame
    const int lane = threadIdx.x, c = lane, b = blockIdx.x;
    const int n = pt_clampi(frames[b], 0, T);
    const int L2 = t.g.lmax + 2;
    const float ninf = -INFINITY;
    const float* pkb = pk + (long)b * T;
    const int32_t* cl = cand_lag + (long)b * T * PT_NC;
    const float* cs = cand_str + (long)b * T * PT_NC;
    const float* clg = cand_lg + (long)b * T * PT_NC;
    float gpk = 0.f;                                          // the largest pk that is a number: an exact max, any order
    for (int f = lane; f < n; f += 64) {
        const float v = pkb[f];
        if (v > gpk) gpk = v;
    }
    for (int d = 32; d; d >>= 1) {
        const float o = __shfl_xor(gpk, d);
        if (o > gpk) gpk = o;
    }
    for (int f = lane; f < n; f += 64) {                      // off the dependent chain, every lane its frames
        float u = PT_VT;
        if (gpk > 0.f) {
            const float q = (float)((double)pkb[f] / (double)gpk);          // correctly rounded: 53 >= 2 * 24 + 2 bits
            const float m = q * PT_K;
            const float d = 2.0f - m;
            u = PT_VT + (d > 0.f ? d : 0.f);
        }
        us[f] = u;
    }
    __syncthreads();

    // this lane's state in frame f: (strength, lg of its lag); absent states hold -inf (pitch_candidates_kernel wrote it)
    auto load = [&](int f, float& s, float& lg) {
        s = ninf;
        lg = 0.f;
        if (f >= n || c >= PT_STATES) return;
        if (c == 0) {
            s = us[f];
        } else {
            s = cs[(long)f * PT_NC + c - 1];
            lg = clg[(long)f * PT_NC + c - 1];
        }
    };

    float D = ninf, lgp = 0.f;
    float cs_[PV_AHEAD], lg_[PV_AHEAD], ns_[PV_AHEAD], nl_[PV_AHEAD];
#pragma unroll
    for (int u = 0; u < PV_AHEAD; ++u) load(u, cs_[u], lg_[u]);
    for (int f0 = 0; f0 < n; f0 += PV_AHEAD) {
#pragma unroll
        for (int u = 0; u < PV_AHEAD; ++u) load(f0 + PV_AHEAD + u, ns_[u], nl_[u]);
#pragma unroll
        for (int u = 0; u < PV_AHEAD; ++u) {
            const int f = f0 + u;
            if (f < n) {                                      // uniform
                const float str = cs_[u], lgc = lg_[u];
                const bool absent = c != 0 && !(str > ninf);  // a present candidate's strength is never -inf (and never NaN)
                float Dn;
                int bi = 0;
                if (f == 0) {
                    Dn = str;
                } else {
                    const float D0 = pt_readlane(D, 0);
                    float best = c == 0 ? D0 : D0 - PT_VUC;
#pragma unroll
                    for (int p = 1; p < PT_STATES; ++p) {
                        const float Dp = pt_readlane(D, p), lp = pt_readlane(lgp, p);
                        const float dl = lp - lgc;
                        const float oj = PT_OJC * fabsf(dl);
                        const float tc = c == 0 ? PT_VUC : oj;
                        const float v = Dp - tc;
                        if (v > best) { best = v; bi = p; }
                    }
                    Dn = best + str;
                }
                if (absent) { Dn = ninf; bi = 0; }
                if (c < PT_STATES) bp[f * PT_STATES + c] = (uint8_t)bi;
                D = Dn;
                lgp = lgc;
            }
        }
#pragma unroll
        for (int u = 0; u < PV_AHEAD; ++u) { cs_[u] = ns_[u]; lg_[u] = nl_[u]; }
    }
    __syncthreads();
    if (n > 0) {
        int cb = 0;
        float top = pt_readlane(D, 0);
#pragma unroll
        for (int k = 1; k < PT_STATES; ++k) {
            const float Dk = pt_readlane(D, k);
            if (Dk > top) { top = Dk; cb = k; }
        }
        for (int f = n - 1; f >= 0; --f) {                    // every lane the same walk (broadcast reads); lane 0 records
            if (lane == 0) st[f] = (uint8_t)cb;
            cb = min((int)bp[f * PT_STATES + cb], PT_STATES - 1);
        }
    }
    __syncthreads();
    for (int f = lane; f < T; f += 64) {
        int l = 0;
        float fz = 0.f;
        if (f < n) {
            const int s = st[f];
            if (s > 0) l = cl[(long)f * PT_NC + s - 1];
            if (l > 0) {
                const int lc = pt_clampi(l, 1, L2 - 2);
                const float* rr = r + ((long)b * T + f) * L2;
                const float a = rr[lc - 1], bb = rr[lc], cc = rr[lc + 1];
                const float den = (a - 2.0f * bb) + cc;
                float d = 0.f;
                if (den < 0.f) d = (0.5f * (a - cc)) / den;
                fz = (float)t.g.fs / ((float)l + d);
            }
        }
        lag_out[(long)b * T + f] = l;
        f0_out[(long)b * T + f] = fz;
    }
}

// ---- targets ---------------------------------------------------------------------------------------------------------------------------
constexpr int PG_THREADS = 256;
constexpr int PG_NONE = 0x7fff;

__device__ __forceinline__ double pg_tree_sum(double v, double* sc, int tid) {
    __syncthreads();
    sc[tid] = v;
    __syncthreads();
    for (int s = PG_THREADS / 2; s; s >>= 1) {
        if (tid < s) sc[tid] += sc[tid + s];
        __syncthreads();
    }
    return sc[0];
}

__global__ __launch_bounds__(PG_THREADS) void pitch_targets_kernel(const PitchTables t, const float* __restrict__ f0, const int32_t* __restrict__ frames,
                                                                   int T, float* __restrict__ cwt_spec, float* __restrict__ f0_mean,
                                                                   float* __restrict__ f0_std, uint8_t* __restrict__ uv, int32_t* __restrict__ status) {
    __shared__ double lf[PT_MAX_T];                           // log of the continuous contour; afterwards its first half holds the table
    __shared__ float xa[PT_MAX_T];                            // first the voiced neighbours (two int16 per frame), afterwards x
    __shared__ double sc[PG_THREADS];
    __shared__ int isc[PG_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x, j = blockIdx.y;
    const int n = pt_clampi(frames[b], 0, T);
    const float* fr = f0 + (long)b * T;
    float* out = cwt_spec + (long)b * T * PT_CWT_SCALES + j;
    int16_t* prv = reinterpret_cast<int16_t*>(xa);
    int16_t* nxt = prv + PT_MAX_T;
    float* h = reinterpret_cast<float*>(lf);

    if (j == 0)
        for (int f = tid; f < T; f += PG_THREADS) uv[(long)b * T + f] = f < n && fr[f] == 0.f ? 1 : 0;

    int stat = 0;
    double mean = 0.0, sd = 1.0;
    if (n < 3) {
        stat = 3;
    } else {
        // the last voiced frame at or before f and the first at or after it: a run of consecutive frames per thread, the runs joined by scans
        const int per = (n + PG_THREADS - 1) / PG_THREADS;
        const int s0 = min(tid * per, n), s1 = min(s0 + per, n);
        int last = -1, first = PG_NONE;
        for (int f = s0; f < s1; ++f)
            if (fr[f] != 0.f) { last = f; if (first == PG_NONE) first = f; }
        isc[tid] = last;
        __syncthreads();
        for (int step = 1; step < PG_THREADS; step <<= 1) {   // inclusive max scan (integers: any order)
            const int o = tid >= step ? isc[tid - step] : -1;
            __syncthreads();
            isc[tid] = max(isc[tid], o);
            __syncthreads();
        }
        int cur = tid > 0 ? isc[tid - 1] : -1;
        const int any = isc[PG_THREADS - 1];
        __syncthreads();
        for (int f = s0; f < s1; ++f) {
            if (fr[f] != 0.f) cur = f;
            prv[f] = (int16_t)cur;
        }
        isc[tid] = first;
        __syncthreads();
        for (int step = 1; step < PG_THREADS; step <<= 1) {   // inclusive min scan from the right
            const int o = tid + step < PG_THREADS ? isc[tid + step] : PG_NONE;
            __syncthreads();
            isc[tid] = min(isc[tid], o);
            __syncthreads();
        }
        cur = tid + 1 < PG_THREADS ? isc[tid + 1] : PG_NONE;
        __syncthreads();
        for (int f = s1 - 1; f >= s0; --f) {
            if (fr[f] != 0.f) cur = f;
            nxt[f] = (int16_t)cur;
        }
        __syncthreads();
        if (any < 0) {
            stat = 1;
        } else {
            double lo = INFINITY, hi = -INFINITY;
            for (int f = tid; f < n; f += PG_THREADS) {
                const int p = prv[f], q = nxt[f];
                double y;
                if (p < 0) y = (double)fr[q];
                else if (q == PG_NONE) y = (double)fr[p];
                else if (p == q) y = (double)fr[f];
                else {
                    const double y0 = (double)fr[p], y1 = (double)fr[q];
                    const double slope = (y1 - y0) / (double)(q - p);
                    y = slope * (double)(f - p) + y0;
                }
                const double l = log(y);
                lf[f] = l;
                lo = fmin(lo, l);
                hi = fmax(hi, l);
            }
            __syncthreads();
            sc[tid] = lo;
            __syncthreads();
            for (int s = PG_THREADS / 2; s; s >>= 1) {
                if (tid < s) sc[tid] = fmin(sc[tid], sc[tid + s]);
                __syncthreads();
            }
            lo = sc[0];
            __syncthreads();
            sc[tid] = hi;
            __syncthreads();
            for (int s = PG_THREADS / 2; s; s >>= 1) {
                if (tid < s) sc[tid] = fmax(sc[tid], sc[tid + s]);
                __syncthreads();
            }
            hi = sc[0];
            if (lo == hi) {
                stat = 2;
                mean = lf[0];
            } else {
                double part = 0.0;
                for (int f = tid; f < n; f += PG_THREADS) part += lf[f];
                mean = pg_tree_sum(part, sc, tid) / (double)n;
                part = 0.0;
                for (int f = tid; f < n; f += PG_THREADS) {
                    const double d = lf[f] - mean;
                    part += d * d;
                }
                sd = sqrt(pg_tree_sum(part, sc, tid) / (double)n);
            }
        }
    }
    if (j == 0 && tid == 0) {
        f0_mean[b] = (float)mean;
        f0_std[b] = (float)sd;
        status[b] = stat;
    }
    if (stat != 0) {                                          // uniform per workgroup
        for (int f = tid; f < T; f += PG_THREADS) out[(long)f * PT_CWT_SCALES] = 0.f;
        return;
    }
    int N = PT_CWT_MIN_N;
    while (N < n) N <<= 1;
    const int n8 = (n + 7) & ~7;
    __syncthreads();                                          // prv / nxt are done with: x takes their place
    float xv[PT_MAX_T / PG_THREADS];
#pragma unroll
    for (int k = 0; k < PT_MAX_T / PG_THREADS; ++k) {
        const int f = tid + k * PG_THREADS;
        xv[k] = f < n ? (float)((lf[f] - mean) / sd) : 0.f;
    }
    __syncthreads();                                          // lf is done with: the table takes its place
#pragma unroll
    for (int k = 0; k < PT_MAX_T / PG_THREADS; ++k) {
        const int f = tid + k * PG_THREADS;
        if (f < n8) xa[f] = xv[k];
    }
    const float* src = t.cwt + (long)j * PT_CWT_LD + (N - PT_CWT_MIN_N);
    for (int m = tid; m < N; m += PG_THREADS) h[m] = src[m];
    __syncthreads();
    const int mask = N - 1;
    for (int f = tid; f < T; f += PG_THREADS) {
        float v = 0.f;
        if (f < n) {
            double acc = 0.0;
            for (int u0 = 0; u0 < n8; u0 += 8) {
                float p = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) p = fmaf(xa[u0 + k], h[(f - u0 - k) & mask], p);
                acc += (double)p;
            }
            v = (float)acc;
        }
        out[(long)f * PT_CWT_SCALES] = v;
    }
}

size_t pitch_ws_bytes(int B, int T) {
    Carver cv(nullptr);
    cv.take<int32_t>((size_t)B * T * PT_NC);
    cv.take<float>((size_t)B * T * PT_NC);
    cv.take<float>((size_t)B * T * PT_NC);
    return (cv.off + 255) & ~(size_t)255;
}

}  // namespace

extern "C" int cmtts_launch_pitch_nacf(const PitchTables* t, const void* wav, int is_int16, long ld, int rows, const int32_t* n_valid, int T, float* r,
                                       float* pk, int32_t* frames, void* stream) {
    if (rows < 1 || rows > PT_MAX_B || T < 1 || T > PT_MAX_T || ld < 1) return -2;
    const dim3 grid((T + PT_FPB - 1) / PT_FPB, rows), block(PN_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool narrow = t->g.lmax + 2 <= 5 * 64;
    const size_t lds = (size_t)(pn_stage(t->g) + PT_FPB * (narrow ? pn_row<5>(t->g.W) : pn_row<8>(t->g.W))) * sizeof(float);
    if (lds > 64 * 1024) return -2;
    if (narrow) {
        if (is_int16) hipLaunchKernelGGL((pitch_nacf_kernel<true, 5>), grid, block, lds, s, *t, wav, ld, n_valid, T, r, pk, frames);
        else hipLaunchKernelGGL((pitch_nacf_kernel<false, 5>), grid, block, lds, s, *t, wav, ld, n_valid, T, r, pk, frames);
    } else {
        if (is_int16) hipLaunchKernelGGL((pitch_nacf_kernel<true, 8>), grid, block, lds, s, *t, wav, ld, n_valid, T, r, pk, frames);
        else hipLaunchKernelGGL((pitch_nacf_kernel<false, 8>), grid, block, lds, s, *t, wav, ld, n_valid, T, r, pk, frames);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_pitch_track(const PitchTables* t, const float* r, const float* pk, const int32_t* frames, int B, int T, int32_t* cand_lag,
                                        float* cand_str, float* cand_lg, int32_t* lag, float* f0, void* stream) {
    if (B < 1 || B > PT_MAX_B || T < 1 || T > PT_MAX_T) return -2;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pitch_candidates_kernel, dim3((T + PC_FPB - 1) / PC_FPB, B), dim3(64 * PC_FPB), 0, s, *t, r, frames, T, cand_lag, cand_str, cand_lg);
    hipLaunchKernelGGL(pitch_viterbi_kernel, dim3(B), dim3(64), 0, s, *t, r, pk, frames, T, cand_lag, cand_str, cand_lg, lag, f0);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_pitch_targets(const PitchTables* t, const float* f0, const int32_t* frames, int B, int T, float* cwt_spec, float* f0_mean,
                                          float* f0_std, uint8_t* uv, int32_t* status, void* stream) {
    if (B < 1 || B > PT_MAX_B || T < 3 || T > PT_MAX_T) return -2;
    hipLaunchKernelGGL(pitch_targets_kernel, dim3(B, PT_CWT_SCALES), dim3(PG_THREADS), 0, (hipStream_t)stream, *t, f0, frames, T, cwt_spec, f0_mean,
                       f0_std, uv, status);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the handle and the C ABI ------------------------------------------------------------------------------------------------------------
struct cmtts_pitch {
    Allocs al;
    PitchTables t{};
};

extern "C" {

int cmtts_pitch_tables(int fs, int hop_length, double floor_hz, double ceiling_hz, int32_t* geometry, float* window, double* r_w, float* lg,
                       float* lg_floor, int cwt_n, float* cwt) {
    const std::string who = "cmtts_pitch_tables";
    PitchGeometry g;
    if (!geometry) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (pitch_geometry(fs, hop_length, floor_hz, ceiling_hz, &g) != 0)
        return fail(CMTTS_E_INVALID, who + ": unsupported geometry (fs >= 1, 1 <= hop <= 1024, 0 < floor < ceiling <= fs / 2, window <= 2048, lags <= 512)");
    geometry[0] = g.W;
    geometry[1] = g.lmin;
    geometry[2] = g.lmax;
    if (window || r_w) {
        std::vector<float> w(g.W);
        std::vector<double> rw(g.lmax + 2);
        pitch_window(g, w.data(), rw.data());
        if (window) std::copy(w.begin(), w.end(), window);
        if (r_w) std::copy(rw.begin(), rw.end(), r_w);
    }
    if (lg || lg_floor) {
        std::vector<float> l(g.lmax + 2);
        float lf = 0.f;
        pitch_lg(g, floor_hz, l.data(), &lf);
        if (lg) std::copy(l.begin(), l.end(), lg);
        if (lg_floor) *lg_floor = lf;
    }
    if (cwt) {
        if (cwt_n < PT_CWT_MIN_N || cwt_n > PT_CWT_MAX_N || (cwt_n & (cwt_n - 1))) return fail(CMTTS_E_INVALID, who + ": cwt_n must be a power of two in [4, 4096]");
        std::vector<float> all((size_t)PT_CWT_SCALES * PT_CWT_LD);
        pitch_cwt_tables(all.data());
        for (int j = 0; j < PT_CWT_SCALES; ++j)
            std::copy(all.begin() + (size_t)j * PT_CWT_LD + (cwt_n - PT_CWT_MIN_N), all.begin() + (size_t)j * PT_CWT_LD + (2 * cwt_n - PT_CWT_MIN_N),
                      cwt + (size_t)j * cwt_n);
    }
    return 0;
}

int cmtts_pitch_create(int fs, int hop_length, double floor_hz, double ceiling_hz, cmtts_pitch** out) {
    const std::string who = "cmtts_pitch_create";
    if (!out) return fail(CMTTS_E_INVALID, who + ": null argument");
    PitchGeometry g;
    if (pitch_geometry(fs, hop_length, floor_hz, ceiling_hz, &g) != 0)
        return fail(CMTTS_E_INVALID, who + ": unsupported geometry (fs >= 1, 1 <= hop <= 1024, 0 < floor < ceiling <= fs / 2, window <= 2048, lags <= 512)");
    std::vector<float> window(g.W), lg(g.lmax + 2), cwt((size_t)PT_CWT_SCALES * PT_CWT_LD);
    std::vector<double> rw(g.lmax + 2);
    float lg_floor = 0.f;
    pitch_window(g, window.data(), rw.data());
    pitch_lg(g, floor_hz, lg.data(), &lg_floor);
    pitch_cwt_tables(cwt.data());
    cmtts_pitch* p = new cmtts_pitch();
    auto up = [&](const void* h, size_t bytes, const void** dst) { return p->al.upload_bytes(h, bytes, (void**)dst); };
    int rc = up(window.data(), window.size() * sizeof(float), (const void**)&p->t.window);
    if (rc == 0) rc = up(rw.data(), rw.size() * sizeof(double), (const void**)&p->t.rw);
    if (rc == 0) rc = up(lg.data(), lg.size() * sizeof(float), (const void**)&p->t.lg);
    if (rc == 0) rc = up(cwt.data(), cwt.size() * sizeof(float), (const void**)&p->t.cwt);
    if (rc != 0) {
        p->al.release();
        delete p;
        return rc;
    }
    p->t.lg_floor = lg_floor;
    p->t.g = g;
    *out = p;
    return 0;
}

void cmtts_pitch_destroy(cmtts_pitch* p) {
    if (!p) return;
    p->al.release();
    delete p;
}

size_t cmtts_pitch_workspace_bytes(int B, int T) {
    if (B < 1 || B > PT_MAX_B || T < 1 || T > PT_MAX_T) return 0;
    return pitch_ws_bytes(B, T);
}

static int pitch_sides(const std::string& who, int B, int T, int t_min, const void* ws, size_t ws_bytes) {
    if (B < 1 || B > PT_MAX_B || T < t_min || T > PT_MAX_T)
        return fail(CMTTS_E_INVALID, who + ": 1 <= rows <= 65535 and " + std::to_string(t_min) + " <= T <= 4096");
    if (!ws || ws_bytes < cmtts_pitch_workspace_bytes(B, T)) return fail(CMTTS_E_WORKSPACE, who + ": workspace too small");
    return 0;
}

int cmtts_pitch_nacf(cmtts_pitch* p, const void* wav, int is_int16, int rows, int64_t ld, const int32_t* n_valid, int T, float* r, float* pk,
                     int32_t* frames, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_pitch_nacf";
    if (!p || !wav || !n_valid || !r || !pk || !frames) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (ld < 1 || ld > INT32_MAX / 2) return fail(CMTTS_E_INVALID, who + ": 1 <= ld < 2^30");
    CHK(pitch_sides(who, rows, T, 1, ws, ws_bytes));
    if (cmtts_launch_pitch_nacf(&p->t, wav, is_int16 != 0, (long)ld, rows, n_valid, T, r, pk, frames, stream) != 0)
        return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

int cmtts_pitch_track(cmtts_pitch* p, const float* r, const float* pk, const int32_t* frames, int B, int T, int32_t* lag, float* f0, void* ws,
                      size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_pitch_track";
    if (!p || !r || !pk || !frames || !lag || !f0) return fail(CMTTS_E_INVALID, who + ": null argument");
    CHK(pitch_sides(who, B, T, 1, ws, ws_bytes));
    Carver cv(ws);
    int32_t* cand_lag = cv.take<int32_t>((size_t)B * T * PT_NC);
    float* cand_str = cv.take<float>((size_t)B * T * PT_NC);
    float* cand_lg = cv.take<float>((size_t)B * T * PT_NC);
    if (cmtts_launch_pitch_track(&p->t, r, pk, frames, B, T, cand_lag, cand_str, cand_lg, lag, f0, stream) != 0) return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

int cmtts_pitch_targets(cmtts_pitch* p, const float* f0, const int32_t* frames, int B, int T, float* cwt_spec, float* f0_mean, float* f0_std,
                        uint8_t* uv, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_pitch_targets";
    if (!p || !f0 || !frames || !cwt_spec || !f0_mean || !f0_std || !uv || !status) return fail(CMTTS_E_INVALID, who + ": null argument");
    CHK(pitch_sides(who, B, T, 3, ws, ws_bytes));
    if (cmtts_launch_pitch_targets(&p->t, f0, frames, B, T, cwt_spec, f0_mean, f0_std, uv, status, stream) != 0)
        return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

}  // extern "C"
