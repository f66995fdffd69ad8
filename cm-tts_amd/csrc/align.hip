// Alignment of a recording to its phonemes by dynamic time warping (include/cmtts_hip.h: cmtts_align_*; definition:
// cmtts_amd/align.py).
//
//   cost       c[i][j] = sum_k (x[i][k] - y[j][k])^2 in the difference form on the VALU.  Per side and channel the mean over the valid frames
//              first, in double and in a fixed order (four interleaved partial sums per channel, joined as (0 + 1) + (2 + 3)).  A workgroup
//              owns a 64 x 64 tile of one pair, stages both sides' mean-removed 64 x 80 features in LDS and gives each thread a 4 x 4
//              micro-tile; the 80 terms are summed as ten fused chains of eight, added up in order (a single chain of 80 loses the bound:
//              DESIGN §3.5j).  Cells at or beyond a pair's lengths are neither read nor written.
//   dp         one workgroup per pair.  A wave carries a STRIP of 64 rows, one per lane, along the anti-diagonals: at step t lane l is at
//              column t - l.  D[i][j-1] is the lane's own previous value, D[i-1][j] comes from lane l - 1 by one cross-lane shift (DPP
//              wave_shr:1) and D[i-1][j-1] is the value that shift delivered one step earlier: no LDS and no wait on the dependent path.
//              Read from the matrix as it lies, a step's 64 cells are 64 cache lines (built first and measured: 390 ns per anti-diagonal
//              at 512 x 512), so a fully parallel launch first lays the cost out in the DP's own order, [strip][step][lane], through LDS tiles:
//              a step is then one 256-byte load, issued eight steps ahead.  Lane 0's neighbour above is the last row of the strip above:
//              that wave leaves it in an LDS ring, AL_SS columns of which the lower wave picks up per barrier interval (one read per
//              lane, handed to lane 0 by v_readlane).  Wave w starts AL_LAG intervals behind wave w - 1: lane 63 lags 63 steps, and an
//              interval's columns must be complete when it begins.  Up to 16 strips run at once; taller pairs go in bands of 16 strips,
//              the band's last row handed on through a full-length LDS row.  Per cell only the step code (one byte: diagonal / up /
//              left) is stored, four steps to a dword, in the same skewed order [t / 4][lane], so every store is one 256-byte line.  The
//              final D goes out once.
//   walk       wave 0 walks back from the end.  The codes around the current point — the strip's 64 lanes x 128 steps, 8 KiB — are staged in
//              LDS, read there (every lane the same address; v_readfirstlane makes the rest of the step scalar) until the walk leaves
//              them, at least 64 steps later, and only the run of rows per column is recorded.  At
//              most x_len + y_len - 2 steps whatever the data holds: on row 0 the walk goes left and on column 0 up without looking at
//              the code.  Then one thread per column picks row[j] from its run.
//   durations  per row the recording's frames of a phoneme are one run of columns (row[] does not decrease): two binary searches per phoneme
//              in LDS, then its costs summed with j ascending.
// No atomics, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "align.h"
#include "launch.h"
#include "model.h"

namespace {

// ---- cost ------------------------------------------------------------------------------------------------------------------------------
constexpr int AC_TILE = 64, AC_LD = AL_CH + 1, AC_THREADS = 256, AM_GROUPS = 4;

__global__ __launch_bounds__(AM_GROUPS* AL_CH) void align_means_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                         const int32_t* __restrict__ lens, int B, int Ts, int Tr,
                                                                         double* __restrict__ means) {
    __shared__ double part[AM_GROUPS][AL_CH];
    const int b = blockIdx.x, side = blockIdx.y, k = threadIdx.x % AL_CH, g = threadIdx.x / AL_CH;
    const int T = side ? Tr : Ts;
    const int n = min(max(lens[side * B + b], 0), T);
    const float* p = (side ? y : x) + (size_t)b * T * AL_CH + k;
    double s = 0.0;
    for (int f = g; f < n; f += AM_GROUPS) s += (double)p[(size_t)f * AL_CH];
    part[g][k] = s;
    __syncthreads();
    if (g == 0) means[((size_t)b * 2 + side) * AL_CH + k] = n > 0 ? ((part[0][k] + part[1][k]) + (part[2][k] + part[3][k])) / (double)n : 0.0;
}

__global__ __launch_bounds__(AC_THREADS) void align_cost_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const int32_t* __restrict__ lens, int B, int Ts, int Tr,
                                                                  const double* __restrict__ means, float* __restrict__ cost) {
    __shared__ float xs[AC_TILE * AC_LD], ys[AC_TILE * AC_LD];
    const int b = blockIdx.z, i0 = blockIdx.y * AC_TILE, j0 = blockIdx.x * AC_TILE;
    const int xl = min(max(lens[b], 0), Ts), yl = min(max(lens[B + b], 0), Tr);
    if (i0 >= xl || j0 >= yl) return;
    const int tid = threadIdx.x;
    const float* xb = x + (size_t)b * Ts * AL_CH;
    const float* yb = y + (size_t)b * Tr * AL_CH;
    const double* mx = means ? means + (size_t)b * 2 * AL_CH : nullptr;
    for (int e = tid; e < AC_TILE * AL_CH; e += AC_THREADS) {
        const int r = e / AL_CH, k = e - r * AL_CH;
        const int gi = i0 + r, gj = j0 + r;
        xs[r * AC_LD + k] = gi < xl ? (float)((double)xb[(size_t)gi * AL_CH + k] - (mx ? mx[k] : 0.0)) : 0.f;
        ys[r * AC_LD + k] = gj < yl ? (float)((double)yb[(size_t)gj * AL_CH + k] - (mx ? mx[AL_CH + k] : 0.0)) : 0.f;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    for (int k0 = 0; k0 < AL_CH; k0 += 8) {
        float xa[4][8], yc[4][8];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                xa[a][k] = xs[(ty + 16 * a) * AC_LD + k0 + k];
                yc[a][k] = ys[(tx + 16 * a) * AC_LD + k0 + k];
            }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float p = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float d = xa[a][k] - yc[c][k];
                    p = fmaf(d, d, p);
                }
                acc[a][c] += p;
            }
    }
    float* cb = cost + (size_t)b * Ts * Tr;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
            if (i < xl && j < yl) cb[(size_t)i * Tr + j] = acc[a][c];
        }
}

// ---- DP + walk -------------------------------------------------------------------------------------------------------------------------
constexpr int AW_T4 = 32;                                   // dwords per lane of the walk's window: 128 steps

// The cost in the DP's order: skew[strip][t][lane] = c[64 strip + lane][t - lane] (0 outside the pair).  A workgroup owns 64 steps of one strip:
// rows are read along j (one line or two per wave-instruction), turned in LDS and written along the lanes.
__global__ __launch_bounds__(256) void align_skew_kernel(const float* __restrict__ cost, const int32_t* __restrict__ lens, int B, int Ts, int Tr,
                                                         float* __restrict__ skew, int nt) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, s = blockIdx.y, tt0 = blockIdx.x * 64;
    const int xl = min(max(lens[b], 1), Ts), yl = min(max(lens[B + b], 1), Tr);
    if (s * AL_STRIP >= xl || tt0 > yl + 62) return;          // the DP looks at steps 0 .. y_len + 62 of its strips only
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const float* c = cost + (size_t)b * Ts * Tr;
    for (int r = wq; r < 64; r += 4) {
        const int i = s * AL_STRIP + r, j = tt0 + lane - r;
        tile[r][lane] = i < xl && j >= 0 && j < yl ? c[(size_t)i * Tr + j] : 0.f;
    }
    __syncthreads();
    float* out = skew + ((size_t)b * ((Ts + AL_STRIP - 1) / AL_STRIP) + s) * nt * 64;
    for (int tl = wq; tl < 64; tl += 4)
        if (tt0 + tl < nt) out[(size_t)(tt0 + tl) * 64 + lane] = tile[lane][tl];
}

// lane l takes lane l - 1's v; lane 0 takes `first`
__device__ __forceinline__ float from_lane_above(float v, float first) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

__global__ __launch_bounds__(64 * AL_MAX_WAVES) void align_dp_kernel(const float* __restrict__ cost, const int32_t* __restrict__ lens, int B, int Ts,
                                                                      int Tr, uint32_t* __restrict__ steps, const float* __restrict__ skew, int nt4,
                                                                      int32_t* __restrict__ row, float* __restrict__ total,
                                                                      int32_t* __restrict__ path_len) {
    __shared__ float ring[AL_MAX_WAVES][AL_RING];
    __shared__ float band[2][AL_MAX_SIDE];                  // after the DP: the walk's window and the runs per column
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
    const int xl = min(max(lens[b], 1), Ts), yl = min(max(lens[B + b], 1), Tr);
    const float* c = cost + (size_t)b * Ts * Tr;
    uint32_t* st = steps + (size_t)b * ((Ts + AL_STRIP - 1) / AL_STRIP) * nt4 * 64;
    const int nstr = (xl + AL_STRIP - 1) / AL_STRIP;
    const int NS = (yl + 63 + AL_SS - 1) / AL_SS;           // barrier intervals a strip takes: steps 0 .. yl + 62
    const int nbands = (nstr + W - 1) / W;
    for (int bd = 0; bd < nbands; ++bd) {
        const int wa = min(W, nstr - bd * W);               // strips of this band
        const int s = bd * W + w;
        const bool mine = w < wa;
        const int i = s * AL_STRIP + lane;
        const bool rowok = mine && i < xl;
        const float* in = w == 0 ? band[(bd & 1) ^ 1] : ring[w - 1];
        const int in_mask = w == 0 ? AL_MAX_SIDE - 1 : AL_RING - 1;
        float* out = w == wa - 1 ? band[bd & 1] : ring[w];
        const int out_mask = w == wa - 1 ? AL_MAX_SIDE - 1 : AL_RING - 1;
        const float* cs = skew + ((size_t)b * ((Ts + AL_STRIP - 1) / AL_STRIP) + (mine ? s : 0)) * nt4 * 4 * 64 + lane;      // [step][lane]
        uint32_t* dst = st + (size_t)(mine ? s : 0) * nt4 * 64 + lane;
        float Dp = 0.f, diag = 0.f;
        float cur[8], nxt[8];                                // the costs of eight steps, and of the eight after them
        const int nq = NS + AL_LAG * (wa - 1);
        for (int q = 0; q < nq; ++q) {
            const int ql = q - AL_LAG * w;
            if (mine && ql >= 0 && ql < NS) {
                const int t0 = ql * AL_SS;
                const float above = s > 0 ? in[(t0 + lane) & in_mask] : 0.f;      // D[first row - 1][t0 + lane]
                if (ql == 0) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) cur[u] = cs[(size_t)u * 64];
                }
                int last = 0;
                for (int ch = 0; ch < AL_SS / 8; ++ch) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) nxt[u] = cs[(size_t)(t0 + (ch + 1) * 8 + u) * 64];      // at the strip's end: the slack of align_nt4
                    uint32_t pk = 0;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int tt = ch * 8 + u, t = t0 + tt, j = t - lane;
                        const bool act = rowok && j >= 0 && j < yl;
                        const float first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(above), tt));
                        const float up = from_lane_above(Dp, first);
                        float best = diag;
                        uint32_t d = 0;
                        if (up < best) { best = up; d = 1; }
                        if (Dp < best) { best = Dp; d = 2; }
                        if (i == 0) { best = Dp; d = 2; }
                        if (j == 0) { best = up; d = 1; }
                        const float Dn = (i == 0 && j == 0) ? cur[u] : cur[u] + best;
                        diag = act ? up : diag;
                        Dp = act ? Dn : Dp;
                        // the strip's last row, column t - 63, collected across the lanes: lane tt of `last`
                        last = lane == tt ? __builtin_amdgcn_readlane(__float_as_int(Dp), 63) : last;
                        pk |= (act ? d : 0u) << (8 * (u & 3));
                        if ((u & 3) == 3) {
                            dst[(size_t)(t >> 2) * 64] = pk;
                            pk = 0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
                }
                const int jl = t0 + lane - 63;                // lane tt < AL_SS holds the last row's column t0 + tt - 63
                if (lane < AL_SS && jl >= 0 && jl < yl) out[jl & out_mask] = __int_as_float(last);
            }
            __syncthreads();
        }
        if (rowok && i == xl - 1) total[b] = Dp;              // the lane of the last row stopped at the last column
    }
    // ---- the walk back: wave 0, every lane the same walk (its LDS reads are broadcasts); lane 0 records
    uint32_t* win = reinterpret_cast<uint32_t*>(&band[0][0]);                     // [AW_T4][64]
    uint16_t* ihi = reinterpret_cast<uint16_t*>(win + AW_T4 * 64);                // [4096]: the largest row of the path in column j
    uint16_t* ilo = ihi + AL_MAX_SIDE;                                            // [4096]: the smallest
    int n = 1;
    if (w == 0) {
        int i = xl - 1, j = yl - 1, ws_ = -1, w4lo = 0;
        if (lane == 0) ihi[j] = (uint16_t)i;
        for (int g = xl + yl - 2; g > 0 && (i > 0 || j > 0); --g) {
            uint32_t d;
            if (i == 0) d = 2;
            else if (j == 0) d = 1;
            else {
                const int s = i >> 6, l = i & 63, t4 = (j + l) >> 2;
                if (s != ws_ || t4 < w4lo || t4 >= w4lo + AW_T4) {
                    ws_ = s;
                    w4lo = max(0, t4 - (AW_T4 - 1));
                    __builtin_amdgcn_wave_barrier();
                    const uint32_t* src = st + ((size_t)s * nt4 + w4lo) * 64 + lane;
#pragma unroll 8
                    for (int r = 0; r < AW_T4; ++r) win[r * 64 + lane] = w4lo + r < nt4 ? src[(size_t)r * 64] : 0u;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                d = ((uint32_t)__builtin_amdgcn_readfirstlane((int)win[(t4 - w4lo) * 64 + l]) >> (8 * ((j + l) & 3))) & 3u;      // one value: scalar from here on
                if (d > 2) d = 0;
            }
            if (d == 1) {
                --i;
            } else {
                if (lane == 0) ilo[j] = (uint16_t)i;
                if (d == 0) --i;
                --j;
                if (lane == 0) ihi[j] = (uint16_t)i;
            }
            ++n;
        }
        if (lane == 0) ilo[j] = (uint16_t)i;
    }
    __syncthreads();
    if (tid == 0) path_len[b] = n;
    // ---- row[j]: the smallest cost among the column's run, ties to the smallest row (walked from the largest: <= replaces)
    for (int j = tid; j < yl; j += blockDim.x) {
        const int hi = min((int)ihi[j], xl - 1), lo = min((int)ilo[j], hi);
        int r = hi;
        float best = c[(size_t)hi * Tr + j];
        for (int i = hi - 1; i >= lo; --i) {
            const float v = c[(size_t)i * Tr + j];
            if (v <= best) { best = v; r = i; }
        }
        row[(size_t)b * Tr + j] = r;
    }
}

// ---- durations -------------------------------------------------------------------------------------------------------------------------
constexpr int AD_THREADS = 256;

__device__ __forceinline__ int first_at_least(const int32_t* r, int n, int v) {      // first j with r[j] >= v (n if none); r does not decrease
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (r[m] < v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(AD_THREADS) void align_durations_kernel(const int32_t* __restrict__ row, const float* __restrict__ cost,
                                                                      const int32_t* __restrict__ d_syn, const int32_t* __restrict__ lens, int B,
                                                                      int Ts, int Tr, int L, int32_t* __restrict__ d_rec,
                                                                      float* __restrict__ phoneme_cost) {
    __shared__ int32_t rs[AL_MAX_SIDE];
    __shared__ int32_t seg[AD_THREADS + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int xl = min(max(lens[b], 1), Ts), yl = min(max(lens[B + b], 1), Tr);
    for (int j = tid; j < yl; j += AD_THREADS) rs[j] = min(max(row[(size_t)b * Tr + j], 0), xl - 1);
    // the integer scan of d_syn: a run of phonemes per thread, the runs' sums scanned by one thread
    const int per = (L + AD_THREADS - 1) / AD_THREADS;
    const int p0 = min(tid * per, L), p1 = min(p0 + per, L);
    const int32_t* d = d_syn + (size_t)b * L;
    long sum = 0;
    for (int p = p0; p < p1; ++p) sum += max(d[p], 0);
    seg[tid + 1] = (int32_t)min(sum, (long)AL_MAX_SIDE + 1);
    __syncthreads();
    if (tid == 0) {
        seg[0] = 0;
        for (int k = 1; k <= AD_THREADS; ++k) seg[k] = min(seg[k - 1] + seg[k], AL_MAX_SIDE + 1);
    }
    __syncthreads();
    const float* c = cost + (size_t)b * Ts * Tr;
    int start = seg[tid];
    for (int p = p0; p < p1; ++p) {
        const int end = min(start + max(d[p], 0), AL_MAX_SIDE + 1);
        const int lo = first_at_least(rs, yl, start), hi = first_at_least(rs, yl, end);
        float s = 0.f;
        for (int j = lo; j < hi; ++j) s += c[(size_t)rs[j] * Tr + j];
        d_rec[(size_t)b * L + p] = hi - lo;
        phoneme_cost[(size_t)b * L + p] = hi > lo ? s / (float)(hi - lo) : 0.f;
        start = end;
    }
}

}  // namespace

AlignWs align_carve(void* ws, int B, int Ts, int Tr) {
    Carver cv(ws);
    AlignWs w;
    w.lens = cv.take<int32_t>((size_t)2 * B);
    w.means = cv.take<double>((size_t)B * 2 * AL_CH);
    w.steps = cv.take<uint32_t>((size_t)B * align_strips(Ts) * align_nt4(Tr) * 64);
    w.skew = cv.take<float>((size_t)B * align_strips(Ts) * align_nt4(Tr) * 4 * 64);
    w.bytes = (cv.off + 255) & ~(size_t)255;
    return w;
}

extern "C" int cmtts_launch_align_cost(const float* x, const float* y, const int32_t* lens, int B, int Ts, int Tr, int normalise, double* means,
                                       float* cost, void* stream) {
    if (B < 1 || B > AL_MAX_B || Ts < 1 || Ts > AL_MAX_SIDE || Tr < 1 || Tr > AL_MAX_SIDE || (normalise && !means)) return -2;
    hipStream_t s = (hipStream_t)stream;
    if (normalise) hipLaunchKernelGGL(align_means_kernel, dim3(B, 2), dim3(AM_GROUPS * AL_CH), 0, s, x, y, lens, B, Ts, Tr, means);
    hipLaunchKernelGGL(align_cost_kernel, dim3((Tr + AC_TILE - 1) / AC_TILE, (Ts + AC_TILE - 1) / AC_TILE, B), dim3(AC_THREADS), 0, s, x, y, lens, B,
                       Ts, Tr, normalise ? means : (const double*)nullptr, cost);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_align_dtw(const float* cost, const int32_t* lens, int B, int Ts, int Tr, uint32_t* steps, float* skew, int32_t* row,
                                      float* total, int32_t* path_len, void* stream) {
    if (B < 1 || B > AL_MAX_B || Ts < 1 || Ts > AL_MAX_SIDE || Tr < 1 || Tr > AL_MAX_SIDE) return -2;
    const int W = std::min(AL_MAX_WAVES, align_strips(Ts));
    const int nt4 = align_nt4(Tr);
    hipLaunchKernelGGL(align_skew_kernel, dim3((nt4 * 4 + 63) / 64, align_strips(Ts), B), dim3(256), 0, (hipStream_t)stream, cost, lens, B, Ts, Tr, skew,
                       nt4 * 4);
    hipLaunchKernelGGL(align_dp_kernel, dim3(B), dim3(64 * W), 0, (hipStream_t)stream, cost, lens, B, Ts, Tr, steps, skew, nt4, row, total, path_len);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_align_durations(const int32_t* row, const float* cost, const int32_t* d_syn, const int32_t* lens, int B, int Ts, int Tr,
                                            int L, int32_t* d_rec, float* phoneme_cost, void* stream) {
    if (B < 1 || B > AL_MAX_B || Ts < 1 || Ts > AL_MAX_SIDE || Tr < 1 || Tr > AL_MAX_SIDE || L < 1 || L > AL_MAX_L) return -2;
    hipLaunchKernelGGL(align_durations_kernel, dim3(B), dim3(AD_THREADS), 0, (hipStream_t)stream, row, cost, d_syn, lens, B, Ts, Tr, L, d_rec,
                       phoneme_cost);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
namespace {

bool align_sides(int B, int Ts, int Tr) { return B >= 1 && B <= AL_MAX_B && Ts >= 1 && Ts <= AL_MAX_SIDE && Tr >= 1 && Tr <= AL_MAX_SIDE; }

// the checks the three entry points share; on success the lengths are on their way into the workspace
int align_begin(const std::string& who, int B, int Ts, int Tr, const int32_t* x_len, const int32_t* y_len, void* ws, size_t ws_bytes, hipStream_t s,
                AlignWs* out) {
    if (!x_len || !y_len) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (!align_sides(B, Ts, Tr)) return fail(CMTTS_E_INVALID, who + ": 1 <= B <= 65535 and 1 <= Ts, Tr <= 4096");
    for (int b = 0; b < B; ++b)
        if (x_len[b] < 1 || x_len[b] > Ts || y_len[b] < 1 || y_len[b] > Tr)
            return fail(CMTTS_E_INVALID, who + ": row " + std::to_string(b) + ": lengths (" + std::to_string(x_len[b]) + ", " + std::to_string(y_len[b]) +
                                             ") outside [1, " + std::to_string(Ts) + "] x [1, " + std::to_string(Tr) + "]");
    if (!ws || ws_bytes < cmtts_align_workspace_bytes(B, Ts, Tr)) return fail(CMTTS_E_WORKSPACE, who + ": workspace too small");
    *out = align_carve(ws, B, Ts, Tr);
    HIPCHK(hipMemcpyAsync(out->lens, x_len, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(out->lens + B, y_len, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return 0;
}

}  // namespace

extern "C" {

size_t cmtts_align_workspace_bytes(int B, int Ts, int Tr) {
    if (!align_sides(B, Ts, Tr)) return 0;
    return align_carve(nullptr, B, Ts, Tr).bytes;
}

int cmtts_align_cost(const float* x, const int32_t* x_len, int Ts, const float* y, const int32_t* y_len, int Tr, int B, int n_mels, int normalise,
                     float* cost, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_align_cost";
    if (!x || !y || !cost) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (n_mels != AL_CH) return fail(CMTTS_E_INVALID, who + ": n_mels must be 80");
    AlignWs w;
    CHK(align_begin(who, B, Ts, Tr, x_len, y_len, ws, ws_bytes, (hipStream_t)stream, &w));
    if (cmtts_launch_align_cost(x, y, w.lens, B, Ts, Tr, normalise != 0, w.means, cost, stream) != 0) return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

int cmtts_align_dtw(const float* cost, const int32_t* x_len, const int32_t* y_len, int B, int Ts, int Tr, int32_t* row, float* total,
                    int32_t* path_len, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "cmtts_align_dtw";
    if (!cost || !row || !total || !path_len) return fail(CMTTS_E_INVALID, who + ": null argument");
    AlignWs w;
    CHK(align_begin(who, B, Ts, Tr, x_len, y_len, ws, ws_bytes, (hipStream_t)stream, &w));
    if (cmtts_launch_align_dtw(cost, w.lens, B, Ts, Tr, w.steps, w.skew, row, total, path_len, stream) != 0) return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

int cmtts_align_durations(const int32_t* row, const float* cost, const int32_t* d_syn, const int32_t* d_syn_host, const int32_t* x_len,
                          const int32_t* y_len, int B, int Ts, int Tr, int L, int32_t* d_rec, float* phoneme_cost, void* ws, size_t ws_bytes,
                          void* stream) {
    const std::string who = "cmtts_align_durations";
    if (!row || !cost || !d_syn || !d_rec || !phoneme_cost) return fail(CMTTS_E_INVALID, who + ": null argument");
    if (L < 1 || L > AL_MAX_L) return fail(CMTTS_E_INVALID, who + ": 1 <= L <= 65536");
    if (d_syn_host && x_len && align_sides(B, Ts, Tr))
        for (int b = 0; b < B; ++b) {
            long sum = 0;
            bool neg = false;
            for (int p = 0; p < L; ++p) {
                neg = neg || d_syn_host[(size_t)b * L + p] < 0;
                sum += d_syn_host[(size_t)b * L + p];
            }
            if (neg || sum != x_len[b])
                return fail(CMTTS_E_INVALID, who + ": row " + std::to_string(b) + ": d_syn must be non-negative and sum to x_len = " +
                                                 std::to_string(x_len[b]) + ", not " + std::to_string(sum));
        }
    AlignWs w;
    CHK(align_begin(who, B, Ts, Tr, x_len, y_len, ws, ws_bytes, (hipStream_t)stream, &w));
    if (cmtts_launch_align_durations(row, cost, d_syn, w.lens, B, Ts, Tr, L, d_rec, phoneme_cost, stream) != 0)
        return fail(CMTTS_E_HIP, who + ": launch failed");
    return 0;
}

}  // extern "C"
