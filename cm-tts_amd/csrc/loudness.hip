// Integrated loudness (ITU-R BS.1770) of fp32 waveform rows and the gain that brings each to a target (include/cmtts_hip.h:
// cmtts_loudness_measure; definition: cmtts_amd/loudness.py).
//
// The K-weighting is a 4th-order IIR (two biquads, poles at radius 0.989 at 22 050 Hz): a serial recurrence over the whole utterance.
// It is parallelised over time twice.
//   Across chunks: the unit is a CHUNK of 0.1 s (a 0.4 s block with its 0.1 s hop is exactly four consecutive chunks).  The workgroup of
//     chunk c restarts the filter from zero state two chunks (0.2 s) earlier — 0.989^4410 is far below fp32 resolution — or at sample 0,
//     where the zero state is exact.
//   Inside the workgroup: the span (<= 3 chunks) is staged into LDS, each lane owns a RUN of consecutive samples.  Pass 1 filters the run
//     from zero state: its end state e_k.  The state entering run k + 1 is s[k + 1] = P s[k] + e_k with the constant 4 x 4 matrix
//     P = A^run (A: one zero-input sample), so the s[k] are a scan: log-step inside a wave with the precomputed P^(2^j), the wave totals
//     carried across the workgroup's waves through LDS.  Pass 2 filters each run again from its true state and accumulates the squares.
// Every reduction runs in a fixed order; a row's result depends on that row's samples [0, n_valid) and on nothing else.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "loudness.h"

namespace {

struct State {
    float z1, z2, w1, w2;
};

// one sample through both biquads (transposed direct form II, the shelf then the high-pass); returns the K-weighted sample
__device__ __forceinline__ float kw_step(State& s, float v, const float* b, const float* c) {
    const float u = fmaf(b[0], v, s.z1);
    s.z1 = fmaf(b[1], v, fmaf(-b[3], u, s.z2));
    s.z2 = fmaf(b[2], v, -b[4] * u);
    const float o = fmaf(c[0], u, s.w1);
    s.w1 = fmaf(c[1], u, fmaf(-c[3], o, s.w2));
    s.w2 = fmaf(c[2], u, -c[4] * o);
    return o;
}

// m (row-major 4 x 4) times s, columns ascending
__device__ __forceinline__ State matvec(const float* m, const State& s) {
    State r;
    r.z1 = fmaf(m[3], s.w2, fmaf(m[2], s.w1, fmaf(m[1], s.z2, m[0] * s.z1)));
    r.z2 = fmaf(m[7], s.w2, fmaf(m[6], s.w1, fmaf(m[5], s.z2, m[4] * s.z1)));
    r.w1 = fmaf(m[11], s.w2, fmaf(m[10], s.w1, fmaf(m[9], s.z2, m[8] * s.z1)));
    r.w2 = fmaf(m[15], s.w2, fmaf(m[14], s.w1, fmaf(m[13], s.z2, m[12] * s.z1)));
    return r;
}

__device__ __forceinline__ State shfl_up_state(const State& s, int d) {
    State r;
    r.z1 = __shfl_up(s.z1, d);
    r.z2 = __shfl_up(s.z2, d);
    r.w1 = __shfl_up(s.w1, d);
    r.w2 = __shfl_up(s.w2, d);
    return r;
}

// lane 0 of the wave receives the sum (max) over its 64 lanes, combined in a fixed tree
__device__ __forceinline__ float wave_sum(float v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int d = 32; d; d >>= 1) v = fmaxf(v, __shfl_down(v, d));
    return v;
}

__device__ __forceinline__ long clamp_len(int n, long ld) { return n < 0 ? 0 : (n > ld ? ld : n); }

constexpr int LD_WAVES = LD_THREADS / 64;

__global__ __launch_bounds__(LD_THREADS) void loudness_chunk_kernel(const float* __restrict__ wav, long ld, const int32_t* __restrict__ n_valid,
                                                                    const LoudnessPlan p, float* __restrict__ sums, float* __restrict__ peaks,
                                                                    int n_chunks) {
    extern __shared__ float xs[];                      // [LD_THREADS * run]: the staged span, zeros behind it
    __shared__ State tot[LD_WAVES];                    // the waves' scan totals
    __shared__ float red[2][LD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.y, c = blockIdx.x, run = p.run;
    const long n = clamp_len(n_valid[row], ld);
    const long beg = (long)c * p.chunk;
    const long o = (long)row * n_chunks + c;
    if (beg >= n) {                                    // uniform per workgroup: nothing of this chunk is valid
        if (tid == 0) {
            sums[o] = 0.f;
            peaks[o] = 0.f;
        }
        return;
    }
    const long end = beg + p.chunk < n ? beg + p.chunk : n;
    const long s0 = beg - 2L * p.chunk > 0 ? beg - 2L * p.chunk : 0;
    const int span = (int)(end - s0);                  // <= 3 chunk <= LD_THREADS * run
    const float* x = wav + (long)row * ld + s0;
    for (int i = tid; i < LD_THREADS * run; i += LD_THREADS) xs[i] = i < span ? x[i] : 0.f;
    __syncthreads();

    // pass 1: the run from zero state
    const float* my = xs + tid * run;
    State e{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < run; ++t) (void)kw_step(e, my[t], p.b, p.c);

    // inclusive scan inside the wave: after step j lane l holds sum over i <= min(l, 2^(j + 1) - 1) of P^i e[l - i]
    State v = e;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const State up = shfl_up_state(v, 1 << j);
        const State add = matvec(p.P[j], up);
        if (lane >= (1 << j)) {
            v.z1 += add.z1;
            v.z2 += add.z2;
            v.w1 += add.w1;
            v.w2 += add.w2;
        }
    }
    if (lane == 63) tot[wave] = v;
    const State prev = shfl_up_state(v, 1);            // the wave's own runs before this lane's
    __syncthreads();
    // the state entering the wave: carry[w + 1] = P^64 carry[w] + tot[w], in wave order
    State carry{0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < wave; ++w) {
        const State t = tot[w];
        carry = matvec(p.P[6], carry);
        carry.z1 += t.z1;
        carry.z2 += t.z2;
        carry.w1 += t.w1;
        carry.w2 += t.w2;
    }
    // ... moved `lane` runs on: P^lane from the binary digits of lane (powers of one matrix commute)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const State m = matvec(p.P[j], carry);
        if (lane & (1 << j)) carry = m;
    }
    State s = carry;
    if (lane > 0) {
        s.z1 += prev.z1;
        s.z2 += prev.z2;
        s.w1 += prev.w1;
        s.w2 += prev.w2;
    }

    // pass 2: the run from its true state; only the chunk's own samples count
    const long first = s0 + (long)tid * run;
    float acc = 0.f, pk = 0.f;
    for (int t = 0; t < run; ++t) {
        const float xv = my[t];
        const float y = kw_step(s, xv, p.b, p.c);
        const long idx = first + t;
        if (idx >= beg && idx < end) {
            acc = fmaf(y, y, acc);
            pk = fmaxf(pk, fabsf(xv));
        }
    }
    acc = wave_sum(acc);
    pk = wave_max(pk);
    if (lane == 0) {
        red[0][wave] = acc;
        red[1][wave] = pk;
    }
    __syncthreads();
    if (tid == 0) {
        float a = red[0][0], m = red[1][0];
        for (int w = 1; w < LD_WAVES; ++w) {
            a += red[0][w];
            m = fmaxf(m, red[1][w]);
        }
        sums[o] = a;
        peaks[o] = m;
    }
}

// One wave per row: the block means from four chunk sums each, both gates, the integrated loudness, the row's peak and the gain.
__global__ __launch_bounds__(LD_FINISH_THREADS) void loudness_finish_kernel(const float* __restrict__ sums, const float* __restrict__ peaks,
                                                                            int n_chunks, long ld, const int32_t* __restrict__ n_valid, int chunk,
                                                                            const float* __restrict__ target, float ceiling, float abs_gate_z,
                                                                            float* __restrict__ stats) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const long n = clamp_len(n_valid[row], ld);
    const float* S = sums + (long)row * n_chunks;
    const float* K = peaks + (long)row * n_chunks;
    const long block = 4L * chunk;
    const bool single = n > 0 && n < block;            // shorter than one block: one block [0, n), the absolute gate only
    const int nb = n == 0 ? 0 : single ? 1 : (int)((n - block) / chunk + 1);

    float pk = 0.f;
    for (int c = lane; c < n_chunks; c += LD_FINISH_THREADS) pk = fmaxf(pk, K[c]);
    pk = __shfl(wave_max(pk), 0);

    auto z_of = [&](int j) {
        if (single) {
            float a = S[0];
            for (int c = 1; c < 4 && c < n_chunks; ++c) a += S[c];
            return a / (float)n;
        }
        return (((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) / (float)block;
    };
    float sum = 0.f, cnt = 0.f;
    for (int j = lane; j < nb; j += LD_FINISH_THREADS) {
        const float z = z_of(j);
        if (z > abs_gate_z) {
            sum += z;
            cnt += 1.f;
        }
    }
    sum = __shfl(wave_sum(sum), 0);
    cnt = __shfl(wave_sum(cnt), 0);
    if (!single && cnt > 0.f) {
        const float rel = 0.1f * (sum / cnt);          // l > l(mean) - 10  <=>  z > mean / 10
        sum = 0.f;
        cnt = 0.f;
        for (int j = lane; j < nb; j += LD_FINISH_THREADS) {
            const float z = z_of(j);
            if (z > abs_gate_z && z > rel) {
                sum += z;
                cnt += 1.f;
            }
        }
        sum = __shfl(wave_sum(sum), 0);
        cnt = __shfl(wave_sum(cnt), 0);
    }
    if (lane != 0) return;
    const float L = cnt > 0.f ? -0.691f + 10.f * log10f(sum / cnt) : -INFINITY;
    const float t = target ? target[row] : NAN;
    float g = 1.f;
    if (cnt > 0.f && !isnan(t) && pk > 0.f) {
        g = exp10f((t - L) / 20.f);
        if (pk * g > ceiling) g = ceiling / pk;
    }
    float* st = stats + 4L * row;
    st[0] = L;
    st[1] = pk;
    st[2] = g;
    st[3] = cnt;
}

}  // namespace

extern "C" int cmtts_launch_loudness_chunks(const float* wav, long ld, int rows, const int32_t* n_valid, const LoudnessPlan* plan, float* sums,
                                            float* peaks, int n_chunks, void* stream) {
    if (rows <= 0 || n_chunks <= 0) return 0;
    if (3L * plan->chunk > (long)LD_THREADS * plan->run || (long)n_chunks * plan->chunk < ld) return -2;
    const size_t lds = (size_t)LD_THREADS * plan->run * sizeof(float);
    if (lds > 60 * 1024 || rows > 65535) return -2;
    hipLaunchKernelGGL(loudness_chunk_kernel, dim3(n_chunks, rows), dim3(LD_THREADS), lds, (hipStream_t)stream, wav, ld, n_valid, *plan, sums,
                       peaks, n_chunks);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int cmtts_launch_loudness_finish(const float* sums, const float* peaks, int n_chunks, long ld, int rows, const int32_t* n_valid,
                                            int chunk, const float* target, float ceiling, float* stats, void* stream) {
    if (rows <= 0) return 0;
    const float abs_gate_z = (float)pow(10.0, (-70.0 + 0.691) / 10.0);          // l > -70  <=>  z > 10^((-70 + 0.691) / 10)
    hipLaunchKernelGGL(loudness_finish_kernel, dim3(rows), dim3(LD_FINISH_THREADS), 0, (hipStream_t)stream, sums, peaks, n_chunks, ld, n_valid,
                       chunk, target, ceiling, abs_gate_z, stats);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
