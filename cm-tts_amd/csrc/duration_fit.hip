// Duration targets and phoneme marks (include/cmtts_hip.h: cmtts_set_duration_targets, cmtts_phoneme_marks; the definition in executable
// form: cmtts_amd/timing.py).
#include "kernels.h"

namespace {

// ---- duration_fit_kernel: behind whichever durations kernel ran, one workgroup per utterance.  The integer durations n = max((int)d, 0)
// of each segment g with a target t = target[b][g] >= 0 and S = sum n > 0 are apportioned to t frames by largest remainder
//     q = n t,  a = q / S,  r = q % S,  R = t - sum a;   the R entries with the largest r take one more frame, ties to the lower index
// in 64-bit integer arithmetic.  Phonemes in no segment (seg = -1, l >= src_len, target -1, S = 0) keep n.  d_rounded (the integers as
// fp32, every phoneme), cum and mel_len are rewritten; unmet[b] counts the segments with S = 0 and t > 0.
//
// Method: all pairs in LDS.  A lane owns phoneme l and walks j = 0 .. L - 1 over the utterance's arrays in LDS — every lane of a wave
// reads the same word, a broadcast — once for S of its own segment, once for sum a and its rank among the segment's remainders
// (#{j : r_j > r_l, or r_j = r_l and j < l}); it takes the extra frame when rank < R.  Nothing is sorted, no per-segment storage
// exists (n_seg is unbounded), no atomic decides a value, and every sum is an integer: the result does not depend on the lane count
// or the launch shape.  O(L^2 / lanes) steps; a threshold search over r would be O(L log L) per segment and is what to write if
// L ~ 1000 with targets ever becomes a hot case (DESIGN.md §3.6d has the measured cost).
// LDS: seg | n -> result | a | r, 4 L ints (dynamic); a[0] is reused as the unmet counter once a is dead.
__global__ __launch_bounds__(1024) void duration_fit_kernel(float* d_rounded, int* cum, int64_t* mel_len, const int64_t* src_lens,
                                                            const int32_t* seg, const int32_t* target, int32_t* unmet, int L, int G) {
    extern __shared__ int fit_lds[];
    int* s_seg = fit_lds;
    int* s_n = s_seg + L;
    int* s_a = s_n + L;
    int* s_r = s_a + L;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t sl = src_lens[b];
    const int src = sl < 0 ? 0 : (sl > L ? L : (int)sl);
    const int32_t* tgt = target + (long)b * G;
    float* drow = d_rounded + (long)b * L;

    for (int l = tid; l < L; l += nt) {
        const int n = (int)drow[l];            // LengthRegulator.expand: int(expand_size), like the durations kernels
        int g = -1;
        if (l < src) {
            g = seg ? seg[(long)b * L + l] : 0;
            if (g < 0 || g >= G || tgt[g] < 0) g = -1;      // out of range = in no segment: nothing is read out of bounds
        }
        s_seg[l] = g;
        s_n[l] = n > 0 ? n : 0;
    }
    __syncthreads();
    // pass 1: S of the own segment -> a, r (r = -1: this phoneme keeps n)
    for (int l = tid; l < L; l += nt) {
        const int g = s_seg[l], n = s_n[l];
        int a = n, r = -1;
        if (g >= 0) {
            int64_t S = 0;
            for (int j = 0; j < L; ++j) S += s_seg[j] == g ? s_n[j] : 0;
            if (S > 0) {
                const int64_t q = (int64_t)n * (int64_t)tgt[g];
                a = (int)(q / S);              // n <= S, so a <= t
                r = (int)(q % S);              // < S <= the utterance's frame count, an int like cum
            }
        }
        s_a[l] = a;
        s_r[l] = r;
    }
    __syncthreads();
    // pass 2: sum a of the segment and the rank of the own remainder -> the result, in place of n (only its owner reads n[l] here)
    for (int l = tid; l < L; l += nt) {
        const int g = s_seg[l], r = s_r[l];
        if (r < 0) continue;
        int64_t sum_a = 0;
        int rank = 0;
        for (int j = 0; j < L; ++j) {
            if (s_seg[j] != g) continue;
            const int rj = s_r[j];
            sum_a += s_a[j];
            rank += (rj > r || (rj == r && j < l)) ? 1 : 0;
        }
        const int64_t R = (int64_t)tgt[g] - sum_a;
        s_n[l] = s_a[l] + (rank < R ? 1 : 0);
    }
    __syncthreads();
    // segments that cannot be met: a target > 0 over durations that are all 0 (or over no phoneme at all) stays at 0 frames
    if (tid == 0) s_a[0] = 0;
    __syncthreads();
    for (int g = tid; g < G; g += nt) {
        if (tgt[g] <= 0) continue;
        int any = 0;
        for (int j = 0; j < L; ++j) any |= (s_seg[j] == g && s_n[j] > 0) ? 1 : 0;
        if (!any) atomicAdd(&s_a[0], 1);
    }
    for (int l = tid; l < L; l += nt) drow[l] = (float)s_n[l];
    __syncthreads();
    if (tid == 0 && unmet) unmet[b] = s_a[0];
    if (tid < 64) {      // cumulative sums by the first wave, as durations_wave_kernel forms them
        int carry = 0;
        for (int l0 = 0; l0 < L; l0 += 64) {
            const int l = l0 + tid;
            int v = l < L ? s_n[l] : 0;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int n = __shfl_up(v, off);
                if (tid >= off) v += n;
            }
            v += carry;
            if (l < L) cum[(long)b * L + l] = v;
            carry = __shfl(v, 63);
        }
        if (tid == 0) mel_len[b] = carry;
    }
}

// ---- phoneme_marks_kernel: marks[b][l] = (start frame, end frame, start sample, end sample) of phoneme l, one wave per utterance.
// Frames from the cumulative sum of max((int)d, 0) over l < src_len, clipped to T when T > 0; samples = ceil(frame * hop * up / down),
// the mapping of the streamed vocoder's chunk offsets (cmtts_amd/resample.py out_len).  Rows l >= src_len repeat the utterance's end.
__global__ __launch_bounds__(64) void phoneme_marks_kernel(const float* d_rounded, const int64_t* src_lens, int4* marks, int L, int T,
                                                           int hop, int up, int down) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t sl = src_lens[b];
    const int src = sl < 0 ? 0 : (sl > L ? L : (int)sl);
    int carry = 0;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        int own = 0;
        if (l < src) {
            own = (int)d_rounded[(long)b * L + l];
            own = own > 0 ? own : 0;
        }
        int v = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int n = __shfl_up(v, off);
            if (lane >= off) v += n;
        }
        v += carry;
        if (l < L) {
            int f0 = v - own, f1 = v;
            if (T > 0) { f0 = f0 < T ? f0 : T; f1 = f1 < T ? f1 : T; }
            const int64_t s0 = ((int64_t)f0 * hop * up + down - 1) / down, s1 = ((int64_t)f1 * hop * up + down - 1) / down;
            marks[(long)b * L + l] = make_int4(f0, f1, (int)s0, (int)s1);
        }
        carry = __shfl(v, 63);
    }
}

}  // namespace

size_t k_duration_fit_lds_bytes(int L) { return (size_t)4 * L * sizeof(int); }

void k_duration_fit(float* d_rounded, int* cum, int64_t* mel_len, const int64_t* src_lens, const int32_t* seg, const int32_t* target,
                    int32_t* unmet, int B, int L, int n_seg, hipStream_t s) {
    const int nt = L >= 1024 ? 1024 : (L + 63) / 64 * 64;      // a lane per phoneme up to the largest workgroup
    hipLaunchKernelGGL(duration_fit_kernel, dim3(B), dim3(nt), k_duration_fit_lds_bytes(L), s, d_rounded, cum, mel_len, src_lens, seg,
                       target, unmet, L, n_seg);
}

void k_phoneme_marks(const float* d_rounded, const int64_t* src_lens, int32_t* marks, int B, int L, int T, int hop, int up, int down,
                     hipStream_t s) {
    hipLaunchKernelGGL(phoneme_marks_kernel, dim3(B), dim3(64), 0, s, d_rounded, src_lens, reinterpret_cast<int4*>(marks), L, T, hop, up,
                       down);
}
