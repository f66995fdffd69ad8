// C ABI of the MI355X-native CM-TTS inference hot path (include/cmtts_hip.h): the error string, what launch.h declares for every unit (the generic
// conv's argument fill and launch, the switch tables' lookup, the side streams), the model handle's life cycle, the option and controls entry points,
// the length regulator, the resampler and loudness entry points and the small utilities (weight import: import.hip; handles: model.h; the text and
// frame side: text_side.hip; the denoiser, sampler, retake and ragged shard: denoiser_side.hip; the vocoder: vocoder.hip).  No allocation and no
// host synchronisation after cmtts_finalize(); everything is enqueued on the caller's stream.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cmtts_hip.h"
#include "model.h"
#include "launch.h"
#include "internal_hooks.h"
#include "kernels.h"
#include "resblock_args.h"
#include "persist_args.h"
#include "resblock_pair.h"
#include "attention.h"
#include "resample.h"
#include "loudness.h"

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// What launch.h declares, for this unit, text_side.hip, denoiser_side.hip and vocoder.hip
ConvArgs conv_args(const PackedConv& w, const float* X, int Tin, int ldx, long x_bs, float* Y, int ldy, long y_bs, int N) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.A = w.w; a.X = X;
    a.M = w.cout; a.N = N; a.K = w.cin;
    a.taps = w.taps; a.dil = 1; a.pad = (w.taps - 1) / 2;
    a.Tin = Tin; a.a_ld = w.ld; a.a_cols = w.ld; a.a_tap_stride = w.tap_stride; a.ldx = ldx;
    a.zdiv = 1; a.x_zs0 = x_bs;
    a.pre_div = 1.f; a.pre_slope = 1.f;
    a.split = INT_MAX;
    for (int i = 0; i < 2; ++i) {
        ConvOut& o = a.out[i];
        o.Y = Y; o.y_zs0 = y_bs; o.ldy = ldy; o.Tout = N; o.ostride = 1;
        o.bias = w.bias; o.alpha = 1.f; o.act = ACT_NONE; o.div = 1.f;
    }
    return a;
}

int launch(const ConvArgs& a, int epi, int nbatch, hipStream_t s) {
    const int r = cmtts_launch_conv(&a, epi, nbatch, (void*)s);
    if (r != 0) return fail(r, "conv launch failed (unsupported shape or HIP launch error)");
    return 0;
}

int knob_set(const Knob* tab, size_t n, const char* name, int value, bool* found) {
    for (size_t i = 0; i < n; ++i)
        if (!strcmp(name, tab[i].name)) {
            *found = true;
            const int prev = *tab[i].var;
            if (value >= tab[i].lo && value <= tab[i].hi) *tab[i].var = value;
            return prev;
        }
    *found = false;
    return 0;
}

// Independent branches of the text side (duration / energy predictors, ...) are short launches that cannot fill the chip:
// a branch runs on a side stream forked from and joined back into the caller's stream with events, so the two overlap.
// One side stream per caller stream (callers that run bucket groups on several streams keep their concurrency).
static int g_branch_streams = 1;
static std::vector<SideStream> g_sides;
SideStream* side_for(hipStream_t s) {
    if (!g_branch_streams) return nullptr;
    if (g_sides.capacity() < 16) g_sides.reserve(16);      // callers keep SideStream pointers across nested side_for() calls: never reallocate (only grows while empty)
    for (auto& x : g_sides)
        if (x.user == s) return &x;
    if (g_sides.size() >= 16) return nullptr;          // more caller streams than that: branches run in line
    SideStream x{s, nullptr, nullptr, nullptr};
    // (round 4: a LOW-priority branch stream was tried — the chip-filling conditioner factor GEMM stretches the latency-bound kernels of the
    // main chain — headline 12.66 ms either way, and the ragged shard's set-aside sampler, which lives on this stream, starves: 18 -> 28 ms)
    if (hipStreamCreateWithFlags(&x.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    g_sides.push_back(x);
    return &g_sides.back();
}
// The vocoder's third stream and chain events, created on first use only: HIP maps streams onto a handful of hardware
// queues in creation order, and idle extra streams made four caller streams (bucket groups) collide (25 -> 39 ms).
bool side2_ready(SideStream* ss) {
    if (ss->side2) return true;
    if (hipStreamCreateWithFlags(&ss->side2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ss->join2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ss->done0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ss->done1, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        ss->side2 = nullptr;
        return false;
    }
    return true;
}

// ... and what the frame side (text_side.hip) needs beyond them
int branch_fork(SideStream* ss) {       // work queued on ss->side after this sees everything queued on ss->user so far
    HIPCHK(hipEventRecord(ss->fork, ss->user));
    HIPCHK(hipStreamWaitEvent(ss->side, ss->fork, 0));
    return 0;
}
int branch_join(SideStream* ss) {       // work queued on ss->user after this sees everything queued on ss->side so far
    HIPCHK(hipEventRecord(ss->join, ss->side));
    HIPCHK(hipStreamWaitEvent(ss->user, ss->join, 0));
    return 0;
}

// =============================================================================== C ABI
extern "C" {

const char* cmtts_last_error(void) { return g_err.c_str(); }
int cmtts_internal_fail(int code, const char* msg) { return fail(code, msg ? msg : "?"); }     // for the other translation units (rccl_gather.hip)
const char* cmtts_version(void) { return "cmtts_hip 0.3 (gfx950)"; }
int cmtts_abi_version(void) { return CMTTS_ABI_VERSION; }

int cmtts_create(const cmtts_config* cfg, cmtts_model** out) {
    if (!cfg || !out) return fail(CMTTS_E_INVALID, "cmtts_create: null argument");
    cmtts_model* m = new cmtts_model();
    m->cfg = *cfg;
    *out = m;
    return 0;
}

int cmtts_set_tensor(cmtts_model* m, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    if (!m || m->finalized) return fail(CMTTS_E_INVALID, "cmtts_set_tensor: model is null or already finalized");
    return set_tensor(m->host, name, host_data, shape, ndim);
}

int cmtts_finalize(cmtts_model* m) {
    if (!m || m->finalized) return fail(CMTTS_E_INVALID, "cmtts_finalize: model is null or already finalized");
    const int r = finalize_model(m);
    if (r != 0) m->al.release();
    if (r == 0) denoiser_error_word_ready();
    return r;
}

void cmtts_destroy(cmtts_model* m) {
    if (!m) return;
    for (cmtts_model::StepRow& e : m->step_rows) (void)hipEventDestroy(e.ready);
    m->al.release();
    delete m;
}

int cmtts_length_regulate(const float* x_ct, const float* durations, int B, int C, int L, int T, float* out_ct,
                          int64_t* mel2ph, int64_t* mel_len, int32_t* scratch_cum, void* stream) {
    if (!x_ct || !durations || !out_ct || !mel2ph || !mel_len || !scratch_cum || B <= 0 || L <= 0 || T <= 0)
        return fail(CMTTS_E_INVALID, "cmtts_length_regulate: bad argument");
    hipStream_t s = (hipStream_t)stream;
    k_cumsum_durations(durations, scratch_cum, mel_len, B, L, s);
    k_mel2ph(scratch_cum, mel2ph, B, L, T, s);
    k_length_regulate(x_ct, mel2ph, out_ct, B, C, L, T, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- output sample rates and encodings (resample.hip)
struct cmtts_resampler {
    int L = 0, M = 0, half = 0, R = 0;
    float* table = nullptr;                 // [L][2 R + 1]
    ResampleSegment* seg = nullptr;         // the validated table of the call in flight
    int seg_cap = 0;
};
int cmtts_resampler_create(int L, int M, const float* taps_host, int half, cmtts_resampler** out) {
    if (!taps_host || !out) return fail(CMTTS_E_INVALID, "cmtts_resampler_create: null argument");
    if (L <= 0 || M <= 0 || half < 0) return fail(CMTTS_E_INVALID, "cmtts_resampler_create: L and M must be positive, half >= 0");
    if (std::__gcd(L, M) != 1) return fail(CMTTS_E_INVALID, "cmtts_resampler_create: L and M must be coprime");
    const long R = ((long)half + L - 1) / L;
    if ((long)L * (2 * R + 1) > RS_MAX_TABLE) return fail(CMTTS_E_UNSUPPORTED, "cmtts_resampler_create: the tap table [L][2 R + 1] exceeds 65536 floats");
    if (((long)(RS_TILE - 1) * M) / L + 2 * R + 2 > RS_MAX_SPAN)
        return fail(CMTTS_E_UNSUPPORTED, "cmtts_resampler_create: a tile of 256 outputs spans more than 8192 source samples");
    const size_t nt = 2 * (size_t)half + 1;
    float *taps = nullptr, *table = nullptr;
    HIPCHK(hipMalloc(&taps, nt * sizeof(float)));
    if (hipMalloc(&table, (size_t)L * (2 * R + 1) * sizeof(float)) != hipSuccess) {
        (void)hipFree(taps);
        return fail(CMTTS_E_HIP, "cmtts_resampler_create: hipMalloc failed");
    }
    hipError_t e = hipMemcpy(taps, taps_host, nt * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && cmtts_launch_resample_table(taps, L, half, (int)R, table, nullptr) != 0) e = hipErrorLaunchFailure;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    (void)hipFree(taps);
    if (e != hipSuccess) {
        (void)hipFree(table);
        return fail(CMTTS_E_HIP, std::string("cmtts_resampler_create: ") + hipGetErrorString(e));
    }
    cmtts_resampler* r = new cmtts_resampler;
    r->L = L; r->M = M; r->half = half; r->R = (int)R; r->table = table;
    *out = r;
    return 0;
}
void cmtts_resampler_destroy(cmtts_resampler* r) {
    if (!r) return;
    if (r->table) (void)hipFree(r->table);
    if (r->seg) (void)hipFree(r->seg);
    delete r;
}
int cmtts_resampler_half_width(const cmtts_resampler* r) {
    if (!r) return fail(CMTTS_E_INVALID, "cmtts_resampler_half_width: null argument");
    return r->R;
}
static int resample_encode(const char* who, cmtts_resampler* r, const float* wav, int rows, int64_t ld, const int32_t* segments, int N,
                           int encoding, float max_wav_value, void* out, int64_t out_ld, const float* gains, void* stream) {
    if (!r || !wav || !segments || !out) return fail(CMTTS_E_INVALID, std::string(who) + ": null argument");
    if (rows <= 0 || ld <= 0 || N <= 0 || N > 65535 || out_ld <= 0)
        return fail(CMTTS_E_INVALID, std::string(who) + ": rows, ld, N and out_ld must be positive (N <= 65535)");
    if (encoding < CMTTS_ENC_F32 || encoding > CMTTS_ENC_ALAW) return fail(CMTTS_E_INVALID, std::string(who) + ": unknown encoding");
    if (!(max_wav_value > 0.f && max_wav_value <= 32768.f)) return fail(CMTTS_E_INVALID, std::string(who) + ": max_wav_value outside (0, 32768]");
    hipStream_t s = (hipStream_t)stream;
    std::vector<ResampleSegment> tab(N);
    bool on_host = false;
    CHK(fetch_table(who, segments, tab.data(), (size_t)N * sizeof(ResampleSegment), s, &on_host));
    const long L = r->L, M = r->M, half = r->half;
    auto fdiv = [](long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };          // floor(a / b), b > 0
    for (int n = 0; n < N; ++n) {
        const ResampleSegment& g = tab[n];
        const char* bad = nullptr;
        if (g.row < 0 || g.row >= rows) bad = "source row outside [0, rows)";
        else if (g.n_valid < 0) bad = "negative sample count";
        else if (g.m0 < 0 || g.m1 < g.m0) bad = "m0 < 0 or m1 < m0";
        else if ((long)g.m1 > ((long)g.n_valid * L + M - 1) / M) bad = "m1 beyond ceil(n L / M)";
        else if ((long)g.m1 - g.m0 > out_ld) bad = "more outputs than out_ld";
        else if (g.m1 > g.m0) {
            const long lo = std::max(-fdiv(-((long)g.m0 * M - half), L), 0L);                  // ceil((m0 M - half) / L)
            const long hi = std::min(fdiv(((long)g.m1 - 1) * M + half, L), (long)g.n_valid - 1);
            if (lo <= hi && (lo < g.origin || hi >= (long)g.origin + ld)) bad = "the row does not hold the source samples these outputs need";
        }
        if (bad) {
            char msg[240];
            snprintf(msg, sizeof msg, "%s: segment %d (%d, %d, %d, %d, %d): %s", who, n, g.row, g.origin, g.m0, g.m1, g.n_valid, bad);
            return fail(CMTTS_E_INVALID, msg);
        }
    }
    if (N > r->seg_cap) {       // hipFree waits for the device: no call in flight still reads the old buffer
        if (r->seg) (void)hipFree(r->seg);
        r->seg = nullptr; r->seg_cap = 0;
        const int cap = std::max(64, N);
        HIPCHK(hipMalloc(&r->seg, (size_t)cap * sizeof(ResampleSegment)));
        r->seg_cap = cap;
    }
    HIPCHK(hipMemcpyAsync(r->seg, segments, (size_t)N * sizeof(ResampleSegment), on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    const int rc = cmtts_launch_resample_encode_gain(wav, (long)ld, r->seg, N, r->table, r->L, r->M, r->R, encoding, max_wav_value, out,
                                                     (long)out_ld, gains, (void*)s);
    if (rc != 0) return fail(CMTTS_E_HIP, "resample_encode launch failed");
    return 0;
}
int cmtts_resample_encode(cmtts_resampler* r, const float* wav, int rows, int64_t ld, const int32_t* segments, int N, int encoding,
                          float max_wav_value, void* out, int64_t out_ld, void* stream) {
    return resample_encode("cmtts_resample_encode", r, wav, rows, ld, segments, N, encoding, max_wav_value, out, out_ld, nullptr, stream);
}
int cmtts_resample_encode_gain(cmtts_resampler* r, const float* wav, int rows, int64_t ld, const int32_t* segments, int N, int encoding,
                               float max_wav_value, void* out, int64_t out_ld, const float* gains, void* stream) {
    return resample_encode("cmtts_resample_encode_gain", r, wav, rows, ld, segments, N, encoding, max_wav_value, out, out_ld, gains, stream);
}

// ---- loudness measurement and output gain (loudness.hip, loudness_coef.cpp)
int cmtts_loudness_coefficients(int fs, double* out10) {
    if (!out10) return fail(CMTTS_E_INVALID, "cmtts_loudness_coefficients: null argument");
    if (loudness_coefficients(fs, out10) != 0)
        return fail(CMTTS_E_INVALID, "cmtts_loudness_coefficients: fs must be a multiple of 10 in [8000, 48000]");
    return 0;
}
static bool loudness_shape_ok(int rows, int64_t ld, int fs) {
    return rows > 0 && rows <= 65535 && ld > 0 && fs >= LD_MIN_RATE && fs <= LD_MAX_RATE && fs % 10 == 0;
}
int64_t cmtts_loudness_workspace_bytes(int rows, int64_t ld, int fs) {
    if (!loudness_shape_ok(rows, ld, fs)) return 0;
    const int64_t chunk = fs / 10, n_chunks = (ld + chunk - 1) / chunk;
    return 2 * rows * n_chunks * (int64_t)sizeof(float);          // the chunk sums and the chunk peaks, [rows][n_chunks] each
}
int cmtts_loudness_measure(const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, const float* target_lufs, float ceiling_db,
                           float* stats, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "cmtts_loudness_measure";
    if (!wav || !n_valid || !stats || !ws) return fail(CMTTS_E_INVALID, std::string(who) + ": null argument");
    if (!loudness_shape_ok(rows, ld, fs))
        return fail(CMTTS_E_INVALID, std::string(who) + ": rows in [1, 65535], ld >= 1 and fs a multiple of 10 in [8000, 48000] are required");
    if (ceiling_db != ceiling_db) return fail(CMTTS_E_INVALID, std::string(who) + ": ceiling_db is NaN");
    if ((int64_t)ws_bytes < cmtts_loudness_workspace_bytes(rows, ld, fs)) return fail(CMTTS_E_INVALID, std::string(who) + ": workspace too small");
    LoudnessPlan plan;
    if (loudness_plan(fs, &plan) != 0) return fail(CMTTS_E_INVALID, std::string(who) + ": no plan for this sample rate");
    const int64_t n_chunks = (ld + plan.chunk - 1) / plan.chunk;
    if (n_chunks > INT_MAX) return fail(CMTTS_E_INVALID, std::string(who) + ": ld too large");
    float* sums = (float*)ws;
    float* peaks = sums + (size_t)rows * n_chunks;
    int rc = cmtts_launch_loudness_chunks(wav, (long)ld, rows, n_valid, &plan, sums, peaks, (int)n_chunks, stream);
    if (rc == -2) return fail(CMTTS_E_UNSUPPORTED, std::string(who) + ": the chunk span does not fit the kernel's LDS");
    if (rc != 0) return fail(CMTTS_E_HIP, "loudness chunk launch failed");
    rc = cmtts_launch_loudness_finish(sums, peaks, (int)n_chunks, (long)ld, rows, n_valid, plan.chunk, target_lufs,
                                      (float)pow(10.0, (double)ceiling_db / 20.0), stats, stream);
    if (rc != 0) return fail(CMTTS_E_HIP, "loudness finish launch failed");
    return 0;
}
int cmtts_internal_duration_fit(float* d_rounded, int* cum, int64_t* mel_len, const int64_t* src_lens, const int32_t* seg, const int32_t* target,
                                int32_t* unmet, int B, int L, int n_seg, void* stream) {
    if (!d_rounded || !cum || !mel_len || !src_lens || !target || B <= 0 || L <= 0 || n_seg < 1 || (!seg && n_seg != 1) ||
        k_duration_fit_lds_bytes(L) > 64 * 1024)
        return fail(CMTTS_E_INVALID, "cmtts_internal_duration_fit: bad argument");
    k_duration_fit(d_rounded, cum, mel_len, src_lens, seg, target, unmet, B, L, n_seg, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- options.  Three tiers:
//   cmtts_set_option            process-wide SCHEDULING knobs of the public ABI: they never change a result bit
//   cmtts_model_set_option /    per-handle NUMERICS choices (another fp32 summation order / another operand precision):
//   cmtts_vocoder_set_option    properties of a model, not of the process
//   cmtts_internal_set          A/B switches between a fused kernel and the path it replaces (bitwise equal, used by tests/ and
//                               tools/ for cross-checks and measurements); declared in csrc/internal_hooks.h, NOT part of the ABI
int cmtts_set_option(const char* name, int value) {
    if (!name) return fail(CMTTS_E_INVALID, "cmtts_set_option: null name");
    if (!strcmp(name, "cooperative_launch")) {   // persistent denoiser through hipLaunchCooperativeKernel: 0 never, 1 always, 2 = automatic
        // (default): with a communicator / process group in the process ("process_group") the first launch of every grid shape is
        // cooperative (the runtime validates co-residency), later ones plain (a cooperative launch drains every queue: +24 % per step)
        const int prev = cmtts_persist_set_cooperative(value == 2 ? -1 : (value == 0 || value == 1) ? value : -2);
        return prev < 0 ? 2 : prev;
    }
    if (!strcmp(name, "process_group")) {        // the host tells the library that a process group exists (torch.distributed initialised)
        return cmtts_persist_note_process_group(value);
    }
    static const Knob tab[] = {
        {"branch_streams", &g_branch_streams, 0, 1},     // independent branches of a call on library-owned side streams
        {"resblock_split", &g_split_resblock, 0, 2},     // fp32 residual block as two launches over 4x the CUs: 0 never, 1 small batches, 2 always (denoiser_side.hip)
        {"step_cache", &g_step_cache, 0, 1},             // cmtts_sample: keep the timestep-only step-embedding rows on the device (denoiser_side.hip)
    };
    bool found;
    const int prev = knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, &found);
    if (found) return prev;
    return fail(CMTTS_E_INVALID, "cmtts_set_option: unknown option");
}

int cmtts_model_set_option(cmtts_model* m, const char* name, int value) {
    if (!m || !name) return fail(CMTTS_E_INVALID, "cmtts_model_set_option: null argument");
    const Knob tab[] = {
        {"ffn2_split", &m->ffn2_split, 0, 1},            // FFN linear of the FFT blocks as 8 K-segment partial GEMMs + one reduction (1) or one launch (0)
        {"text16", &m->text16, 0, 1},                    // bf16 / fp16 models: 16-bit operands in the FFT blocks' FFN contractions as well (default 0)
        {"winograd", &m->winograd, 0, 2},                // fp32 persistent denoiser stack: the gated k = 3 conv as Winograd F(4,3) (default 1), F(2,3) (2) or in the direct form (0: bitwise the per-layer kernels)
        {"batch_invariant", &m->batch_invariant, 0, 1},  // fp32, winograd = 1: the per-layer residual blocks of small batches in the stack's F(4,3) form too (default 0)
    };
    bool found;
    const int prev = knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, &found);
    if (found) return prev;
    return fail(CMTTS_E_INVALID, "cmtts_model_set_option: unknown option");
}

// csrc/internal_hooks.h — fused kernel vs the path it replaces; every pair is bitwise equal (tests/test_gpu_parity.py)
int cmtts_internal_set(const char* name, int value) {
    if (!name) return fail(CMTTS_E_INVALID, "cmtts_internal_set: null name");
    if (!strcmp(name, "attn_qb")) return cmtts_attention_set_qb(value);       // attention.hip: queries split over workgroups (round 6; same bits)
    if (!strcmp(name, "xres_nt")) return cmtts_xres_set_nt(value);            // conv_xres tile width for launches that do not choose one (measurements)      // conv_xl: m-tiles over several workgroups for launches of a few column tiles
    bool found;
    int prev = vocoder_internal_set(name, value, &found);      // vocoder.hip: voc_*, post_v4
    if (found) return prev;
    prev = text_internal_set(name, value, &found);             // text_side.hip: the FFT blocks', predictors' and frame side's switches
    if (found) return prev;
    prev = denoiser_internal_set(name, value, &found);         // denoiser_side.hip: cond_*, persist_tail, persist_wino, inproj_fused
    if (found) return prev;
    return fail(CMTTS_E_INVALID, "cmtts_internal_set: unknown switch");
}

int cmtts_set_precision(cmtts_model* m, int mode) {
    if (!m || mode < 0 || mode > 3) return fail(CMTTS_E_INVALID, "cmtts_set_precision: mode 0 (fp32), 1 (bf16), 2 (fp16) or 3 (fp16x3)");
    m->precision = mode;
    return 0;
}

int cmtts_set_variance_controls(cmtts_model* m, const cmtts_variance_controls* vc) {
    if (!m) return fail(CMTTS_E_INVALID, "cmtts_set_variance_controls: null model");
    const cmtts_variance_controls off = {1.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!vc) { m->vc = off; return 0; }
    if (!(vc->p_control > 0.f) || !(vc->e_control == vc->e_control))
        return fail(CMTTS_E_INVALID, "cmtts_set_variance_controls: p_control must be > 0 (it also scales the uv logit)");
    if (vc->cwt_spec && (!vc->f0_mean || !vc->f0_std || (m->cfg.use_uv && !vc->uv)))
        return fail(CMTTS_E_INVALID, "cmtts_set_variance_controls: a pitch target needs cwt_spec, f0_mean, f0_std (and uv)");
    m->vc = *vc;
    return 0;
}

int cmtts_set_control_tables(cmtts_model* m, const cmtts_control_tables* t) {
    if (!m) return fail(CMTTS_E_INVALID, "cmtts_set_control_tables: null model");
    const cmtts_control_tables off = {nullptr, nullptr, nullptr, 0};
    if (!t) t = &off;
    if ((t->d || t->e || t->p) && t->ld <= 0)
        return fail(CMTTS_E_INVALID, "cmtts_set_control_tables: ld (the row pitch = L of the next text-side call) must be > 0");
    m->ct = *t;
    return 0;
}

int cmtts_set_duration_targets(cmtts_model* m, const cmtts_duration_targets* t) {
    if (!m) return fail(CMTTS_E_INVALID, "cmtts_set_duration_targets: null model");
    const cmtts_duration_targets off = {nullptr, nullptr, nullptr, 0, 0};
    if (!t) { m->dt = off; return 0; }
    if (!t->target) return fail(CMTTS_E_INVALID, "cmtts_set_duration_targets: target is required (NULL struct clears)");
    if (t->ld <= 0) return fail(CMTTS_E_INVALID, "cmtts_set_duration_targets: ld (the row pitch = L of the next text-side call) must be > 0");
    if (t->n_seg < 1 || (!t->seg && t->n_seg != 1))
        return fail(CMTTS_E_INVALID, "cmtts_set_duration_targets: n_seg must be >= 1, and 1 without a segment table");
    m->dt = *t;
    return 0;
}

int cmtts_phoneme_marks(const float* d_rounded, const int64_t* src_lens, int B, int L, int T, int hop, int up, int down,
                        int32_t* marks, void* stream) {
    if (!d_rounded || !src_lens || !marks || B <= 0 || L <= 0 || T < 0 || hop <= 0 || up <= 0 || down <= 0)
        return fail(CMTTS_E_INVALID, "cmtts_phoneme_marks: bad argument");
    k_phoneme_marks(d_rounded, src_lens, marks, B, L, T, hop, up, down, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_set_debug_stamps(void* dev_buf) {
    cmtts_resblock_set_debug((long long*)dev_buf);
    cmtts_persist_set_debug((long long*)dev_buf);
    cmtts_pair_set_debug((long long*)dev_buf);
    cmtts_xres_set_debug((long long*)dev_buf);
    {   // generic conv kernel: CMTTS_CONV_DBG_MK="M,K" selects the launches to stamp (tools/conv_phases.py)
        int M = 0, K = 0;
        const char* mk = getenv("CMTTS_CONV_DBG_MK");
        if (mk && sscanf(mk, "%d,%d", &M, &K) == 2) cmtts_conv_set_debug(dev_buf ? (long long*)dev_buf : nullptr, M, K);
        else cmtts_conv_set_debug(nullptr, 0, 0);
    }
    return 0;
}

int cmtts_wav_to_int16(const float* wav, int16_t* pcm, int64_t n, float max_wav_value, void* stream) {
    if (!wav || !pcm || n < 0) return fail(CMTTS_E_INVALID, "cmtts_wav_to_int16: bad argument");
    if (n) k_wav_to_int16(wav, pcm, (long)n, max_wav_value, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_length_mask(const int64_t* lens, uint8_t* mask, int B, int W, void* stream) {
    if (!lens || !mask || B <= 0 || W < 0) return fail(CMTTS_E_INVALID, "cmtts_length_mask: bad argument");
    if (W == 0) return 0;
    k_length_mask(lens, mask, B, W, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_transpose(const float* in, float* out, int B, int R, int C, void* stream) {
    if (!in || !out || B <= 0 || R <= 0 || C <= 0) return fail(CMTTS_E_INVALID, "cmtts_transpose: bad argument");
    k_transpose(in, out, B, R, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_pack_conv_weight(const float* host_w, int Cout, int Cin, int K, float** dev_packed, int* ld) {
    if (!host_w || !dev_packed || !ld || Cout <= 0 || Cin <= 0 || K <= 0) return fail(CMTTS_E_INVALID, "cmtts_pack_conv_weight: bad argument");
    HostTensor W;
    W.shape = {Cout, Cin, K};
    W.data.assign(host_w, host_w + (size_t)Cout * Cin * K);
    Allocs al;
    PackedConv p;
    CHK(pack_conv(al, W, nullptr, nullptr, &p));
    *dev_packed = p.w;
    *ld = p.ld;
    return 0;
}
void cmtts_free_device(void* p) {
    if (p) (void)hipFree(p);
}
int cmtts_conv1d(const float* x, const float* packed_w, int ld, const float* bias, int B, int Cin, int Cout, int T, int K,
                 int dilation, int padding, int act, float* y, void* stream) {
    if (!x || !packed_w || !y) return fail(CMTTS_E_INVALID, "cmtts_conv1d: bad argument");
    PackedConv w;
    w.w = const_cast<float*>(packed_w); w.bias = const_cast<float*>(bias);
    w.cout = Cout; w.cin = Cin; w.taps = K; w.ld = ld; w.tap_stride = (long)Cin * ld;
    const int Tout = T + 2 * padding - dilation * (K - 1);
    if (Tout <= 0) return fail(CMTTS_E_INVALID, "cmtts_conv1d: empty output");
    ConvArgs a = conv_args(w, x, T, T, (long)Cin * T, y, Tout, (long)Cout * Tout, Tout);
    a.dil = dilation; a.pad = padding;
    a.out[0].act = act;
    CHK(launch(a, EPI_PLAIN, B, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
