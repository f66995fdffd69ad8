// C ABI of the MI355X-native CM-TTS inference hot path (include/cmtts_hip.h): the entry points, workspace carving and the
// host-side launch sequences of the denoiser, sampler, retake, resampler and loudness side (weight import: import.hip; handles: model.h; the text and frame side:
// text_side.hip; the vocoder: vocoder.hip; shared helpers: launch.h).  No allocation and no
// host synchronisation after cmtts_finalize(); everything is enqueued on the caller's stream.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/cmtts_hip.h"
#include "model.h"
#include "launch.h"
#include "internal_hooks.h"
#include "kernels.h"
#include "resblock_args.h"
#include "persist_args.h"
#include "cond_gemm.h"
#include "resblock_pair.h"
#include "inproj.h"
#include "attention.h"
#include "text_state.h"
#include "stream_windows.h"
#include "resample.h"
#include "loudness.h"
#include "noise_philox.h"
#include "retake.h"

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// What launch.h declares, for this unit, text_side.hip and vocoder.hip
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

int persist_blocks() {          // workgroups that are certainly co-resident: one 1024-thread workgroup per CU
    static int n = [] { int dev = 0, v = 0; (void)hipGetDevice(&dev);
                        (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev); return v; }();
    return n;
}

// The phoneme-level factor of the conditioner projections (CondFactors below), computed by the frame side beside its predictors:
// P1 = Wc * out1 for utterances [b0, b0 + B) of a text workspace: [B][NL*C][Lp]
int cond_phoneme_factor(cmtts_model* m, const float* out1, int B, int Lp, float* p1, hipStream_t s) {
    const cmtts_config& c = m->cfg;
    if (!m->cond_p2) return fail(CMTTS_E_UNSUPPORTED, "factored conditioner projections are not available for this model");
    CondGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.X = out1; g.Wf = m->cond_all_f; g.bias = m->cond_zero_bias; g.Y = p1;
    g.B = B; g.T = Lp; g.M = c.res_layers * c.res_channels; g.K = c.hidden; g.force = 1;
    g.flat = 1;          // 64-column tiles over all utterances' phonemes: 32 x 88 columns = 44 tiles, not 32 x 2
    // workgroups = column tiles x row groups: as close to one per CU as the 512-row passes divide (a workgroup takes a pass in ~38 us)
    const long tiles = ((long)B * Lp + 63) / 64;
    const int npass = g.M / 512;
    int best = 1;
    double best_t = 1e30;
    for (int sp = 1; sp <= npass; ++sp) {
        const int ppg = (npass + sp - 1) / sp, groups = (npass + ppg - 1) / ppg;
        const long wg = tiles * groups, cap = persist_blocks();
        const double t = (double)((wg + cap - 1) / cap) * ppg;          // rounds x passes per workgroup
        if (t < best_t - 1e-9) { best_t = t; best = sp; }
    }
    g.row_split = best;
    const int r = cmtts_launch_cond_gemm(&g, (void*)s);
    return r == 0 ? 0 : fail(r == -2 ? CMTTS_E_UNSUPPORTED : CMTTS_E_HIP, "cond_gemm (phoneme factor) launch failed");
}

namespace {

// Optional HIP-event instrumentation of the dominant kernel (the gated k=3 conv of the denoiser
// residual block), recorded on the launch stream: bench.py's live roofline figure.
struct Profile {
    bool on = false;
    std::vector<hipEvent_t> ev;   // start/stop pairs
    size_t used = 0;
    int stride = 1;               // every stride-th launch is bracketed (event records cost launch-queue time)
    long seen = 0;
} g_prof;

bool g_fused_resblock = true;
int g_persist_tail = 1;      // skip head + post-scaling inside the persistent denoiser launch (false: separate launches)
int g_inproj_fused = 1;         // denoiser input: c_in scaling + transpose + input projection + halo clearing in one launch (same bits); 0 = three launches
int g_step_cache = 1;           // cmtts_sample: reuse the timestep-only part of the step embedding across calls (same bits); 0 = recompute every call
int g_persist_wino = 3;         // fp32 persistent denoiser: the k = 3 conv in a Winograd form (NOT bitwise the direct form): 3 = F(4,3), the 8-wave WINO == 2 instances
                                // of denoiser_persist.hip (default since round 5: half of the conv's MFMAs), 1 = F(2,3), the 8-wave WINO == 1 instances (2/3), 0 = direct
                                // (2 was round 5's one-wave-per-SIMD F(2,3) stack — same bits as 1, measured 4-10 % slower, out of the build since round 6: tools/attic/ — and runs as 1)
int g_split_resblock = 1;       // fp32 residual block as two launches over 4x the CUs (resblock_split.hip): 0 never, 1 small batches, 2 always
int g_cond_gemm16 = 1;          // bf16 / fp16 / fp16x3 models: conditioner GEMM with 16-bit operands (cond_gemm16.hip); 0 = fp32 operands as until round 3 (different numerics)
int g_cond_gemm = 1;            // stacked conditioner GEMM through cond_gemm.hip: 0 never (generic kernel), 1 when it pays, 2 whenever supported
int g_persist = 1;              // residual layers in one persistent launch (denoiser_persist.hip): 0 never, 1 when it pays, 2 whenever supported
unsigned* g_tmo_host = nullptr;  // pinned, device-visible: 1 = a neighbour wait of the persistent kernel expired, 2 = a denoiser evaluation wrote a
                                 // non-finite mel value (persist_tail.h, mel_post_kernel: the sampler's post-scaling sees every output element), 3 = a conv
                                 // input of the fp16 / fp16x3 residual blocks left the fp16 range (denoiser_persist_lp.hip, resblock_fused_lp.hip)
// Reads and clears the device flag word (one atomic exchange: a device store between a read and a clear cannot be lost).
// cmtts_poll_error() reports every code.  A denoiser call checks the word before it launches (before_launch): only code 1 — a neighbour
// wait that expired, i.e. a chip that did not hold the whole grid — refuses the launch; codes 2 / 3 describe the numerics of ONE earlier
// request (possibly another model's, on another stream) and stay in the word for cmtts_poll_error(): they do not fail an unrelated call
// (ADVICE r05).
int check_device_flag(bool before_launch = false) {
    if (!g_tmo_host) return 0;
    unsigned v = __atomic_load_n(g_tmo_host, __ATOMIC_RELAXED);
    if (!v) return 0;
    if (before_launch && v != 1) return 0;
    v = __atomic_exchange_n(g_tmo_host, 0u, __ATOMIC_ACQ_REL);
    if (!v) return 0;
    if (v == 1) return fail(CMTTS_E_HIP, "persistent denoiser: a neighbour wait timed out (the affected utterances' mel is NaN)");
    if (v == 3) return fail(CMTTS_E_HIP, "denoiser, fp16 / fp16x3 operands: a conv input left the fp16 range (|u| > 65504) in an earlier evaluation — the "
                                         "mel is finite but wrong; use bf16 or fp32 for this model / input scale");
    return fail(CMTTS_E_HIP, "denoiser: non-finite mel values in an earlier evaluation (fp16 / fp16x3 operands overflow at 65504: "
                             "use bf16 or fp32 for this model / input scale; fp32: non-finite weights or inputs)");
}

// Persistent launches need ALL of their workgroups resident (one per CU): two grids that together exceed the CU count
// would split the chip and wait for each other's missing neighbours.  Launches of this process on different streams
// are therefore admitted by capacity: a launch waits (stream-side, through events) for the oldest launches in flight on
// OTHER streams until the workgroups still possibly running plus its own fit the chip.  Small grids (bucket groups of a
// ragged shard on separate streams) then run side by side; full-chip launches still run one after the other.
struct PersistInFlight { hipEvent_t ev; hipStream_t stream; int blocks; };
std::vector<PersistInFlight> g_persist_inflight;    // oldest first
std::vector<hipEvent_t> g_persist_free_events;

// Round 6: as long as ONE stream has ever launched persistent grids, its launches run one after the other by themselves and need neither
// admission nor an event behind every launch (an event record is a barrier packet: ~5 us between a launch and the next evaluation's input
// projection, four times per T = 4 sample).  The first launch from a second stream drains the device once and switches the tracking on.
hipStream_t g_persist_only_stream = (hipStream_t)(intptr_t)-1;
bool g_persist_multi = false;
int persist_admit(hipStream_t s, int blocks, int capacity) {
    if (!g_persist_multi) {
        if (g_persist_only_stream == (hipStream_t)(intptr_t)-1) g_persist_only_stream = s;
        if (s == g_persist_only_stream) return 0;
        HIPCHK(hipDeviceSynchronize());          // launches so far carry no event: nothing of them may still be running when tracking starts
        g_persist_multi = true;
    }
    // drop launches that have certainly finished
    for (size_t i = 0; i < g_persist_inflight.size();) {
        if (hipEventQuery(g_persist_inflight[i].ev) == hipSuccess) {
            g_persist_free_events.push_back(g_persist_inflight[i].ev);
            g_persist_inflight.erase(g_persist_inflight.begin() + i);
        } else {
            ++i;
        }
    }
    (void)hipGetLastError();          // hipErrorNotReady from the queries is not an error
    // launches of one stream run one after the other: a stream holds at most its largest launch in flight, and it is
    // certainly idle once its NEWEST launch has finished
    struct PerStream { hipStream_t stream; int blocks; hipEvent_t newest; };
    std::vector<PerStream> per;          // in order of each stream's first launch in flight (oldest first)
    for (const auto& f : g_persist_inflight) {
        if (f.stream == s) continue;     // launches on `s` itself are ordered before this one by the stream
        size_t i = 0;
        while (i < per.size() && per[i].stream != f.stream) ++i;
        if (i == per.size()) per.push_back({f.stream, 0, f.ev});
        per[i].blocks = std::max(per[i].blocks, f.blocks);
        per[i].newest = f.ev;
    }
    int others = 0;
    for (const auto& q : per) others += q.blocks;
    for (const auto& q : per) {
        if (others + blocks <= capacity) break;
        HIPCHK(hipStreamWaitEvent(s, q.newest, 0));
        others -= q.blocks;
    }
    return 0;
}
int persist_launched(hipStream_t s, int blocks) {
    if (!g_persist_multi) return 0;
    hipEvent_t ev;
    if (!g_persist_free_events.empty()) { ev = g_persist_free_events.back(); g_persist_free_events.pop_back(); }
    else HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, s));
    g_persist_inflight.push_back({ev, s, blocks});
    return 0;
}

constexpr long SPLIT_MAX_TILES = 176;    // 32-frame tiles up to which the two-launch residual block wins (tools/split_crossover.py: 0.88 vs 1.86 ms per evaluation up to 64 tiles, 1.46 vs 2.08 at 128, 2.00 vs 2.19 at 192, 2.65 vs 2.39 at 256)

// ---------------------------------------------------------------- workspaces
struct DenWs {
    float *hin, *h, *u, *zb, *skip, *emb, *e1, *e2, *dproj, *sproj, *dp, *tbuf, *xcur, *cp;
    float* pst;                 // kernel-private state of the persistent denoiser's Winograd instances
    unsigned long long* halo;   // edge-column granules of the persistent denoiser kernel
    size_t bytes;
};
DenWs carve_den(const cmtts_config& c, int B, int T, void* base) {
    Carver cv(base);
    DenWs w;
    const int C = c.res_channels, NL = c.res_layers;
    const size_t n = (size_t)B * C * T;
    w.hin = cv.take<float>((size_t)B * c.n_mels * T);
    w.h = cv.take<float>(n);
    w.u = cv.take<float>(n);
    w.zb = cv.take<float>(n);
    w.skip = cv.take<float>(n);
    w.emb = cv.take<float>((size_t)B * C);
    w.e1 = cv.take<float>((size_t)B * 4 * C);
    w.e2 = cv.take<float>((size_t)B * C);
    w.dproj = cv.take<float>((size_t)B * NL * C);
    w.sproj = cv.take<float>((size_t)B * NL * C);
    w.dp = cv.take<float>((size_t)B * NL * C);
    w.tbuf = cv.take<float>((size_t)B);
    w.xcur = cv.take<float>((size_t)B * T * c.n_mels);
    w.cp = cv.take<float>((size_t)NL * n);       // conditioner projections of all layers [B][NL*C][T]
    w.halo = cv.take<unsigned long long>(cmtts_persist_halo_bytes(B, T) / sizeof(unsigned long long));
    w.pst = cv.take<float>(cmtts_persist_state_floats(B, T));
    w.bytes = cv.off + 256;
    return w;
}

// Denoiser.forward (model/modules.py:600-639) on x_src [B][T][80] scaled by in_scale -> F in w.hin [B][80][T]
// cp[b][l*C + m][t] = conditioner_projection_l(cond)[m][t] + bias: one stacked GEMM, reused by every step
int cond_projections(cmtts_model* m, const DenWs& w, const float* cond_ct, int B, int T, hipStream_t s) {
    const cmtts_config& c = m->cfg;
    if (g_cond_gemm16 && m->precision >= 1 && m->precision <= 3 && m->cond_all_f16[m->precision - 1]) {
        // bf16 / fp16 / fp16x3 models: the conditioner projections are residual-block contractions too — 16-bit operands (pairs), fp32 accumulate and output
        // (round 3; the oracle's operands16 modes quantise the same operands).  Shapes the kernel does not take run the fp32 kernels below.
        CondGemmArgs g;
        g.X = cond_ct; g.Wf = nullptr; g.bias = m->cond_all.bias; g.Y = w.cp;
        g.row_split = 0;
        g.B = B; g.T = T; g.M = c.res_layers * c.res_channels; g.K = c.hidden; g.force = 1;      // every shape: the numerics of a 16-bit model do not depend on the batch
        const int r = cmtts_launch_cond_gemm16(&g, m->cond_all_f16[m->precision - 1], m->precision, (void*)s);
        if (r == 0) return 0;
        if (r != -2) return fail(CMTTS_E_HIP, "cond_gemm16 launch failed");
    }
    if (m->cond_all_f) {   // X tile resident in LDS, one walk over all 20 x 256 rows (bitwise equal to the generic kernel)
        CondGemmArgs g;
        g.X = cond_ct; g.Wf = m->cond_all_f; g.bias = m->cond_all.bias; g.Y = w.cp;
        g.row_split = 0;
        g.B = B; g.T = T; g.M = c.res_layers * c.res_channels; g.K = c.hidden; g.force = g_cond_gemm == 2;
        const int r = g_cond_gemm ? cmtts_launch_cond_gemm(&g, (void*)s) : -2;
        if (r == 0) return 0;
        if (r != -2) return fail(CMTTS_E_HIP, "cond_gemm launch failed");
    }
    ConvArgs a = conv_args(m->cond_all, cond_ct, T, T, (long)c.hidden * T, w.cp, T, (long)c.res_layers * c.res_channels * T, T);
    return launch(a, EPI_PLAIN, B, s);
}

// The conditioner projections from their FACTORS (round 4).  The conditioning the path itself produces is
//   cond[:, t] = out1[:, mel2ph[t] - 1] (length regulator, 0 for padding) + pitch_embed[p_idx[t]]      (model/modules.py:373-395),
// so  Wc * cond[:, t] + b = (Wc * out1)[:, mel2ph[t] - 1] + (Wc * pitch_embed^T + b)[:, p_idx[t]]:  the stacked GEMM runs over the
// PHONEMES (L = T / 6 columns at the bench shape: 7 instead of 43 GFLOP) — cmtts_frame_forward_sub does it beside the frame-level
// predictors — the pitch-table factor is a constant of the model (cmtts_finalize), and the sampler only expands the two into
// cp[b][l*C + m][t] (cond_expand_kernel: one HBM-bound write of the tensor the dense GEMM wrote anyway).  Not bitwise the dense
// GEMM: W (a + b) and W a + W b round differently (relative 1e-7 on cp; tests/test_gpu_parity.py::test_cond_factored).  A caller that
// brings its own conditioning (CMDenoiserTTS.forward, tts_net.py:29-37) has no factors and takes the dense GEMM.
struct CondFactors {
    const float* p1 = nullptr;       // [B][NL*C][ldp]: Wc * out1, no bias
    const float* p1t = nullptr;      // [B][NL][ldp][C]: the same with the channels contiguous (sample_core / sample_ragged transpose it into the unused cp buffer)
    int ldp = 0, L = 0;
    const int64_t* mel2ph = nullptr; // [B][T]
    const int64_t* p_idx = nullptr;  // [B][T]
    bool usable(const cmtts_model* m) const;
};
int g_cond_factored = 1;        // internal switch "cond_factored": 0 = always the dense GEMM
int g_cond_inkernel = 1;        // internal switch "cond_inkernel": the fp32 persistent kernel gathers the factors itself (FACT instances: no cp tensor, the
                                // same bits as cond_expand_kernel + the plain instance); 0 = expand into cp first
inline bool C_IS_256(const cmtts_config& c) { return c.res_channels == 256; }
bool CondFactors::usable(const cmtts_model* m) const {
    return g_cond_factored && p1 && mel2ph && p_idx && m->precision == 0 && m->cond_p2 && g_fused_resblock;
}
int cond_factored(cmtts_model* m, const DenWs& w, const CondFactors& f, int B, int T, hipStream_t s) {
    const cmtts_config& c = m->cfg;
    const int r = cmtts_launch_cond_expand(f.p1, f.ldp, f.L, m->cond_p2, c.pitch_bins, f.mel2ph, f.p_idx, w.cp, B, c.res_layers * c.res_channels, T, (void*)s);
    return r == 0 ? 0 : fail(CMTTS_E_HIP, "cond_expand launch failed");
}
// DiffusionEmbedding -> mlp (Linear, Mish, Linear) -> the 20 stacked diffusion (+ speaker) projections
// (model/blocks.py:633-640,669-674; model/modules.py:579-583,626-627).  Depends only on the timesteps and
// the speaker vector, so the sampler re-uses it across evaluations at the same sigma (T = 2, 4: always 80).
// t_host: the (rescaled) timestep every row of `timesteps` holds, when the caller knows it (cmtts_sample); NaN otherwise
int step_embedding(cmtts_model* m, const DenWs& w, const float* timesteps, const float* spk, int B, hipStream_t s,
                   float t_host = NAN) {
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers;
    if (c.multi_speaker && !spk) return fail(CMTTS_E_INVALID, "speaker_emb is required for a multi-speaker model");
    const bool cacheable = g_step_cache && t_host == t_host;
    if (cacheable) {
        for (const cmtts_model::StepRow& e : m->step_rows)
            if (e.t == t_host && hipEventQuery(e.ready) == hipSuccess) {
                // the same bits as the computation below: every row of dproj is that computation on the same timestep
                k_broadcast_row(e.row, w.dproj, B, NL * C, s);
                if (c.multi_speaker) {   // dp = dproj + speaker projection (dense_small's "sum, then + add")
                    k_dense_small(spk, c.hidden, 1, m->sproj_wt, nullptr, nullptr, w.sproj, B, c.hidden, NL * C, DENSE_NONE, s);
                    k_add_rows(w.dproj, w.sproj, w.dp, (long)B * NL * C, s);
                }
                return 0;
            }
    }
    k_diff_embed(timesteps, m->omega_res, w.emb, B, C, s);
    k_dense_small(w.emb, C, 1, m->mlp0_wt, nullptr, nullptr, w.e1, B, C, 4 * C, DENSE_MISH, s);
    k_dense_small(w.e1, 4 * C, 1, m->mlp2_wt, nullptr, nullptr, w.e2, B, 4 * C, C, DENSE_NONE, s);
    k_dense_small(w.e2, C, 1, m->dproj_wt, nullptr, nullptr, w.dproj, B, C, NL * C, DENSE_NONE, s);
    if (c.multi_speaker) {
        k_dense_small(spk, c.hidden, 1, m->sproj_wt, nullptr, nullptr, w.sproj, B, c.hidden, NL * C, DENSE_NONE, s);
        k_dense_small(w.e2, C, 1, m->dproj_wt, nullptr, w.sproj, w.dp, B, C, NL * C, DENSE_NONE, s);
    }
    if (cacheable && m->step_rows.size() < 16) {
        bool known = false;
        for (const cmtts_model::StepRow& e : m->step_rows) known = known || e.t == t_host;
        if (!known) {
            cmtts_model::StepRow e{t_host, nullptr, nullptr};
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)NL * C * sizeof(float)) == hipSuccess && hipEventCreateWithFlags(&e.ready, hipEventDisableTiming) == hipSuccess) {
                e.row = (float*)p;
                m->al.ptrs.push_back(p);
                HIPCHK(hipMemcpyAsync(e.row, w.dproj, (size_t)NL * C * sizeof(float), hipMemcpyDeviceToDevice, s));
                HIPCHK(hipEventRecord(e.ready, s));
                m->step_rows.push_back(e);
            } else if (p) {
                (void)hipFree(p);
            }
        }
    }
    return 0;
}

// The sampler's post-scaling of the denoiser output (karras_diffusion.py:406,852): out = c_out*F + c_skip*xold (+ noise*nstd*0.85)
struct MelPost {
    const float* xold;
    const float* noise;
    float c_out, c_skip, nstd;
    float* out;
    // cmtts_sample_mixed: the three scalars, the re-noise switch and the destination per utterance (persist_args.h: PostRow); null = the scalars
    const PostRow* rows = nullptr;
    float* out_final = nullptr;
};

// The part of an evaluation in front of the residual layers: c_in scaling + transpose + input projection (+ clearing of the persistent
// kernel's halo granules) and the step embedding.  *halo_zeroed: the granules of this (B, T) batch have been cleared on `s`.
int denoiser_prologue(cmtts_model* m, const DenWs& w, const float* x_src, float in_scale, const float* timesteps, const float* spk, int B,
                      int T, hipStream_t s, bool embed, float t_host, bool* halo_zeroed, const float* in_scale_b = nullptr) {
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    const long cs = (long)C * T;
    *halo_zeroed = false;
    int rin = -2;
    if (g_inproj_fused && m->in_proj_f) {   // c_in scaling + transpose + input projection (+ halo clearing) in one launch: same bits
        InProjArgs ia;
        memset(&ia, 0, sizeof(ia));
        ia.x = x_src; ia.scale = in_scale; ia.scale_b = in_scale_b; ia.wf = m->in_proj_f; ia.bias = m->in_proj.bias; ia.h = w.h;
        ia.B = B; ia.T = T; ia.M = M; ia.C = C;
        const bool persist_path = g_fused_resblock && g_persist && NL <= PERSIST_MAX_LAYERS;
        if (persist_path) { ia.zero = w.halo; ia.zero_f4 = (long)(cmtts_persist_halo_bytes(B, T) / 16); }
        rin = cmtts_launch_inproj(&ia, (void*)s);
        if (rin == -3) return fail(CMTTS_E_HIP, "inproj launch failed");
        *halo_zeroed = rin == 0 && persist_path && cmtts_persist_halo_bytes(B, T) % 16 == 0;
    }
    if (rin != 0) {
        k_mel_prep(x_src, in_scale_b, in_scale, w.hin, B, T, M, s);
        ConvArgs a = conv_args(m->in_proj, w.hin, T, T, (long)M * T, w.h, T, cs, T);
        a.out[0].act = ACT_RELU;   // relu(relu(.)) == relu(.), model/modules.py:575-577,624
        CHK(launch(a, EPI_PLAIN, B, s));
    }
    if (embed) CHK(step_embedding(m, w, timesteps, spk, B, s, t_host));
    return 0;
}

// Model option "batch_invariant" (fp32 models): 1 = the per-layer residual blocks take the persistent stack's F(4,3) form
// (resblock_split_w43.hip), so that an utterance's bits do not depend on whether its batch took that stack; 0 = off or nothing to do (the
// stack runs the direct form, or a 16-bit model: one form at every shape); -1 = the stack would run F(2,3), which has no per-layer
// counterpart: every denoiser call refuses before it launches anything.
int batch_invariant_form(const cmtts_model* m) {
    if (!m->batch_invariant || m->precision != 0 || !m->winograd || !g_persist_wino || !m->res[0].w3w) return 0;
    return m->winograd == 1 && g_persist_wino == 3 && m->res[0].w3w43 ? 1 : -1;
}
int check_batch_invariant(const cmtts_model* m) {
    if (batch_invariant_form(m) >= 0) return 0;
    return fail(CMTTS_E_UNSUPPORTED, "batch_invariant: the persistent denoiser stack runs the F(2,3) form (model option \"winograd\" = 2), "
                                     "which has no per-layer counterpart; set \"winograd\" to 1 or 0");
}

int denoiser_core(cmtts_model* m, const DenWs& w, const float* x_src, float in_scale, const float* timesteps,
                  const float* cond_ct, const float* spk, int B, int T, const MelPost& post, hipStream_t s, bool embed = true,
                  SideStream* pending = nullptr, float t_host = NAN,    // pending: a side branch (the conditioner GEMM) to join before the layers
                  const CondFactors* cfk = nullptr, bool* cp_ready = nullptr,     // cfk: w.cp was NOT filled — the persistent kernel gathers the factors (FACT)
                  const float* in_scale_b = nullptr) {                            // device [B]: c_in per utterance in place of in_scale (cmtts_sample_mixed)
    CHK(check_device_flag(true));
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    const long cs = (long)C * T;
    bool halo_zeroed = false;
    CHK(denoiser_prologue(m, w, x_src, in_scale, timesteps, spk, B, T, s, embed, t_host, &halo_zeroed, in_scale_b));
    if (pending) CHK(branch_join(pending));
    const float* dp = m->cfg.multi_speaker ? w.dp : w.dproj;
    const bool unfused = !g_fused_resblock;   // three-launch form of the residual block (A/B and bitwise tests)
    float* hcur = w.h;
    float* halt = w.u;
    bool layers_done = false;
    if (!unfused && g_persist && NL <= PERSIST_MAX_LAYERS) {
        // Denoiser.forward's layer loop (model/modules.py:626-633) as ONE persistent launch per utterance chunk
        PersistArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.x0 = w.h; pa.cp = w.cp; pa.cp_bstride = (long)NL * C * T;
        pa.dp = dp; pa.d = w.dproj; pa.vec_stride = (long)NL * C;
        pa.skip = w.skip; pa.halo = w.halo; pa.tmo = g_tmo_host;
        pa.B = B; pa.T = T; pa.NL = NL;
        pa.halo_zeroed = halo_zeroed;
        const int prec = m->precision;
        if (cfk && !(cp_ready && *cp_ready)) {
            pa.fact = 1; pa.p1 = cfk->p1; pa.p2 = m->cond_p2; pa.mel2ph = (const long long*)cfk->mel2ph; pa.pidx = (const long long*)cfk->p_idx;
            pa.ldp = cfk->ldp; pa.Lph = cfk->L; pa.ld2 = c.pitch_bins;
            pa.p1t = cfk->p1t; pa.p2t = m->cond_p2t;
        }
        if (g_persist_tail && m->skip_f && m->outp_f) {   // skip head + post-scaling inside the launch
            pa.tail = 1;
            pa.Wsf = m->skip_f; pa.bs = m->skip_proj.bias; pa.Wpf = m->outp_f; pa.bp = m->out_proj.bias;
            pa.skip_div = (float)sqrt((double)NL); pa.n_mels = M;
            pa.xold = post.xold; pa.noise = post.noise; pa.c_out = post.c_out; pa.c_skip = post.c_skip; pa.nstd = post.nstd;
            pa.out = post.out;
            pa.post_rows = post.rows; pa.out_final = post.out_final;
        }
        pa.wino = g_persist_wino && m->winograd && !prec && m->res[0].w3w && w.pst;
        if (pa.wino && g_persist_wino == 3 && m->winograd == 1 && m->res[0].w3w43) pa.wino = 3;     // F(4,3) (model option "winograd" = 2 keeps F(2,3))
        pa.xst = w.pst;
        for (int l = 0; l < NL; ++l) {
            pa.W3f[l] = prec ? (const float*)m->res[l].w3f16[prec - 1] : (pa.wino == 3 ? m->res[l].w3w43 : pa.wino ? m->res[l].w3w : m->res[l].w3f);
            pa.Wof[l] = prec ? (const float*)m->res[l].wof16[prec - 1] : m->res[l].wof;
            pa.b3[l] = m->res[l].b3f; pa.bo[l] = m->res[l].outp.bias;
        }
        const bool prof = g_prof.on && g_prof.used + 2 <= g_prof.ev.size();
        // fp16x3 exists as the persistent stack only: shapes that do not take it run the exact fp32 kernels
        const int need = cmtts_persist_plan(B, T, NL, persist_blocks(), g_persist == 2);
        if (need) CHK(persist_admit(s, need, persist_blocks()));
        if (prof) (void)hipEventRecord(g_prof.ev[g_prof.used], s);
        const int rc = prec ? cmtts_launch_denoiser_persist_lp(&pa, prec, persist_blocks(), g_persist == 2, (void*)s)
                            : cmtts_launch_denoiser_persist(&pa, persist_blocks(), g_persist == 2, (void*)s);
        if (rc == -3) return fail(CMTTS_E_HIP, "persistent denoiser launch failed");
        if (rc == 0) {
            CHK(persist_launched(s, need));
            if (prof) { (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s); g_prof.used += 2; }
            layers_done = true;
            if (pa.tail) return 0;
        }
    }
    if (!layers_done && cfk && !(cp_ready && *cp_ready)) {
        // the persistent launch was expected to gather the factors and did not take this shape after all: expand them now
        CHK(cond_factored(m, w, *cfk, B, T, s));
        if (cp_ready) *cp_ready = true;
    }
    // "batch_invariant": every layer below takes the persistent stack's F(4,3) form (the fused, split and three-launch routes alike)
    const bool w43 = batch_invariant_form(m) > 0;
    for (int l = 0; l < NL && !layers_done; ++l) {
        const ResLayer& R = m->res[l];
        const bool prof = g_prof.on && g_prof.used + 2 <= g_prof.ev.size() && (g_prof.seen++ % g_prof.stride) == 0;
        if (!unfused) {   // ResidualBlock.forward (model/blocks.py:667-686) as one kernel, x ping-pongs
            ResArgs ra;
            memset(&ra, 0, sizeof(ra));
            ra.x_in = hcur; ra.cp = w.cp + (long)l * C * T; ra.cp_bstride = (long)NL * C * T;
            ra.dp = dp + (long)l * C; ra.d = w.dproj + (long)l * C;
            ra.x_out = halt; ra.skip = w.skip;
            ra.W3f = R.w3f; ra.b3 = R.b3f; ra.Wof = R.wof; ra.bo = R.outp.bias;
            ra.vec_stride = (long)NL * C; ra.B = B; ra.T = T; ra.accum_skip = l > 0; ra.flag = g_tmo_host;
            if (prof) (void)hipEventRecord(g_prof.ev[g_prof.used], s);
            int lrc;
            if (m->precision == 0 || m->precision == 3) {
                // few 32-frame tiles: one workgroup per tile leaves most of the chip idle for 83 us per layer; four
                // workgroups per tile in two launches finish sooner (measured crossover, tools/latency_bench.py)
                const long tiles32 = (long)((T + 31) / 32) * B;
                ra.z = w.zb;
                if (w43) {
                    ra.W3f = R.w3w43;
                    lrc = cmtts_launch_resblock_w43(&ra, (void*)s);
                } else if (g_split_resblock == 2 || (g_split_resblock == 1 && tiles32 <= SPLIT_MAX_TILES)) lrc = cmtts_launch_resblock_split(&ra, (void*)s);
                else lrc = cmtts_launch_resblock(&ra, (void*)s);
            } else {
                ra.W3f = (const float*)R.w3f16[m->precision - 1];
                ra.Wof = (const float*)R.wof16[m->precision - 1];
                lrc = cmtts_launch_resblock_lp(&ra, m->precision, (void*)s);
            }
            if (lrc != 0) return fail(CMTTS_E_HIP, "fused residual block launch failed");
            if (prof) { (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s); g_prof.used += 2; }
            float* t = hcur; hcur = halt; halt = t;
            continue;
        }
        {   // u = (x + d [+ p]) + conditioner_projection(cond)      (model/blocks.py:669-677)
            ConvArgs a = conv_args(R.cond, cond_ct, T, T, (long)c.hidden * T, halt, T, cs, T);
            a.out[0].bvec = dp + (long)l * C; a.out[0].bvec_zs = (long)NL * C;
            a.out[0].res = hcur; a.out[0].r_zs0 = cs; a.out[0].ldr = T;
            CHK(launch(a, EPI_PLAIN, B, s));
        }
        if (w43) {   // "batch_invariant": the F(4,3) conv on that u, then the split projection kernel; x ping-pongs (u is consumed first)
            ResArgs ra;
            memset(&ra, 0, sizeof(ra));
            ra.u = halt; ra.x_in = hcur; ra.x_out = halt; ra.skip = w.skip; ra.z = w.zb;
            ra.d = w.dproj + (long)l * C; ra.dp = dp + (long)l * C; ra.cp = w.cp;
            ra.W3f = R.w3w43; ra.b3 = R.b3f; ra.Wof = R.wof; ra.bo = R.outp.bias;
            ra.vec_stride = (long)NL * C; ra.B = B; ra.T = T; ra.accum_skip = l > 0;
            if (cmtts_launch_resblock_w43(&ra, (void*)s) != 0) return fail(CMTTS_E_HIP, "F(4,3) residual block launch failed");
            float* t = hcur; hcur = halt; halt = t;
            continue;
        }
        {   // z = sigmoid(gate) * tanh(filter) of the k=3 conv        (:675-679)
            ConvArgs a = conv_args(R.conv3, halt, T, T, cs, w.zb, T, cs, T);
            if (prof) (void)hipEventRecord(g_prof.ev[g_prof.used], s);
            CHK(launch(a, EPI_GATED, B, s));
            if (prof) { (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s); g_prof.used += 2; }
        }
        {   // o = output_projection(z); x' = (o[:C] + (x + d)) / sqrt(2); skip += o[C:]   (:681-686)
            ConvArgs a = conv_args(R.outp, w.zb, T, T, cs, hcur, T, cs, T);
            a.split = C;
            a.out[0].res = hcur; a.out[0].r_zs0 = cs; a.out[0].ldr = T;
            a.out[0].bvec = w.dproj + (long)l * C; a.out[0].bvec_zs = (long)NL * C;
            a.out[0].rmul = 0.70710678118654752440f;      // every form of the block scales by the fp32 reciprocal of sqrt(2) (gate.h: CMTTS_RSQRT2)
            a.out[1].Y = w.skip; a.out[1].row_off = C; a.out[1].accum = l > 0;
            CHK(launch(a, EPI_PLAIN, B, s));
        }
    }
    {   // sum(skips)/sqrt(NL) -> skip_projection -> relu -> output_projection   (model/modules.py:634-637)
        ConvArgs a = conv_args(m->skip_proj, w.skip, T, T, cs, halt, T, cs, T);
        a.pre_div = (float)sqrt((double)NL);
        a.out[0].act = ACT_RELU;
        CHK(launch(a, EPI_PLAIN, B, s));
        ConvArgs b = conv_args(m->out_proj, halt, T, T, cs, w.hin, T, (long)M * T, T);
        CHK(launch(b, EPI_PLAIN, B, s));
    }
    if (post.rows) k_mel_post_rows(w.hin, post.xold, post.noise, post.rows, post.out, post.out_final, B, T, M, g_tmo_host, s);
    else k_mel_post(w.hin, post.xold, post.noise, post.c_out, post.c_skip, post.nstd, post.out, B, T, M, g_tmo_host, s);
    return 0;
}

}  // namespace

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
    if (r == 0 && !g_tmo_host) {   // one pinned word for the whole process
        if (hipHostMalloc((void**)&g_tmo_host, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) g_tmo_host = nullptr;
        else *g_tmo_host = 0;
    }
    return r;
}

void cmtts_destroy(cmtts_model* m) {
    if (!m) return;
    for (cmtts_model::StepRow& e : m->step_rows) (void)hipEventDestroy(e.ready);
    m->al.release();
    delete m;
}

size_t cmtts_denoiser_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_den(m->cfg, B, T, nullptr).bytes; }

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

int cmtts_denoiser_forward(cmtts_model* m, const float* x, const float* timesteps, const float* cond_ct,
                           const float* speaker_emb, int B, int T, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!x || !timesteps || !cond_ct || !out || !ws || B <= 0 || T <= 0)
        return fail(CMTTS_E_INVALID, "cmtts_denoiser_forward: bad argument");
    CHK(check_batch_invariant(m));
    DenWs w = carve_den(m->cfg, B, T, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "denoiser workspace too small");
    hipStream_t s = (hipStream_t)stream;
    // the conditioner GEMM (all layers' projections of cond) and the input projection + step-embedding MLP are
    // independent: the GEMM runs on the side stream and is joined before the first residual layer
    SideStream* ss = g_fused_resblock ? side_for(s) : nullptr;
    if (ss) CHK(branch_fork(ss));
    if (g_fused_resblock) CHK(cond_projections(m, w, cond_ct, B, T, ss ? ss->side : s));
    const MelPost post = {nullptr, nullptr, 1.0f, 0.0f, 0.0f, out};
    CHK(denoiser_core(m, w, x, 1.0f, timesteps, cond_ct, speaker_emb, B, T, post, s, true, ss));
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_schedule(const cmtts_model* m, int n_steps, float* sigmas, float* renoise_std) {
    if (!m || !sigmas || !renoise_std || n_steps < 1) return fail(CMTTS_E_INVALID, "cmtts_schedule: bad argument");
    const cmtts_config& c = m->cfg;
    if (n_steps == 1) {   // sample_onestep: sigmas[0] = sigma_max (get_sigmas_karras, karras_diffusion.py:580-586)
        sigmas[0] = c.sigma_max;
        renoise_std[0] = -1.0f;   // no re-noising
        return 0;
    }
    // synthesize.py:122-147: sampler="multistep", steps=2, ts=(0,)*T+(1,)
    const double rho = c.rho, tmax = pow((double)c.sigma_max, 1.0 / rho), tmin = pow((double)c.sigma_min, 1.0 / rho);
    for (int i = 0; i < n_steps; ++i) {
        const double tsi = 0.0, tsn = (i + 1 == n_steps) ? 1.0 : 0.0;
        const double t = pow(tmax + tsi / 1.0 * (tmin - tmax), rho);
        double nt = pow(tmax + tsn / 1.0 * (tmin - tmax), rho);
        nt = nt < c.sigma_min ? (double)c.sigma_min : (nt > c.sigma_max ? (double)c.sigma_max : nt);
        sigmas[i] = (float)t;
        renoise_std[i] = (float)sqrt(nt * nt - (double)c.sigma_min * (double)c.sigma_min);   // x0.85 is applied in-kernel
    }
    return 0;
}

}  // extern "C" (reopened below)
namespace {
// cmtts_sample_mixed (per-utterance schedules on a batch sorted by non-increasing step count): evaluation i runs on the prefix [0, Bi) with
// the scalings of its rows in the device table (c_in [B], t [B], PostRow [B] per evaluation, uploaded once before the first launch).
struct MixedEval {
    int Bi;                   // utterances still evaluated: #{b : n_b > i}
    const float* c_in;        // device [B]
    const float* t;           // device [B]: the rescaled timestep of every row (rows that have left keep their last one)
    const PostRow* rows;      // device [B]
    bool embed;               // some active row's timestep differs from the one its step embedding holds
    bool t_uniform;           // all active rows share t_host: cmtts_sample's step-embedding path, cached row included
    float t_host;
    bool renoise;             // some active row is re-noised after this evaluation
};
struct MixedPlan {
    std::vector<MixedEval> ev;
    int n_re = 0;             // re-noise draws 1 .. n_re are read
};
long g_sample_rows = 0;       // utterance-evaluations launched by the last sampler call (cmtts_internal_sample_rows)

// The sampler on one padded (B, T) batch whose workspace is already carved.  noise_stride = elements between consecutive noise tensors
// (B * T * n_mels for a whole batch; a sub-batch [b0, b0 + B) of a larger batch keeps the larger batch's stride).
// seeds (cmtts_sample_seeded): device int64 [B] — x_T is generated straight into w.xcur (noise_philox.hip, draw 0 scaled by sigma_max:
// the bits of a draw-0 tensor through k_scale) and `noise` is a buffer of n_steps tensors that takes the re-noise draws 1.. in one
// launch on the side stream, beside the conditioner branch.
int sample_core(cmtts_model* m, const DenWs& w, const float* noise, long noise_stride, const float* cond_ct, const float* speaker_emb, int B,
                int T, int n_steps, const float* sigmas, const float* renoise_std, float* mel, hipStream_t s, const CondFactors* cf = nullptr,
                const int64_t* seeds = nullptr, const MixedPlan* mx = nullptr) {      // mx: n_steps = its evaluations, sigmas / renoise_std unused
    const cmtts_config& c = m->cfg;
    const long nel = (long)B * T * c.n_mels;
    g_sample_rows = 0;
    // once for all n_steps evaluations, on the side stream: joined before the first residual layer of the first evaluation
    SideStream* ss = g_fused_resblock ? side_for(s) : nullptr;
    if (ss) CHK(branch_fork(ss));
    const CondFactors* cfk = nullptr;       // non-null: no cp tensor at all, the persistent launches gather the factors (denoiser_core)
    CondFactors cf_local;
    bool cp_ready = false;
    if (g_fused_resblock) {
        if (cf && cf->usable(m)) {
            const bool inkernel = g_cond_inkernel && g_persist && g_persist_tail && m->skip_f && m->outp_f && c.res_layers <= PERSIST_MAX_LAYERS &&
                                  cmtts_persist_plan(B, T, c.res_layers, persist_blocks(), g_persist == 2) > 0;
            if (inkernel && cf->ldp <= T && m->cond_p2t && C_IS_256(c)) {
                // the persistent launches gather the factors: w.cp (NL * C * T floats per utterance) is free and takes p1 with the channels
                // contiguous, [B][NL][ldp][C] — one 57-MB transpose per sample call (bench shape, ~25 us) buys 16-byte gathers in every layer of
                // every evaluation
                // (round 6: on the side stream — nothing before the first persistent launch reads it; it ran in front of the input projection)
                cf_local = *cf;
                if (!cf_local.p1t) {
                    k_transpose(cf->p1, w.cp, B * c.res_layers, c.res_channels, cf->ldp, ss ? ss->side : s);
                    cf_local.p1t = w.cp;
                }
                cfk = &cf_local;
            } else CHK(cond_factored(m, w, *cf, B, T, ss ? ss->side : s));
        } else CHK(cond_projections(m, w, cond_ct, B, T, ss ? ss->side : s));
    }
    const float* renoise0 = noise + noise_stride;       // draw 1 + i at renoise0 + i * noise_stride
    if (seeds) {
        renoise0 = noise;
        int n_re = 0;
        for (int i = 0; i < n_steps && !mx; ++i)
            if (renoise_std[i] >= 0.0f) n_re = i + 1;
        if (mx) n_re = mx->n_re;
        if (cmtts_launch_noise_fill(seeds, B, T, c.n_mels, 0, 1, 0, c.sigma_max, w.xcur, nullptr, (void*)s) != 0 ||
            (n_re && cmtts_launch_noise_fill(seeds, B, T, c.n_mels, 1, n_re, 0, 1.0f, const_cast<float*>(noise), nullptr, (void*)(ss ? ss->side : s)) != 0))
            return fail(CMTTS_E_HIP, "seeded noise launch failed");
    } else
        k_scale(noise, w.xcur, nel, c.sigma_max, s);        // x_T = randn * sigma_max (karras_diffusion.py:534)
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
    for (int i = 0; i < n_steps && mx; ++i) {
        // per-utterance schedules: the same evaluation on the prefix of utterances that still have one to take — every buffer is batch-major,
        // so the prefix is the same workspace with a smaller B.  The step embedding runs on all B rows (include/cmtts_hip.h: the K-slicing of
        // its MLP is a function of the row count), on the side stream in front of the first evaluation as below.
        const MixedEval& e = mx->ev[i];
        if (e.embed) {
            hipStream_t es = i == 0 && ss ? ss->side : s;
            if (e.t_uniform) k_fill_float(w.tbuf, e.t_host, B, es);
            CHK(step_embedding(m, w, e.t_uniform ? w.tbuf : e.t, speaker_emb, B, es, e.t_uniform ? e.t_host : NAN));
        }
        MelPost post = {w.xcur, e.renoise ? renoise0 + (long)i * noise_stride : nullptr, 0.0f, 0.0f, 0.0f, w.xcur};
        post.rows = e.rows; post.out_final = mel;
        CHK(denoiser_core(m, w, w.xcur, 1.0f, w.tbuf, cond_ct, speaker_emb, e.Bi, T, post, s, false, i == 0 ? ss : nullptr, NAN, cfk, &cp_ready, e.c_in));
        g_sample_rows += e.Bi;
    }
    for (int i = 0; i < n_steps && !mx; ++i) {
        // get_scalings_for_boundary_condition in fp32 (karras_diffusion.py:87-102)
        const float sg = sigmas[i];
        const float dm = sg - smin;
        const float c_skip = sd2 / (dm * dm + sd2);
        const float rt = sqrtf(sg * sg + sd2);
        const float c_out = dm * c.sigma_data / rt;
        const float c_in = 1.0f / rt;
        const float t_resc = 250.0f * logf(sg + 1e-44f);
        const bool new_sigma = i == 0 || sigmas[i] != sigmas[i - 1];
        // the first evaluation's step embedding reads only the timestep (and the speaker vector): side stream, beside x_T's scaling and the
        // input projection, joined with the conditioner branch before the residual layers (round 6; same kernels, same bits)
        const bool embed_side = i == 0 && ss != nullptr;
        if (new_sigma) k_fill_float(w.tbuf, t_resc, B, embed_side ? ss->side : s);
        if (embed_side) CHK(step_embedding(m, w, w.tbuf, speaker_emb, B, ss->side, t_resc));
        const bool last = i + 1 == n_steps;
        const bool renoise = renoise_std[i] >= 0.0f;
        const MelPost post = {w.xcur, renoise ? renoise0 + (long)i * noise_stride : nullptr, c_out, c_skip,
                              renoise ? renoise_std[i] : 0.0f, last ? mel : w.xcur};
        CHK(denoiser_core(m, w, w.xcur, c_in, w.tbuf, cond_ct, speaker_emb, B, T, post, s, new_sigma && !embed_side, i == 0 ? ss : nullptr, t_resc, cfk, &cp_ready));
        g_sample_rows += B;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The workspace of utterances [b0, B) of a batch carved for (B, T): every buffer is batch-major, so a sub-batch is a pointer offset
// (the halo granules are the persistent kernel's and are not used by the sub-batch path).
DenWs den_slice(const cmtts_config& c, const DenWs& w, int b0, int T) {
    const long C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    DenWs v = w;
    v.hin += (long)b0 * M * T; v.h += b0 * C * T; v.u += b0 * C * T; v.zb += b0 * C * T; v.skip += b0 * C * T;
    v.emb += b0 * C; v.e1 += b0 * 4 * C; v.e2 += b0 * C; v.dproj += b0 * NL * C; v.sproj += b0 * NL * C; v.dp += b0 * NL * C;
    v.tbuf += b0; v.xcur += (long)b0 * T * M; v.cp += (long)b0 * NL * C * T;
    return v;
}
}  // namespace
extern "C" {

int cmtts_sample(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T,
                 int n_steps, const float* sigmas, const float* renoise_std, float* mel, void* ws, size_t ws_bytes,
                 void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!noise || !cond_ct || !mel || !ws || !sigmas || !renoise_std || B <= 0 || T <= 0 || n_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_sample: bad argument");
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    DenWs w = carve_den(c, B, T, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "denoiser workspace too small");
    return sample_core(m, w, noise, (long)B * T * c.n_mels, cond_ct, speaker_emb, B, T, n_steps, sigmas, renoise_std, mel, (hipStream_t)stream);
}

// cmtts_sample for conditioning that cmtts_frame_forward_sub produced together with its phoneme-level factor `cond_p1`: the stacked
// conditioner GEMM over the frames is replaced by the expansion of the factors (cond_factored above).  cond_ct is still required
// (16-bit models and the unfused path use it); a NULL cond_p1 is cmtts_sample.
int cmtts_sample_factored(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T,
                          int n_steps, const float* sigmas, const float* renoise_std, float* mel, void* ws, size_t ws_bytes,
                          void* stream, const float* cond_p1, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx) {
    return cmtts_sample_factored_t(m, noise, cond_ct, speaker_emb, B, T, n_steps, sigmas, renoise_std, mel, ws, ws_bytes, stream, cond_p1, nullptr, p1_ld, L,
                                   mel2ph, p_idx);
}

int cmtts_sample_factored_t(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T,
                            int n_steps, const float* sigmas, const float* renoise_std, float* mel, void* ws, size_t ws_bytes,
                            void* stream, const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!noise || !cond_ct || !mel || !ws || !sigmas || !renoise_std || B <= 0 || T <= 0 || n_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_sample_factored: bad argument");
    if (cond_p1 && (!mel2ph || !p_idx || L <= 0 || p1_ld < L)) return fail(CMTTS_E_INVALID, "cmtts_sample_factored: incomplete factors");
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    DenWs w = carve_den(c, B, T, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "denoiser workspace too small");
    CondFactors cf;
    cf.p1 = cond_p1; cf.ldp = p1_ld; cf.L = L; cf.mel2ph = mel2ph; cf.p_idx = p_idx;
    cf.p1t = cond_p1 ? cond_p1t : nullptr;      // the caller's channel-contiguous copy (cmtts_frame_forward_sub_t): no transpose at the sampler's entry
    return sample_core(m, w, noise, (long)B * T * c.n_mels, cond_ct, speaker_emb, B, T, n_steps, sigmas, renoise_std, mel, (hipStream_t)stream,
                       cond_p1 ? &cf : nullptr);
}

// ---- seeded per-utterance noise (noise_philox.hip)
int cmtts_noise_fill(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, float* out, void* stream) {
    if (!seeds || !out || B < 1 || T < 1 || M < 1 || n_draws < 1 || first_draw < 0 || t0 < 0)
        return fail(CMTTS_E_INVALID, "cmtts_noise_fill: bad argument");
    const int rc = cmtts_launch_noise_fill(seeds, B, T, M, first_draw, n_draws, t0, 1.0f, out, nullptr, stream);
    if (rc == -2) return fail(CMTTS_E_UNSUPPORTED, "cmtts_noise_fill: B or n_draws > 65535, or T * ceil(M / 4) >= 2^31");
    if (rc != 0) return fail(CMTTS_E_HIP, "cmtts_noise_fill: launch failed");
    return 0;
}

int cmtts_noise_fill_groups(const cmtts_noise_group* groups, int n_groups, int M, int first_draw, int n_draws, void* stream) {
    if (!groups || n_groups < 1 || M < 1 || n_draws < 1 || first_draw < 0) return fail(CMTTS_E_INVALID, "cmtts_noise_fill_groups: bad argument");
    std::vector<NoiseGroup> gs((size_t)n_groups);
    for (int g = 0; g < n_groups; ++g) {
        const cmtts_noise_group& G = groups[g];
        if (!G.seeds || !G.out || G.B < 1 || G.T < 1) return fail(CMTTS_E_INVALID, "cmtts_noise_fill_groups: bad group");
        gs[g] = NoiseGroup{G.seeds, G.out, G.B, G.T, 0, 1};
    }
    const int rc = cmtts_launch_noise_fill_groups(gs.data(), n_groups, M, first_draw, n_draws, stream);
    if (rc == -2) return fail(CMTTS_E_UNSUPPORTED, "cmtts_noise_fill_groups: n_draws > 65535 or a launch of more than 2^31 - 1 workgroups");
    if (rc != 0) return fail(CMTTS_E_HIP, "cmtts_noise_fill_groups: launch failed");
    return 0;
}

int cmtts_internal_noise_bits(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, uint32_t* bits, void* stream) {
    if (!seeds || !bits || B < 1 || T < 1 || M < 1 || n_draws < 1 || first_draw < 0 || t0 < 0)
        return fail(CMTTS_E_INVALID, "cmtts_internal_noise_bits: bad argument");
    if (cmtts_launch_noise_fill(seeds, B, T, M, first_draw, n_draws, t0, 1.0f, nullptr, bits, stream) != 0)
        return fail(CMTTS_E_HIP, "cmtts_internal_noise_bits: launch failed");
    return 0;
}

// The denoiser workspace, then the re-noise draws 1 .. n_steps of the batch ([n_steps][B][1][T][n_mels], 256-byte aligned).
static size_t seeded_tail_offset(const cmtts_config& c, int B, int T) { return (carve_den(c, B, T, nullptr).bytes + 255) & ~(size_t)255; }
size_t cmtts_sample_seeded_workspace_bytes(const cmtts_model* m, int B, int T, int n_steps) {
    if (!m || B < 1 || T < 1 || n_steps < 1) return 0;
    return seeded_tail_offset(m->cfg, B, T) + (size_t)n_steps * B * T * m->cfg.n_mels * sizeof(float);
}

int cmtts_sample_seeded(cmtts_model* m, const int64_t* seeds, const float* cond_ct, const float* speaker_emb, int B, int T,
                        int n_steps, const float* sigmas, const float* renoise_std, float* mel, void* ws, size_t ws_bytes,
                        void* stream, const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!seeds || !cond_ct || !mel || !ws || !sigmas || !renoise_std || B <= 0 || T <= 0 || n_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_sample_seeded: bad argument");
    if (cond_p1 && (!mel2ph || !p_idx || L <= 0 || p1_ld < L)) return fail(CMTTS_E_INVALID, "cmtts_sample_seeded: incomplete factors");
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    if (B > 65535) return fail(CMTTS_E_UNSUPPORTED, "cmtts_sample_seeded: B > 65535");
    DenWs w = carve_den(c, B, T, ws);
    if (ws_bytes < cmtts_sample_seeded_workspace_bytes(m, B, T, n_steps)) return fail(CMTTS_E_WORKSPACE, "seeded sampler workspace too small");
    const float* tail = reinterpret_cast<const float*>(static_cast<char*>(ws) + seeded_tail_offset(c, B, T));
    CondFactors cf;
    cf.p1 = cond_p1; cf.ldp = p1_ld; cf.L = L; cf.mel2ph = mel2ph; cf.p_idx = p_idx;
    cf.p1t = cond_p1 ? cond_p1t : nullptr;
    return sample_core(m, w, tail, (long)B * T * c.n_mels, cond_ct, speaker_emb, B, T, n_steps, sigmas, renoise_std, mel, (hipStream_t)stream,
                       cond_p1 ? &cf : nullptr, seeds);
}

// ---- mixed step counts in one batch (include/cmtts_hip.h; the definition: cmtts_amd/steps.py)
// The seeded sampler's workspace (denoiser workspace, max_steps noise tensors), then the table: per evaluation c_in [B], t [B], PostRow [B].
static size_t mixed_table_offset(const cmtts_config& c, int B, int T, int max_steps) {
    return (seeded_tail_offset(c, B, T) + (size_t)max_steps * B * T * c.n_mels * sizeof(float) + 255) & ~(size_t)255;
}
static size_t mixed_eval_bytes(int B) { return (size_t)B * (2 * sizeof(float) + sizeof(PostRow)); }
size_t cmtts_sample_mixed_workspace_bytes(const cmtts_model* m, int B, int T, int max_steps) {
    if (!m || B < 1 || T < 1 || max_steps < 1) return 0;
    return mixed_table_offset(m->cfg, B, T, max_steps) + (size_t)max_steps * mixed_eval_bytes(B) + 256;
}

int cmtts_sample_mixed(cmtts_model* m, const int64_t* seeds, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T,
                       const cmtts_step_plan* plan, float* mel, void* ws, size_t ws_bytes, void* stream, const float* cond_p1,
                       const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!cond_ct || !mel || !ws || !plan || !plan->n_steps || !plan->sigmas || !plan->renoise_std || B <= 0 || T <= 0 || plan->max_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: bad argument");
    if ((seeds != nullptr) == (noise != nullptr)) return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: give seeds or noise (exactly one of them)");
    if (cond_p1 && (!mel2ph || !p_idx || L <= 0 || p1_ld < L)) return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: incomplete factors");
    const cmtts_config& c = m->cfg;
    if (c.multi_speaker && !speaker_emb) return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: speaker_emb is required for a multi-speaker model");
    const int NS = plan->max_steps;
    const int32_t* ns = plan->n_steps;
    if (ns[0] != NS) return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: n_steps[0] != max_steps");
    for (int b = 0; b < B; ++b) {
        if (ns[b] < 1 || ns[b] > NS) return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: n_steps[" + std::to_string(b) + "] outside [1, max_steps]");
        if (b && ns[b] > ns[b - 1])
            return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: n_steps must be non-increasing (utterance " + std::to_string(b) +
                                             "); sort the batch by step count first (cmtts_amd/steps.py: order)");
        for (int i = 0; i < ns[b]; ++i) {
            const float sg = plan->sigmas[(long)i * B + b];
            if (!(sg > 0.0f) || !(sg <= 3.402823466e38f))
                return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: sigma of utterance " + std::to_string(b) + ", evaluation " + std::to_string(i) +
                                                 " is not a finite positive number");
            if (!(plan->renoise_std[(long)i * B + b] >= 0.0f) && i + 1 != ns[b])
                return fail(CMTTS_E_INVALID, "cmtts_sample_mixed: only an utterance's last evaluation may go without re-noising (renoise_std < 0; utterance " +
                                                 std::to_string(b) + ")");
        }
    }
    CHK(check_batch_invariant(m));
    if (seeds && B > 65535) return fail(CMTTS_E_UNSUPPORTED, "cmtts_sample_mixed: B > 65535");
    if (ws_bytes < cmtts_sample_mixed_workspace_bytes(m, B, T, NS)) return fail(CMTTS_E_WORKSPACE, "mixed sampler workspace too small");
    DenWs w = carve_den(c, B, T, ws);
    const float* tail = reinterpret_cast<const float*>(static_cast<char*>(ws) + seeded_tail_offset(c, B, T));
    const long per = (long)B * T * c.n_mels;
    hipStream_t s = (hipStream_t)stream;
    CondFactors cf;
    cf.p1 = cond_p1; cf.ldp = p1_ld; cf.L = L; cf.mel2ph = mel2ph; cf.p_idx = p_idx;
    cf.p1t = cond_p1 ? cond_p1t : nullptr;
    // a uniform plan is the uniform sampler: same launches, same bits
    bool uniform = ns[B - 1] == NS;
    for (int i = 0; i < NS && uniform; ++i)
        for (int b = 1; b < B && uniform; ++b) {
            const float s0 = plan->renoise_std[(long)i * B], sb = plan->renoise_std[(long)i * B + b];
            uniform = plan->sigmas[(long)i * B + b] == plan->sigmas[(long)i * B] && (s0 >= 0.0f ? sb == s0 : !(sb >= 0.0f));
        }
    if (uniform) {
        std::vector<float> sg((size_t)NS), sd((size_t)NS);
        for (int i = 0; i < NS; ++i) { sg[i] = plan->sigmas[(long)i * B]; sd[i] = plan->renoise_std[(long)i * B]; }
        return sample_core(m, w, seeds ? tail : noise, per, cond_ct, speaker_emb, B, T, NS, sg.data(), sd.data(), mel, s, cond_p1 ? &cf : nullptr, seeds);
    }
    // the table: the scalings of every (evaluation, utterance) by sample_core's fp32 expressions, once
    const size_t eb = mixed_eval_bytes(B);
    std::vector<char> host((size_t)NS * eb);
    char* dev = static_cast<char*>(ws) + mixed_table_offset(c, B, T, NS);
    MixedPlan mx;
    mx.ev.resize((size_t)NS);
    std::vector<float> held((size_t)B, NAN);      // the timestep whose embedding row b of the workspace holds
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
    for (int i = 0; i < NS; ++i) {
        float* c_in = reinterpret_cast<float*>(host.data() + (size_t)i * eb);
        float* tt = c_in + B;
        PostRow* rows = reinterpret_cast<PostRow*>(tt + B);
        MixedEval& e = mx.ev[i];
        e.Bi = 0; e.embed = false; e.t_uniform = true; e.renoise = false;
        for (int b = 0; b < B; ++b) {
            if (i >= ns[b]) {      // left: the row is not evaluated; its timestep stays a valid one for the full-batch step embedding
                c_in[b] = 0.0f; tt[b] = held[b]; rows[b] = PostRow{0.0f, 0.0f, 0.0f, 0u};
                continue;
            }
            // get_scalings_for_boundary_condition in fp32 (karras_diffusion.py:87-102)
            const float sg = plan->sigmas[(long)i * B + b], nstd = plan->renoise_std[(long)i * B + b];
            const float dm = sg - smin;
            const float c_skip = sd2 / (dm * dm + sd2);
            const float rt = sqrtf(sg * sg + sd2);
            const float c_out = dm * c.sigma_data / rt;
            c_in[b] = 1.0f / rt;
            tt[b] = 250.0f * logf(sg + 1e-44f);
            const bool renoise = nstd >= 0.0f;
            rows[b] = PostRow{c_out, c_skip, renoise ? nstd : 0.0f, (renoise ? POSTROW_RENOISE : 0u) | (i + 1 == ns[b] ? POSTROW_FINAL : 0u)};
            e.Bi = b + 1;
            e.embed = e.embed || tt[b] != held[b];
            e.t_uniform = e.t_uniform && tt[b] == tt[0];
            e.renoise = e.renoise || renoise;
            if (renoise) mx.n_re = i + 1;
        }
        e.t_host = tt[0];
        if (e.embed)
            for (int b = 0; b < B; ++b) held[b] = e.t_uniform ? e.t_host : tt[b];
        e.c_in = reinterpret_cast<const float*>(dev + (size_t)i * eb);
        e.t = e.c_in + B;
        e.rows = reinterpret_cast<const PostRow*>(e.t + B);
    }
    HIPCHK(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, s));
    return sample_core(m, w, seeds ? tail : noise, per, cond_ct, speaker_emb, B, T, NS, nullptr, nullptr, mel, s, cond_p1 ? &cf : nullptr, seeds, &mx);
}

// Test hook (internal_hooks.h): utterance-evaluations launched by the last sampler call
long cmtts_internal_sample_rows(void) { return g_sample_rows; }

// ---- re-taking spans of an utterance: the masked sampler on frame windows (retake.hip)
}  // extern "C" (reopened below)
namespace {
// The denoiser workspace of the window batch (N, Tw), then the sampler's own buffers.
struct RetakeWs {
    DenWs den;
    float *x0, *known, *cond, *spk;
    int64_t* seeds;
    uint8_t* regen;
    StreamWindow* win;
    size_t bytes;
};
RetakeWs carve_retake(const cmtts_config& c, int N, int Tw, void* base) {
    RetakeWs r;
    r.den = carve_den(c, N, Tw, base);
    Carver cv(base);
    cv.off = r.den.bytes;
    const size_t nel = (size_t)N * Tw * c.n_mels;
    r.x0 = cv.take<float>(nel);
    r.known = cv.take<float>(nel);
    r.cond = cv.take<float>((size_t)N * c.hidden * Tw);
    r.spk = cv.take<float>((size_t)N * c.hidden);
    r.seeds = cv.take<int64_t>((size_t)N);
    r.regen = cv.take<uint8_t>((size_t)N * Tw);
    r.win = cv.take<StreamWindow>((size_t)N);
    r.bytes = cv.off + 256;
    return r;
}
// Every window inside [0, T], every core inside its window, the cores of one utterance disjoint.
bool retake_windows_ok(const int32_t* windows, int N, int B, int T, int Tw, std::string* why) {
    std::vector<std::array<long, 3>> cores;      // (utterance, first frame, end)
    for (int n = 0; n < N; ++n) {
        const int32_t b = windows[4 * n], start = windows[4 * n + 1], off = windows[4 * n + 2], len = windows[4 * n + 3];
        if (b < 0 || b >= B) { *why = "window " + std::to_string(n) + ": utterance out of range"; return false; }
        if (start < 0 || (long)start + Tw > T) { *why = "window " + std::to_string(n) + " reaches outside [0, T]"; return false; }
        if (off < 0 || len < 1 || (long)off + len > Tw) { *why = "window " + std::to_string(n) + ": core outside its window"; return false; }
        cores.push_back({(long)b, (long)start + off, (long)start + off + len});
    }
    std::sort(cores.begin(), cores.end());
    for (size_t k = 1; k < cores.size(); ++k)
        if (cores[k][0] == cores[k - 1][0] && cores[k][1] < cores[k - 1][2]) {
            *why = "two cores of utterance " + std::to_string(cores[k][0]) + " overlap";
            return false;
        }
    return true;
}
}  // namespace
extern "C" {

size_t cmtts_retake_workspace_bytes(const cmtts_model* m, int N, int Tw) {
    if (!m || N < 1 || Tw < 1) return 0;
    return carve_retake(m->cfg, N, Tw, nullptr).bytes;
}

int cmtts_retake(cmtts_model* m, const float* mel_known, const uint8_t* regen, const float* cond_ct, const float* speaker_emb, const int64_t* seeds,
                 int B, int T, const int32_t* windows, int N, int Tw, int n_steps, const float* sigmas, const float* renoise_std, float* mel_out,
                 void* ws, size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!mel_known || !regen || !cond_ct || !seeds || !windows || !sigmas || !renoise_std || !mel_out || !ws || B < 1 || T < 1 || N < 1 || Tw < 1 ||
        n_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_retake: bad argument");
    const cmtts_config& c = m->cfg;
    if (c.multi_speaker && !speaker_emb) return fail(CMTTS_E_INVALID, "cmtts_retake: speaker_emb is required for a multi-speaker model");
    if (Tw > T) return fail(CMTTS_E_INVALID, "cmtts_retake: Tw > T");
    for (int i = 0; i + 1 < n_steps; ++i)      // the kept frames of the next evaluation's input are known + noise at its sigma
        if (!(renoise_std[i] >= 0.0f)) return fail(CMTTS_E_INVALID, "cmtts_retake: only the last evaluation may go without re-noising (renoise_std < 0)");
    std::string why;
    if (!retake_windows_ok(windows, N, B, T, Tw, &why)) return fail(CMTTS_E_INVALID, "cmtts_retake: " + why);
    CHK(check_batch_invariant(m));
    if (N > 65535) return fail(CMTTS_E_UNSUPPORTED, "cmtts_retake: N > 65535");
    const RetakeWs w = carve_retake(c, N, Tw, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "retake workspace too small");
    const DenWs& d = w.den;
    const int M = c.n_mels;
    hipStream_t s = (hipStream_t)stream;
    // the window batch: everything is gathered before the first write to mel_out, which may be mel_known
    HIPCHK(hipMemcpyAsync(w.win, windows, (size_t)N * sizeof(StreamWindow), hipMemcpyHostToDevice, s));
    if (cmtts_launch_retake_gather(mel_known, regen, speaker_emb, seeds, w.win, N, T, Tw, M, c.hidden, w.known, w.regen, w.spk, w.seeds, (void*)s) != 0 ||
        cmtts_launch_mel_window_gather(cond_ct, c.hidden, T, w.win, N, Tw, w.cond, (void*)s) != 0)
        return fail(CMTTS_E_HIP, "cmtts_retake: gather launch failed");
    if (mel_out != mel_known) HIPCHK(hipMemcpyAsync(mel_out, mel_known, (size_t)B * T * M * sizeof(float), hipMemcpyDeviceToDevice, s));
    const float* spk = speaker_emb ? w.spk : nullptr;
    // sample_core's loop on the [N, Tw] batch, the dense conditioner GEMM on the side stream
    SideStream* ss = g_fused_resblock ? side_for(s) : nullptr;
    if (ss) CHK(branch_fork(ss));
    if (g_fused_resblock) CHK(cond_projections(m, d, w.cond, N, Tw, ss ? ss->side : s));
    RetakeStepArgs st;
    memset(&st, 0, sizeof(st));
    st.x0 = w.x0; st.known = w.known; st.regen = w.regen; st.seeds = w.seeds; st.win = w.win;
    st.N = N; st.Tw = Tw; st.M = M; st.T = T;
    st.out = d.xcur; st.draw = 0; st.scale = c.sigma_max; st.mode = RETAKE_INIT;
    if (cmtts_launch_retake_step(&st, (void*)s) != 0) return fail(CMTTS_E_HIP, "cmtts_retake: first-draw launch failed");
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
    for (int i = 0; i < n_steps; ++i) {
        const float sg = sigmas[i];
        const float dm = sg - smin;
        const float c_skip = sd2 / (dm * dm + sd2);
        const float rt = sqrtf(sg * sg + sd2);
        const float c_out = dm * c.sigma_data / rt;
        const float c_in = 1.0f / rt;
        const float t_resc = 250.0f * logf(sg + 1e-44f);
        const bool new_sigma = i == 0 || sigmas[i] != sigmas[i - 1];
        const bool embed_side = i == 0 && ss != nullptr;
        if (new_sigma) k_fill_float(d.tbuf, t_resc, N, embed_side ? ss->side : s);
        if (embed_side) CHK(step_embedding(m, d, d.tbuf, spk, N, ss->side, t_resc));
        const bool last = i + 1 == n_steps;
        const MelPost post = {d.xcur, nullptr, c_out, c_skip, 0.0f, w.x0};      // x0 = c_out F + c_skip x, exactly as the plain sampler forms it
        CHK(denoiser_core(m, d, d.xcur, c_in, d.tbuf, w.cond, spk, N, Tw, post, s, new_sigma && !embed_side, i == 0 ? ss : nullptr, t_resc));
        st.draw = 1 + i; st.scale = renoise_std[i];
        st.mode = last ? RETAKE_LAST : RETAKE_MID;
        st.out = last ? mel_out : d.xcur;
        if (cmtts_launch_retake_step(&st, (void*)s) != 0) return fail(CMTTS_E_HIP, "cmtts_retake: step launch failed");
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Test hook (internal_hooks.h): retake_step_kernel alone on the caller's device buffers
int cmtts_internal_retake_step(const float* x0, const float* known, const uint8_t* regen, const int64_t* seeds, const int32_t* windows, int N, int Tw,
                               int M, int T, int draw, float scale, int mode, float* out, void* stream) {
    if (!seeds || !windows || !out || N < 1 || Tw < 1 || M < 1 || T < Tw || draw < 0 || mode < RETAKE_INIT || mode > RETAKE_LAST ||
        (mode != RETAKE_INIT && (!x0 || !regen)) || (mode == RETAKE_MID && !known))
        return fail(CMTTS_E_INVALID, "cmtts_internal_retake_step: bad argument");
    RetakeStepArgs st;
    memset(&st, 0, sizeof(st));
    st.x0 = x0; st.known = known; st.regen = regen; st.seeds = seeds; st.win = reinterpret_cast<const StreamWindow*>(windows);
    st.N = N; st.Tw = Tw; st.M = M; st.T = T; st.out = out; st.draw = draw; st.scale = scale; st.mode = mode;
    if (cmtts_launch_retake_step(&st, stream) != 0) return fail(CMTTS_E_HIP, "cmtts_internal_retake_step: launch failed");
    return 0;
}

// karras_sample_tts for a RAGGED shard (BASELINE.json configs[3]: utterances dealt into static frame buckets): every group is a
// padded (B, T) batch with its own buffers — results are defined per padded bucket (model/modules.py:429-430 via model/cmtts.py:61-62)
// — but the residual layers of ALL groups run in ONE persistent launch per evaluation (denoiser_persist.hip, RAGGED instance), so that
// small buckets fill the chip together instead of one after the other.
int cmtts_sample_ragged(cmtts_model* m, const cmtts_sample_group* groups, int n_groups, int n_steps, const float* sigmas,
                        const float* renoise_std, int tail_frames, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!groups || n_groups < 1 || n_steps < 1 || !sigmas || !renoise_std || tail_frames < 0)
        return fail(CMTTS_E_INVALID, "cmtts_sample_ragged: bad argument");
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    hipStream_t s = (hipStream_t)stream;
    long padded_tiles = 0;
    for (int g = 0; g < n_groups; ++g) {
        const cmtts_sample_group& G = groups[g];
        if (!G.noise || !G.cond_ct || !G.mel || !G.ws || G.B <= 0 || G.T <= 0) return fail(CMTTS_E_INVALID, "cmtts_sample_ragged: bad group");
        if (c.multi_speaker && !G.speaker_emb) return fail(CMTTS_E_INVALID, "speaker_emb is required for a multi-speaker model");
        if (G.ws_bytes < carve_den(c, G.B, G.T, nullptr).bytes) return fail(CMTTS_E_WORKSPACE, "denoiser workspace too small");
        padded_tiles += (long)G.B * ((G.T + 63) / 64);
    }
    // the one-launch form needs the fp32 persistent kernel with its in-kernel tail; anything else (16-bit modes, switches off, more
    // groups / longer utterances than a descriptor holds, too little work to beat the per-layer kernels) runs group after group
    bool one_launch = m->precision == 0 && g_fused_resblock && g_persist && g_persist_tail && g_inproj_fused && m->skip_f && m->outp_f &&
                      m->in_proj_f && NL <= PERSIST_MAX_LAYERS && n_groups <= PERSIST_MAX_GROUPS && padded_tiles * 2 > persist_blocks();
    // (an utterance with more tiles than the launch can keep resident is known NOW: fall back before anything is queued — ADVICE r03)
    for (int g = 0; g < n_groups && one_launch; ++g)
        if ((groups[g].T + 63) / 64 > 127 || (groups[g].T + 63) / 64 > std::min(persist_blocks(), PERSIST_MAX_WG) || groups[g].B > 1023 || (long)C * groups[g].T >= (1L << 30) ||
            cmtts_persist_halo_bytes(groups[g].B, groups[g].T) % 16 != 0)
            one_launch = false;
    if (!one_launch) {
        for (int g = 0; g < n_groups; ++g) {
            const cmtts_sample_group& G = groups[g];
            const int rc = cmtts_sample_factored(m, G.noise, G.cond_ct, G.speaker_emb, G.B, G.T, n_steps, sigmas, renoise_std, G.mel, G.ws, G.ws_bytes,
                                                 stream, G.cond_p1, G.p1_ld, G.L, G.mel2ph, G.p_idx);
            if (rc != 0) return rc;
        }
        return 0;
    }
    CHK(check_device_flag(true));
    // ---- which utterances share the persistent launch.  Every workgroup of that launch must be resident, so a shard with more active
    // tiles than CUs needs a second ROUND of 20 layers (2.7 ms per evaluation whatever its size).  When leaving out a few SMALL
    // utterances (<= 64 active tiles together: the range where the per-layer / split kernels take < 1 ms per evaluation,
    // tools/split_crossover.py) makes the rest fit one round, those go through the ordinary sampler on the side stream instead: 2.7 +
    // ~0.9 ms per evaluation where two rounds cost 5.4.  They are taken from the END of the groups with the shortest padded length
    // (a sub-batch [b0, B) of a group is a pointer offset: every buffer is batch-major); keep[g] = utterances of group g that stay.
    const int cap_all = std::min(persist_blocks(), PERSIST_MAX_WG);
    auto utt_tiles = [&](const cmtts_sample_group& G, int b, int eval) {
        const int tiles = (G.T + 63) / 64;
        if (!G.active_frames) return (long)tiles;
        const long need = (long)G.active_frames[b] + tail_frames + (long)NL * (n_steps - eval);
        return std::min<long>(tiles, std::max<long>(1, (need + 63) / 64));
    };
    std::vector<int> keep(n_groups);
    {
        long total = 0;
        for (int g = 0; g < n_groups; ++g) {
            keep[g] = groups[g].B;
            for (int b = 0; b < groups[g].B; ++b) total += utt_tiles(groups[g], b, 0);
        }
        if (total > cap_all) {
            std::vector<int> order(n_groups), k2 = keep;
            for (int g = 0; g < n_groups; ++g) order[g] = g;
            std::sort(order.begin(), order.end(), [&](int x, int y) { return groups[x].T < groups[y].T; });
            long out = 0, rest = total;
            for (int g : order) {
                while (rest > cap_all && k2[g] > 0) {
                    const long t = utt_tiles(groups[g], k2[g] - 1, 0);
                    out += t; rest -= t; --k2[g];
                }
                if (rest <= cap_all) break;
            }
            if (rest <= cap_all && rest > 0 && out <= 64) keep = k2;
        }
    }
    // every group that takes part in the one launch brings usable conditioner factors: the FACT instance of the ragged kernel
    bool fact_all = g_cond_inkernel != 0;
    for (int g = 0; g < n_groups && fact_all; ++g) {
        if (keep[g] == 0) continue;
        CondFactors cf;
        cf.p1 = groups[g].cond_p1; cf.ldp = groups[g].p1_ld; cf.L = groups[g].L; cf.mel2ph = groups[g].mel2ph; cf.p_idx = groups[g].p_idx;
        if (!cf.usable(m) || groups[g].p1_ld > groups[g].T || !m->cond_p2t) fact_all = false;
    }
    std::vector<DenWs> ws(n_groups);
    SideStream* ss = side_for(s);
    // whatever path leaves this function after a fork, the caller's stream is ordered behind the side stream again
    struct JoinGuard {
        SideStream* ss; bool armed;
        ~JoinGuard() { if (armed && ss) (void)branch_join(ss); }
    } guard{ss, false};
    if (ss) { CHK(branch_fork(ss)); guard.armed = true; }
    bool any_aside = false;
    for (int g = 0; g < n_groups; ++g) {
        const cmtts_sample_group& G = groups[g];
        ws[g] = carve_den(c, G.B, G.T, G.ws);
        if (keep[g] < G.B) any_aside = true;
        if (keep[g] == 0) continue;
        CondFactors cf;
        cf.p1 = G.cond_p1; cf.ldp = G.p1_ld; cf.L = G.L; cf.mel2ph = G.mel2ph; cf.p_idx = G.p_idx;
        if (fact_all) {   // the ragged FACT instance gathers the factors itself: no cp tensor — the buffer takes p1 with the channels contiguous
            k_transpose(G.cond_p1, ws[g].cp, keep[g] * NL, C, G.p1_ld, s);
        }
        else if (cf.usable(m)) CHK(cond_factored(m, ws[g], cf, keep[g], G.T, ss ? ss->side : s));
        else CHK(cond_projections(m, ws[g], G.cond_ct, keep[g], G.T, ss ? ss->side : s));   // once for all evaluations, beside the first prologues
        k_scale(G.noise, ws[g].xcur, (long)keep[g] * G.T * M, c.sigma_max, s);         // x_T = randn * sigma_max (karras_diffusion.py:534)
        if (G.active_frames) HIPCHK(hipMemsetAsync(G.mel, 0, (size_t)keep[g] * G.T * M * sizeof(float), s));   // frames beyond the trimmed range: zeros
    }
    if (ss) { guard.armed = false; CHK(branch_join(ss)); }          // the conditioner projections; the side stream then carries the set-aside groups
    if (any_aside) {
        // the small groups: the ordinary sampler (per-layer / split kernels), queued on the side stream so that its launches fill the
        // gaps of the main stream (prologues, launch boundaries) and whatever CUs the persistent grid leaves free
        hipStream_t q = ss ? ss->side : s;
        if (ss) { CHK(branch_fork(ss)); guard.armed = true; }
        const int prev_persist = g_persist;
        g_persist = 0;
        int rc = 0;
        for (int g = 0; g < n_groups && rc == 0; ++g)
            if (keep[g] < groups[g].B) {
                const cmtts_sample_group& G = groups[g];
                const int b0 = keep[g], nb = G.B - b0;
                const long per = (long)G.T * M;
                CondFactors cf;
                cf.p1 = G.cond_p1 ? G.cond_p1 + (long)b0 * NL * C * G.p1_ld : nullptr; cf.ldp = G.p1_ld; cf.L = G.L;
                cf.mel2ph = G.mel2ph ? G.mel2ph + (long)b0 * G.T : nullptr; cf.p_idx = G.p_idx ? G.p_idx + (long)b0 * G.T : nullptr;
                rc = sample_core(m, den_slice(c, ws[g], b0, G.T), G.noise + b0 * per, (long)G.B * per, G.cond_ct + (long)b0 * c.hidden * G.T,
                                 G.speaker_emb ? G.speaker_emb + (long)b0 * c.hidden : nullptr, nb, G.T, n_steps, sigmas, renoise_std,
                                 G.mel + b0 * per, q, &cf);
            }
        g_persist = prev_persist;
        if (rc != 0) return rc;
    }
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
    const int cap = cap_all;
    PersistArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.vec_stride = (long)NL * C; pa.tmo = g_tmo_host; pa.NL = NL; pa.halo_zeroed = 1;
    pa.tail = 1;
    pa.Wsf = m->skip_f; pa.bs = m->skip_proj.bias; pa.Wpf = m->outp_f; pa.bp = m->out_proj.bias;
    pa.skip_div = (float)sqrt((double)NL); pa.n_mels = M;
    pa.wino = g_persist_wino && m->winograd && m->res[0].w3w;
    for (int g = 0; g < n_groups && pa.wino; ++g)
        if (keep[g] > 0 && !ws[g].pst) pa.wino = 0;
    if (pa.wino && g_persist_wino == 3 && m->winograd == 1 && m->res[0].w3w43) pa.wino = 3;
    for (int l = 0; l < NL; ++l) {
        pa.W3f[l] = pa.wino == 3 ? m->res[l].w3w43 : pa.wino ? m->res[l].w3w : m->res[l].w3f; pa.Wof[l] = m->res[l].wof; pa.b3[l] = m->res[l].b3f; pa.bo[l] = m->res[l].outp.bias;
    }
    pa.n_groups = n_groups;
    if (fact_all) { pa.fact = 1; pa.p2 = m->cond_p2; pa.p2t = m->cond_p2t; pa.ld2 = c.pitch_bins; }
    for (int i = 0; i < n_steps; ++i) {
        // get_scalings_for_boundary_condition in fp32 (karras_diffusion.py:87-102)
        const float sg = sigmas[i];
        const float dm = sg - smin;
        const float c_skip = sd2 / (dm * dm + sd2);
        const float rt = sqrtf(sg * sg + sd2);
        const float c_out = dm * c.sigma_data / rt;
        const float c_in = 1.0f / rt;
        const float t_resc = 250.0f * logf(sg + 1e-44f);
        const bool new_sigma = i == 0 || sigmas[i] != sigmas[i - 1];
        const bool last = i + 1 == n_steps;
        const bool renoise = renoise_std[i] >= 0.0f;
        // an output frame depends on NL frames of input to either side (NL k = 3 layers): evaluation i must be exact on every frame the
        // later evaluations and the caller's `tail_frames` reach, so it is computed NL * (n_steps - i) frames beyond that
        struct Utt { int g, b, act; };
        std::vector<Utt> utts;
        long total = 0;
        for (int g = 0; g < n_groups; ++g) {
            const cmtts_sample_group& G = groups[g];
            const int Bk = keep[g];
            if (Bk == 0) continue;
            const DenWs& w = ws[g];
            if (new_sigma) k_fill_float(w.tbuf, t_resc, Bk, s);
            bool hz = false;
            CHK(denoiser_prologue(m, w, w.xcur, c_in, w.tbuf, G.speaker_emb, Bk, G.T, s, new_sigma, t_resc, &hz));
            if (!hz) HIPCHK(hipMemsetAsync(w.halo, 0, cmtts_persist_halo_bytes(Bk, G.T), s));
            const int tiles = (G.T + 63) / 64;
            PersistGroup& pg = pa.grp[g];
            pg.x0 = w.h; pg.cp = w.cp; pg.cp_bstride = (long)NL * C * G.T;
            pg.dp = c.multi_speaker ? w.dp : w.dproj; pg.d = w.dproj; pg.skip = w.skip; pg.xst = w.pst; pg.halo = w.halo;
            pg.xold = w.xcur; pg.noise = renoise ? G.noise + (long)(1 + i) * G.B * G.T * M : nullptr; pg.out = last ? G.mel : w.xcur;
            pg.B = Bk; pg.T = G.T; pg.tiles = tiles;
            if (fact_all) { pg.p1 = G.cond_p1; pg.p1t = w.cp; pg.mel2ph = (const long long*)G.mel2ph; pg.pidx = (const long long*)G.p_idx; pg.ldp = G.p1_ld; pg.Lph = G.L; }
            for (int b = 0; b < Bk; ++b) {
                const int act = (int)utt_tiles(G, b, i);
                utts.push_back({g, b, act});
                total += act;
            }
        }
        pa.c_out = c_out; pa.c_skip = c_skip; pa.nstd = renoise ? renoise_std[i] : 0.0f;
        // rounds: every workgroup of a launch must be resident, so a shard with more active tiles than CUs runs as balanced rounds of
        // whole utterances (tiles of one utterance exchange their edge columns and must share a launch)
        const int nrounds = (int)((total + cap - 1) / cap);
        const long target = (total + nrounds - 1) / nrounds;
        size_t u = 0;
        while (u < utts.size()) {
            int n = 0;
            while (u < utts.size() && n + utts[u].act <= cap && (n == 0 || n + utts[u].act <= target + 8)) {
                for (int t = 0; t < utts[u].act; ++t)
                    pa.desc[n++] = (unsigned)utts[u].g | ((unsigned)utts[u].b << 3) | ((unsigned)t << 13) | ((unsigned)utts[u].act << 20);
                ++u;
            }
            if (n == 0) return fail(CMTTS_E_UNSUPPORTED, "cmtts_sample_ragged: an utterance has more 64-frame tiles than the GPU has CUs");
            pa.n_wg = n;
            const bool prof = g_prof.on && g_prof.used + 2 <= g_prof.ev.size();
            CHK(persist_admit(s, n, persist_blocks()));
            if (prof) (void)hipEventRecord(g_prof.ev[g_prof.used], s);
            const int rc = cmtts_launch_denoiser_persist_ragged(&pa, (void*)s);
            if (rc != 0) return fail(rc == -2 ? CMTTS_E_UNSUPPORTED : CMTTS_E_HIP, "ragged persistent denoiser launch failed");
            CHK(persist_launched(s, n));
            if (prof) { (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s); g_prof.used += 2; }
        }
    }
    if (any_aside && ss) { guard.armed = false; CHK(branch_join(ss)); }
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
        {"resblock_split", &g_split_resblock, 0, 2},     // fp32 residual block as two launches over 4x the CUs: 0 never, 1 small batches, 2 always
        {"step_cache", &g_step_cache, 0, 1},             // cmtts_sample: keep the timestep-only step-embedding rows on the device
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
    static const Knob tab[] = {
        {"cond_inkernel", &g_cond_inkernel, 0, 1}, // fp32 persistent denoiser gathers the conditioner factors itself (same bits as expanding them into cp first)
        {"cond_factored", &g_cond_factored, 0, 1}, // fp32 models: conditioner projections expanded from their phoneme-level / pitch-table factors when the caller hands them over (NOT bitwise the dense GEMM: W a + W b against W (a + b))
        {"cond_gemm16", &g_cond_gemm16, 0, 1},     // 16-bit models: conditioner GEMM with 16-bit operands (NOT bitwise: another operand precision)
        {"cond_gemm", &g_cond_gemm, 0, 2},         // stacked conditioner GEMM on cond_gemm.hip: 0 never, 1 when it pays, 2 whenever supported
        {"persist_tail", &g_persist_tail, 0, 1},   // skip head + post-scaling inside the persistent launch
        {"persist_wino", &g_persist_wino, 0, 3},   // fp32 persistent denoiser's k = 3 conv: 0 direct, 1 (and 2) Winograd F(2,3), 3 F(4,3) (NOT bitwise the direct form)
        {"inproj_fused", &g_inproj_fused, 0, 1},   // denoiser input as one launch
    };
    if (!strcmp(name, "attn_qb")) return cmtts_attention_set_qb(value);       // attention.hip: queries split over workgroups (round 6; same bits)
    if (!strcmp(name, "xres_nt")) return cmtts_xres_set_nt(value);            // conv_xres tile width for launches that do not choose one (measurements)      // conv_xl: m-tiles over several workgroups for launches of a few column tiles
    bool found;
    int prev = vocoder_internal_set(name, value, &found);      // vocoder.hip: voc_*, post_v4
    if (found) return prev;
    prev = text_internal_set(name, value, &found);             // text_side.hip: the FFT blocks', predictors' and frame side's switches
    if (found) return prev;
    prev = knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, &found);
    if (found) return prev;
    return fail(CMTTS_E_INVALID, "cmtts_internal_set: unknown switch");
}

int cmtts_internal_cond_projections(cmtts_model* m, const float* cond_ct, int B, int T, float* cp, void* stream) {
    if (!m || !cond_ct || !cp || B <= 0 || T <= 0) return fail(CMTTS_E_INVALID, "cmtts_internal_cond_projections: bad argument");
    DenWs w;
    memset(&w, 0, sizeof(w));
    w.cp = cp;
    return cond_projections(m, w, cond_ct, B, T, (hipStream_t)stream);
}

// Test hook: the conditioner projections expanded from their factors (cond_factored) into cp [B][NL*C][T]
int cmtts_internal_cond_factored(cmtts_model* m, const float* p1, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx, int B, int T,
                                 float* cp, void* stream) {
    if (!m || !m->finalized || !p1 || !mel2ph || !p_idx || !cp) return fail(CMTTS_E_INVALID, "cmtts_internal_cond_factored: bad argument");
    if (!m->cond_p2) return fail(CMTTS_E_UNSUPPORTED, "no pitch-table factor for this model");
    DenWs w;
    memset(&w, 0, sizeof(w));
    w.cp = cp;
    CondFactors cf;
    cf.p1 = p1; cf.ldp = p1_ld; cf.L = L; cf.mel2ph = mel2ph; cf.p_idx = p_idx;
    return cond_factored(m, w, cf, B, T, (hipStream_t)stream);
}

int cmtts_poll_error(void) { return check_device_flag(); }

int cmtts_set_persistent_denoiser(int mode) {
    const int prev = g_persist;
    if (mode >= 0 && mode <= 2) g_persist = mode;
    return prev;
}

int cmtts_set_fused_resblock(int on) {
    const int prev = g_fused_resblock ? 1 : 0;
    g_fused_resblock = on != 0;
    return prev;
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

int cmtts_set_resblock_tile(int frames) {
    if (frames != 0 && frames != 32 && frames != 64) return fail(CMTTS_E_INVALID, "cmtts_set_resblock_tile: 0, 32 or 64");
    cmtts_resblock_set_tile(frames);
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

int cmtts_profile_begin(int max_launches, int stride) {
    if (max_launches <= 0 || stride <= 0) return fail(CMTTS_E_INVALID, "cmtts_profile_begin: bad argument");
    g_prof.stride = stride;
    g_prof.seen = 0;
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.assign((size_t)max_launches * 2, nullptr);
    for (auto& e : g_prof.ev) HIPCHK(hipEventCreate(&e));
    g_prof.used = 0;
    g_prof.on = true;
    return 0;
}
int cmtts_profile_end(double* total_ms, int* n_launches) {
    if (!total_ms || !n_launches) return fail(CMTTS_E_INVALID, "cmtts_profile_end: bad argument");
    g_prof.on = false;
    double tot = 0.0;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        HIPCHK(hipEventSynchronize(g_prof.ev[i + 1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *n_launches = (int)(g_prof.used / 2);
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear();
    g_prof.used = 0;
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
