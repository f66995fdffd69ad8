// C ABI of the MI355X-native CM-TTS inference hot path (include/cmtts_hip.h): the entry points, workspace carving and the
// host-side launch sequences (weight import: import.hip; handles: model.h; the vocoder: vocoder.hip, shared helpers: launch.h).  No allocation and no
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

// What launch.h declares, for this unit and vocoder.hip
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
extern "C" int cmtts_launch_conv_xresq(const ConvArgs* a, const float* wq, int nbatch, void* stream, int form);      // conv_xres.hip
int g_ffn_wino = 1;             // FFT blocks, fp32: the k = 9 FFN conv of the fused launch as three Winograd tap groups (conv_xres.hip WQ instances; NOT bitwise the direct form: fp32
                                // rounding): 1 (default since round 6) = F(2,3) over output pairs, 2 = F(4,3) over output quads (round 5's default), 0 = direct.  Every fp32 FFN
                                // whose shape the X-resident kernel covers then takes it — whatever L and B — so that the text side's bits, and with them durations and lengths,
                                // still do not depend on the batch.
int g_ffn_fused = 1;            // FFT blocks: the FFN linear's K-segment partial products formed inside the k = 9 conv's launch (conv_xres.hip; same bits); 0 = its own launch
int g_inproj_fused = 1;         // denoiser input: c_in scaling + transpose + input projection + halo clearing in one launch (same bits); 0 = three launches
int g_step_cache = 1;           // cmtts_sample: reuse the timestep-only part of the step embedding across calls (same bits); 0 = recompute every call
int g_persist_wino = 3;         // fp32 persistent denoiser: the k = 3 conv in a Winograd form (NOT bitwise the direct form): 3 = F(4,3), the 8-wave WINO == 2 instances
                                // of denoiser_persist.hip (default since round 5: half of the conv's MFMAs), 1 = F(2,3), the 8-wave WINO == 1 instances (2/3), 0 = direct
                                // (2 was round 5's one-wave-per-SIMD F(2,3) stack — same bits as 1, measured 4-10 % slower, out of the build since round 6: tools/attic/ — and runs as 1)
int g_pred_xl = 1;              // frame-level 256 -> 256 predictor convs on the X-resident conv_xl kernel (bitwise equal); 0 = generic kernel
int g_pred_head = 1;            // predictors: last LayerNorm + linear head as one launch (ln_linear_kernel); 0 = layernorm_ct + chan_linear
int g_text_xres = 7;            // FFT blocks, bit mask: 1 = LayerNorm1 + in-projection in one X-resident launch, 2 = out-projection on that kernel (round 4: its 32-column instance, default on), 4 = LayerNorm2 as the prologue of the FFN conv; 0 = separate LayerNorm launches
int g_attn_fused = 1;           // FFT-block attention as QKV projection + ONE fused kernel (attention.hip; key-chunked with an online softmax above L = 192): 0 = three-launch path
int g_qkv_nt = 0;              // internal switch "qkv_nt": conv_xres tile width of the in-projection (0 = launcher's rule, 1, 3) — measurements
int g_stats_mlp = 1;           // round 6: cwt_stats_layers as one launch (kernels.hip: stats_mlp_kernel; same bits); 0 = three dense_small launches
int g_cwt_in_phoneme = 1;      // round 4: the pitch predictor's input projection applied before the length regulator (same bits); 0 = over the frames
int g_xres_small = 1;          // round 4: conv_xres with 32-column tiles for text-side launches that cannot fill the chip (same bits); 0 = the generic kernel there
int g_ffn_xres = 1;            // encoder k=9 FFN conv through conv_xres.hip when the shape suits it (false: generic kernel)
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

constexpr long SPLIT_MAX_TILES = 176;    // 32-frame tiles up to which the two-launch residual block wins (tools/split_crossover.py: 0.88 vs 1.86 ms per evaluation up to 64 tiles, 1.46 vs 2.08 at 128, 2.00 vs 2.19 at 192, 2.65 vs 2.39 at 256)

int persist_blocks() {          // workgroups that are certainly co-resident: one 1024-thread workgroup per CU
    static int n = [] { int dev = 0, v = 0; (void)hipGetDevice(&dev);
                        (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev); return v; }();
    return n;
}

// ---------------------------------------------------------------- workspaces
// The FFN linear (K = 4 H = 1024 -> H) is DEFINED as FFN2_SEG partial sums over 128-row K segments, added in ascending order,
// then + bias, + residual, mask — for every batch size and path: the segments are independent GEMMs (8x the workgroups of a
// launch whose single 1024-long accumulation chain per tile left most of the chip waiting: 60 us for 1.4 GFLOP) and a
// batch's values still do not depend on its size.
constexpr int FFN2_SEG = 8;
struct TextWs {
    float *x, *h, *qk, *vt, *st, *o, *f, *part, *c1, *c2, *spk, *out1, *h128, *logd, *dround, *epred, *escaled, *pctl;
    int* cum;
    int64_t *eidx, *mlen;
    size_t bytes;
};
TextWs carve_text(const cmtts_config& c, int B, int L, void* base) {
    const int Lp = round_up(L, 4), H = c.hidden;
    Carver cv(base);
    TextWs w;
    const size_t n = (size_t)B * H * Lp;
    // persistent state (read by cmtts_frame_forward) first
    w.out1 = cv.take<float>(n);
    w.cum = cv.take<int>((size_t)B * L);
    w.spk = cv.take<float>((size_t)B * H);
    w.h128 = cv.take<float>((size_t)B * c.cwt_hidden * Lp);      // cwt_predictor[0] applied at the phoneme level (round 4): [B][cwt_hidden][Lp]
    w.x = cv.take<float>(n);
    w.h = cv.take<float>(n);
    w.qk = cv.take<float>(3 * n);      // fused attention: [B][3H][Lp] (Q | K | V); three-launch path: Q,K [B][2H][Lp] + V^T [B][Lp][H] behind it
    w.vt = w.qk + 2 * n;
    w.st = cv.take<float>((size_t)B * c.enc_heads * Lp * Lp);
    w.o = cv.take<float>(n);
    w.f = cv.take<float>(4 * n);
    w.part = cv.take<float>(FFN2_SEG * n);     // partial sums of the FFN linear, one [B][H][Lp] slab per K segment
    w.c1 = cv.take<float>(n);
    w.c2 = cv.take<float>(n);
    w.logd = cv.take<float>((size_t)B * L);
    w.dround = cv.take<float>((size_t)B * L);
    w.epred = cv.take<float>((size_t)B * L);
    w.eidx = cv.take<int64_t>((size_t)B * L);
    w.mlen = cv.take<int64_t>((size_t)B);
    w.escaled = cv.take<float>((size_t)B * L);      // energy prediction x control (behind everything else: the other offsets do not depend on it)
    w.pctl = cv.take<float>((size_t)B * L);         // the pitch control table's rows (cmtts_set_control_tables): persistent state like cum — the frame side reads it, a text-state record carries it
    w.bytes = cv.off + 256;
    return w;
}

struct FrameWs {
    float *xlr, *h128, *hp, *c1, *c2, *cwt, *r, *s1, *s2, *stats, *f0;
    int64_t* pidx;
    size_t bytes;
};
FrameWs carve_frame(const cmtts_config& c, int B, int T, void* base) {
    Carver cv(base);
    FrameWs w;
    const size_t n = (size_t)B * c.hidden * T;
    w.xlr = cv.take<float>(n);
    w.h128 = cv.take<float>((size_t)B * c.cwt_hidden * T);
    w.hp = cv.take<float>((size_t)B * c.cwt_hidden * T);
    w.c1 = cv.take<float>(n);
    w.c2 = cv.take<float>(n);
    w.cwt = cv.take<float>((size_t)B * T * 16);
    w.r = cv.take<float>((size_t)B * T);
    w.s1 = cv.take<float>((size_t)B * c.cwt_hidden);
    w.s2 = cv.take<float>((size_t)B * c.cwt_hidden);
    w.stats = cv.take<float>((size_t)B * 2);
    w.f0 = cv.take<float>((size_t)B * T);
    w.pidx = cv.take<int64_t>((size_t)B * T);
    w.bytes = cv.off + 256;
    return w;
}

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

// conv stack of Duration/Pitch/Energy predictors (model/modules.py:477-487): Conv1d + ReLU ->
// LayerNorm over channels (eps 1e-12) [-> mask].  Result ends in bufB.
// conv -> ReLU -> LayerNorm blocks of a predictor followed by its linear head (model/modules.py:470-506, 520-554): the last
// block's LayerNorm and the head are one launch (ln_linear_kernel) unless cmtts_internal_set("pred_head", 0)
// mode16: 0, or the 16-bit operand mode (1 = bf16, 2 = fp16) of a model with the opt-in "text16": the convs on conv_mfma16.hip (bias + ReLU in fp32)
struct EnergyHead {        // round 6: get_energy_embedding + the embedding add (model/modules.py:318-328,358-363) as the epilogue of the energy predictor's head (kernels.hip: ln_linear_kernel<1, true>)
    const float* xin; const float* e_target; float e_control; const float* bins; int nbins; const float* E; float* out1; int64_t* e_idx; float* e_scaled;
    bool done;
    const float* e_table = nullptr;      // control table [B][T] in place of e_control (ln_linear_kernel<1, 2>)
};
int g_energy_head = 1;          // internal switch "energy_head": 1 = in the head's launch (same bits), 0 = energy_embed_kernel behind the join
int g_pred_wino = 1;            // round 6: the frame-level pitch predictor's k = 5 convs as F(4,3) tap groups (conv_k5q.hip; NOT bitwise the direct form: fp32 Winograd rounding), at every launch size
int g_pred_xres = 1;            // round 4: phoneme-level 256 -> 256 predictor convs on conv_xres (32-column tiles), the previous block's LayerNorm as its prologue (same bits); 0 = generic kernel + LayerNorm launches
int predictor(const Predictor& P, const float* in, int ld_in, int B, int T, int ld, const int64_t* ln_lens,
              const int64_t* out_lens, float* bufA, float* bufB, float* out, int O, hipStream_t s, int mode16 = 0, bool frame_level = false,
              EnergyHead* eh = nullptr) {      // eh: the energy predictor — bucketize + embedding add inside the head's launch (eh->done reports it)
    const float* cur = in;
    int ldc = ld_in;
    auto other = [&](const float* p) { return p == bufA ? bufB : bufA; };
    int pend_ln = -1;            // >= 0: `cur` holds block pend_ln's conv + ReLU output, its LayerNorm not yet applied
    for (size_t li = 0; li < P.convs.size(); ++li) {
        const PackedConv& w = P.convs[li];
        int rx = -2;
        float* dst = other(cur);
        // frame-level k = 5 convs (the pitch predictor, round 6): F(4,3) tap groups over frame quads, the pending LayerNorm as the prologue — at
        // EVERY launch size (conv_k5q.hip splits a tile's rows over workgroups when there are few tiles; the bits do not depend on it).  Only the
        // frame-level predictor: the phoneme-level energy predictor (k = 5 too) feeds a bucketize, has 1/6 of the columns and stays in the direct form
        if (frame_level && !mode16 && g_pred_wino && !ln_lens && li < P.convs_q.size() && P.convs_q[li] && w.taps == 5 && w.cout == 256 &&
            (pend_ln < 0 || w.cin == 256)) {
            ConvXlArgs xa;
            memset(&xa, 0, sizeof(xa));
            xa.x = cur; xa.y = dst; xa.wf = P.convs_q[li]; xa.bias = w.bias; xa.bstride = (long)w.cout * ld;
            xa.B = B; xa.C = 256; xa.T = T; xa.ld = ld; xa.k = w.taps; xa.dil = 1; xa.slope = 1.0f; xa.relu = 1;
            if (w.cin != 256) { xa.cin = w.cin; xa.xbstride = (long)w.cin * ldc; }
            if (pend_ln >= 0) { xa.ln_g = P.ln_g[pend_ln]; xa.ln_b = P.ln_b[pend_ln]; xa.ln_eps = 1e-12f; }
            if (ldc == ld || w.cin != 256) {
                rx = cmtts_launch_conv_k5q(&xa, (void*)s);
                if (rx == -3) return fail(CMTTS_E_HIP, "conv_k5q launch failed");
                if (rx == 0) pend_ln = -2;
            }
        }
        // phoneme-level 256 -> 256 convs (round 4): X-resident, one 32-column n-tile per wave, the pending LayerNorm (eps 1e-12, length
        // mask) applied to the staged tile.  (Round 2 tried this with 96-column tiles: 64 workgroups of ~45 us — slower; deleted in round 3.)
        const bool small = (long)((T + 63) / 64) * B < 192;
        if (rx != 0 && !mode16 && g_pred_xres && small && P.convs_f[li] && w.cin == 256 && w.cout == 256 && ldc == ld) {
            ConvArgs a = conv_args(w, cur, T, ldc, (long)w.cin * ldc, dst, ld, (long)w.cout * ld, T);
            a.out[0].act = ACT_RELU;
            a.xres_nt = 1;
            if (pend_ln >= 0) { a.ln_g = P.ln_g[pend_ln]; a.ln_b = P.ln_b[pend_ln]; a.ln_eps = 1e-12f; a.ln_lens = ln_lens; a.ln_skip_tiles = 1; }      // (the next block's LayerNorm / ln_linear masks the same columns)
            rx = cmtts_launch_conv_xres(&a, P.convs_f[li], B, (void*)s);
            if (rx == -3) return fail(CMTTS_E_HIP, "conv_xres launch failed");
            if (rx == 0) pend_ln = -2;       // consumed (if any)
        }
        if (pend_ln >= 0) {                  // the LayerNorm as its own launch
            float* nd = other(cur);
            k_layernorm_ct(cur, nd, P.ln_g[pend_ln], P.ln_b[pend_ln], 1e-12f, ln_lens, B, T, ld, s);
            cur = nd;
            dst = other(cur);
        }
        pend_ln = -1;
        if (mode16 && li < P.convs_f16[mode16 - 1].size() && P.convs_f16[mode16 - 1][li]) {
            ConvArgs a = conv_args(w, cur, T, ldc, (long)w.cin * ldc, dst, ld, (long)w.cout * ld, T);
            a.out[0].act = ACT_RELU;
            a.text_epi = 1;
            rx = cmtts_launch_conv16(&a, P.convs_f16[mode16 - 1][li], mode16, B, (void*)s);
            if (rx == -3) return fail(CMTTS_E_HIP, "text16: predictor conv launch failed");
        }
        if (rx != 0 && g_pred_xl && P.convs_f[li] && ldc == ld && (long)((T + 63) / 64) * B >= 192) {
            // frame-level 256 -> 256 conv: whole x tile + halo resident in LDS, weights streamed as A fragments (the HiFi-GAN
            // kernel, resblock_pair.hip; same accumulation order and epilogue expressions as the generic kernel => same bits)
            ConvXlArgs xa;
            memset(&xa, 0, sizeof(xa));
            xa.x = cur; xa.y = dst; xa.wf = P.convs_f[li]; xa.bias = w.bias; xa.bstride = (long)w.cout * ld;
            xa.B = B; xa.C = 256; xa.T = T; xa.ld = ld; xa.k = w.taps; xa.dil = 1; xa.slope = 1.0f; xa.relu = 1;
            if (w.cin != 256) { xa.cin = w.cin; xa.xbstride = (long)w.cin * ldc; }
            rx = cmtts_launch_conv_xl(&xa, (void*)s);
            if (rx == -3) return fail(CMTTS_E_HIP, "conv_xl launch failed");
        }
        if (rx != 0) {
            ConvArgs a = conv_args(w, cur, T, ldc, (long)w.cin * ldc, dst, ld, (long)w.cout * ld, T);
            a.out[0].act = ACT_RELU;
            CHK(launch(a, EPI_PLAIN, B, s));
        }
        cur = dst;
        ldc = ld;
        if (g_pred_head && eh && g_energy_head && O == 1 && li + 1 == P.convs.size() && w.cout == 256) {
            k_ln_linear_energy(cur, P.ln_g[li], P.ln_b[li], 1e-12f, P.lin_w, P.lin_b, out, ln_lens, out_lens, B, T, ld, eh->xin, eh->e_target, eh->e_control,
                               eh->bins, eh->nbins, eh->E, eh->out1, eh->e_idx, eh->e_scaled, s, eh->e_table);
            eh->done = true;
            return 0;
        }
        if (g_pred_head && li + 1 == P.convs.size() && w.cout == 256 &&
            k_ln_linear(cur, P.ln_g[li], P.ln_b[li], 1e-12f, P.lin_w, P.lin_b, out, ln_lens, out_lens, B, T, ld, O, s))
            return 0;
        pend_ln = (int)li;
    }
    if (pend_ln >= 0) {
        float* nd = other(cur);
        k_layernorm_ct(cur, nd, P.ln_g[pend_ln], P.ln_b[pend_ln], 1e-12f, ln_lens, B, T, ld, s);
        cur = nd;
    }
    k_chan_linear(cur, P.lin_w, P.lin_b, out, out_lens, B, P.convs.back().cout, T, ld, O, s);
    return 0;
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
};

// The part of an evaluation in front of the residual layers: c_in scaling + transpose + input projection (+ clearing of the persistent
// kernel's halo granules) and the step embedding.  *halo_zeroed: the granules of this (B, T) batch have been cleared on `s`.
int denoiser_prologue(cmtts_model* m, const DenWs& w, const float* x_src, float in_scale, const float* timesteps, const float* spk, int B,
                      int T, hipStream_t s, bool embed, float t_host, bool* halo_zeroed) {
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    const long cs = (long)C * T;
    *halo_zeroed = false;
    int rin = -2;
    if (g_inproj_fused && m->in_proj_f) {   // c_in scaling + transpose + input projection (+ halo clearing) in one launch: same bits
        InProjArgs ia;
        memset(&ia, 0, sizeof(ia));
        ia.x = x_src; ia.scale = in_scale; ia.wf = m->in_proj_f; ia.bias = m->in_proj.bias; ia.h = w.h;
        ia.B = B; ia.T = T; ia.M = M; ia.C = C;
        const bool persist_path = g_fused_resblock && g_persist && NL <= PERSIST_MAX_LAYERS;
        if (persist_path) { ia.zero = w.halo; ia.zero_f4 = (long)(cmtts_persist_halo_bytes(B, T) / 16); }
        rin = cmtts_launch_inproj(&ia, (void*)s);
        if (rin == -3) return fail(CMTTS_E_HIP, "inproj launch failed");
        *halo_zeroed = rin == 0 && persist_path && cmtts_persist_halo_bytes(B, T) % 16 == 0;
    }
    if (rin != 0) {
        k_mel_prep(x_src, nullptr, in_scale, w.hin, B, T, M, s);
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
                  const CondFactors* cfk = nullptr, bool* cp_ready = nullptr) {   // cfk: w.cp was NOT filled — the persistent kernel gathers the factors (FACT)
    CHK(check_device_flag(true));
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    const long cs = (long)C * T;
    bool halo_zeroed = false;
    CHK(denoiser_prologue(m, w, x_src, in_scale, timesteps, spk, B, T, s, embed, t_host, &halo_zeroed));
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
    k_mel_post(w.hin, post.xold, post.noise, post.c_out, post.c_skip, post.nstd, post.out, B, T, M, g_tmo_host, s);
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

size_t cmtts_text_workspace_bytes(const cmtts_model* m, int B, int L) { return carve_text(m->cfg, B, L, nullptr).bytes; }
size_t cmtts_frame_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_frame(m->cfg, B, T, nullptr).bytes; }
size_t cmtts_denoiser_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_den(m->cfg, B, T, nullptr).bytes; }

// FFTBlocks.forward's layer loop (model/modules.py:97-99): pre-LN self-attention + Conv1D FFN blocks over channel-major
// x = w.x [B][H][Lp], masked by `lens`.  Shared by the text encoder (L = phonemes) and the FastspeechDecoder (L = frames).
// pad_lens (ragged text batch, else NULL): columns l >= pad_lens[b] do not exist for utterance b.  The one place of an FFT block where that
// matters: LayerNorm2 turns a masked (zero) column into its bias vector, and the k = 9 FFN conv reads up to four such columns beyond
// src_len — inside the padded batch they hold that bias, beyond it the conv's zero padding (model/blocks.py:612-615, 539-546): the
// normalised tile is zeroed from pad_lens[b] on.  (LayerNorm1 feeds k = 1 projections; padded keys are masked, padded queries dropped.)
int fft_stack(cmtts_model* m, const std::vector<EncLayer>& layers, const TextWs& w, const int64_t* src_lens, int B, int L,
              hipStream_t s, const int64_t* pad_lens = nullptr) {
    const cmtts_config& c = m->cfg;
    const int H = c.hidden, Lp = round_up(L, 4), NH = c.enc_heads, dh = H / NH;
    const long hs = (long)H * Lp;
    // X-resident kernel (conv_xres.hip) for the K = 256 contractions: with 96-column tiles (three n-tiles per wave) when they pad no more
    // than 64-column ones and give every CU a workgroup; round 4: with 32-column tiles (one n-tile per wave, a third of the X tile staged
    // per workgroup) for launches that cannot fill the chip anyway — one request, a few utterances: the LayerNorm prologue, the FFN
    // fusion and a K loop without barriers instead of LayerNorm + generic kernel (+ FFN linear); every path has the same bits
    const int t96 = (L + 95) / 96, t64 = (L + 63) / 64;
    const bool cols96 = t96 * 96 <= t64 * 64;
    const bool xres_small = g_ffn_xres && g_xres_small && (long)t96 * B * 8 < 128;        // the FFN conv's 96-column grid leaves CUs idle
    const bool xres_cols = g_ffn_xres && (cols96 || xres_small);
    for (size_t i = 0; i < layers.size(); ++i) {
        const EncLayer& E = layers[i];
        const bool fused_attn = g_attn_fused && dh == 128;      // L <= 192: all keys in registers; longer: key-chunked online softmax (attention.hip)
        // LayerNorm1 as the prologue of the in-projection: one launch, no normalised copy in HBM
        // opt-in ("text16", cmtts_model_set_option; bf16 / fp16 models): the block's four K = 256 / 1024 contractions (in-projection, out-projection, FFN
        // conv, FFN linear) with 16-bit MFMA operands and fp32 accumulate on conv_mfma16.hip; LayerNorm, softmax, bias, scale, GELU, residuals, masks fp32
        const int pm = m->precision;
        const bool t16 = m->text16 && (pm == 1 || pm == 2) && E.ffn1_f16[pm - 1] && E.ffn2_f16[pm - 1] && E.qkv_f16[pm - 1] && E.wo_f16[pm - 1];
        const bool ln_qkv = !t16 && fused_attn && (g_text_xres & 1) && E.qkv_f && xres_cols && ((long)t96 * (3 * H / 128) * B >= 128 || xres_small);
        if (!ln_qkv) k_layernorm_ct(w.x, w.h, E.ln1_g, E.ln1_b, 1e-12f, nullptr, B, L, Lp, s);
        bool attn_done = false;
        if (fused_attn) {
            // q, k, v = h * W_in^T as ONE contraction, then softmax(q k^T / sqrt(dh) + mask) v in one launch per layer:
            // scores and probabilities never leave the CU (attention.hip)
            int rq = -2;
            if (ln_qkv) {
                ConvArgs a = conv_args(E.qkv, w.x, L, Lp, hs, w.qk, Lp, 3 * hs, L);
                a.ln_g = E.ln1_g; a.ln_b = E.ln1_b; a.ln_eps = 1e-12f;
                if (g_text_xres & 8) {   // debugging aid: the projection on the X-resident kernel behind a separate LayerNorm launch
                    k_layernorm_ct(w.x, w.h, E.ln1_g, E.ln1_b, 1e-12f, nullptr, B, L, Lp, s);
                    a.X = w.h; a.ln_g = a.ln_b = nullptr;
                }
                // more workgroups than CUs with 96-column tiles (B = 64, or two column tiles per utterance): the 32-column instance packs two
                // per CU and overlaps their phases — 45-55 us less per text side at 64 x 85 and 32 x 171 phonemes, neutral at 32 x 85 (tools/text_xres_ab2.py)
                a.xres_nt = g_qkv_nt ? g_qkv_nt : ((long)t96 * (3 * H / 128) * B > persist_blocks() ? 1 : 0);
                rq = cmtts_launch_conv_xres(&a, E.qkv_f, B, (void*)s);
                a.xres_nt = 0;
                if (rq == -3) return fail(CMTTS_E_HIP, "conv_xres launch failed");
                if (rq != 0) k_layernorm_ct(w.x, w.h, E.ln1_g, E.ln1_b, 1e-12f, nullptr, B, L, Lp, s);
            }
            if (rq != 0 && t16) {
                ConvArgs a = conv_args(E.qkv, w.h, L, Lp, hs, w.qk, Lp, 3 * hs, L);
                a.text_epi = 1;
                rq = cmtts_launch_conv16(&a, E.qkv_f16[pm - 1], pm, B, (void*)s);
                if (rq == -3) return fail(CMTTS_E_HIP, "text16: in-projection launch failed");
            }
            if (rq != 0) {
                ConvArgs a = conv_args(E.qkv, w.h, L, Lp, hs, w.qk, Lp, 3 * hs, L);
                CHK(launch(a, EPI_PLAIN, B, s));
            }
            AttnArgs at;
            memset(&at, 0, sizeof(at));
            at.qkv = w.qk; at.out = w.o; at.lens = src_lens; at.bstride = 3 * hs; at.obstride = hs;
            at.B = B; at.H = NH; at.dh = dh; at.L = L; at.ld = Lp; at.scale = (float)(1.0 / sqrt((double)dh));
            const int arc = cmtts_launch_attention(&at, (void*)s);
            if (arc == -3) return fail(CMTTS_E_HIP, "attention launch failed");
            attn_done = arc == 0;
        }
        // the V projection is needed only by the PV product: side stream, joined after the softmax
        SideStream* ss = attn_done ? nullptr : side_for(s);
        if (!attn_done) {
        hipStream_t sv = ss ? ss->side : s;
        if (ss) CHK(branch_fork(ss));
        {   // Q,K = h * W[0:2H]^T, channel-major [B][2H][Lp]
            ConvArgs a = conv_args(E.qk, w.h, L, Lp, hs, w.qk, Lp, 2 * hs, L);
            CHK(launch(a, EPI_PLAIN, B, s));
        }
        {   // V^T[b] = h[b]^T * Wv^T : [L][H]   (A operand = activation, X operand = weights)
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.A = w.h; a.a_ld = Lp; a.a_cols = Lp; a.M = L; a.K = H; a.taps = 1; a.dil = 1;
            a.X = E.wvT; a.ldx = H; a.Tin = H; a.N = H;
            a.zdiv = 1; a.a_zs0 = hs; a.x_zs0 = 0;
            a.pre_div = 1.f; a.pre_slope = 1.f; a.split = INT_MAX;
            ConvOut& o = a.out[0];
            o.Y = w.vt; o.y_zs0 = (long)Lp * H; o.ldy = H; o.Tout = H; o.ostride = 1; o.alpha = 1.f; o.div = 1.f;
            CHK(launch(a, EPI_PLAIN, B, sv));
        }
        {   // S^T[b,h][j][i] = sum_d K[d][j] Q[d][i] / sqrt(dh)
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.A = w.qk + hs; a.a_ld = Lp; a.a_cols = Lp; a.M = L; a.K = dh; a.taps = 1; a.dil = 1;
            a.X = w.qk; a.ldx = Lp; a.Tin = L; a.N = L;
            a.zdiv = NH; a.a_zs0 = 2 * hs; a.a_zs1 = (long)dh * Lp; a.x_zs0 = 2 * hs; a.x_zs1 = (long)dh * Lp;
            a.pre_div = 1.f; a.pre_slope = 1.f; a.split = INT_MAX;
            ConvOut& o = a.out[0];
            o.Y = w.st; o.y_zs0 = (long)NH * Lp * Lp; o.y_zs1 = (long)Lp * Lp; o.ldy = Lp; o.Tout = L; o.ostride = 1;
            o.alpha = (float)(1.0 / sqrt((double)dh)); o.div = 1.f;
            CHK(launch(a, EPI_PLAIN, B * NH, s));
        }
        k_softmax_cols(w.st, src_lens, B * NH, NH, L, Lp, (long)Lp * Lp, s);
        if (ss) CHK(branch_join(ss));
        {   // O[b,h][d][i] = sum_j V^T[j][d] P^T[j][i]
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.A = w.vt; a.a_ld = H; a.a_cols = dh; a.M = dh; a.K = L; a.taps = 1; a.dil = 1;
            a.X = w.st; a.ldx = Lp; a.Tin = L; a.N = L;
            a.zdiv = NH; a.a_zs0 = (long)Lp * H; a.a_zs1 = dh; a.x_zs0 = (long)NH * Lp * Lp; a.x_zs1 = (long)Lp * Lp;
            a.pre_div = 1.f; a.pre_slope = 1.f; a.split = INT_MAX;
            ConvOut& o = a.out[0];
            o.Y = w.o; o.y_zs0 = hs; o.y_zs1 = (long)dh * Lp; o.ldy = Lp; o.Tout = L; o.ostride = 1; o.alpha = 1.f; o.div = 1.f;
            CHK(launch(a, EPI_PLAIN, B * NH, s));
        }
        }   // three-launch attention
        {   // x = (x + out_proj(o)) * nonpad      (model/blocks.py:609-610)
            ConvArgs a = conv_args(E.wo, w.o, L, Lp, hs, w.x, Lp, hs, L);
            a.out[0].res = w.x; a.out[0].r_zs0 = hs; a.out[0].ldr = Lp; a.out[0].lens = src_lens;
            int rc = -2;
            if (t16) {
                a.text_epi = 1;
                rc = cmtts_launch_conv16(&a, E.wo_f16[pm - 1], pm, B, (void*)s);
                if (rc == -3) return fail(CMTTS_E_HIP, "text16: out-projection launch failed");
                a.text_epi = 0;
            } else if (E.wo_f && g_ffn_xres && (g_text_xres & 2)) {
                // round 4: M = 256 is two m-blocks — with 96-column tiles 64 workgroups at B = 32 (measured slower than the generic kernel in round 2);
                // with 32-column tiles 192 workgroups of one short chain each, the tile staged once, no barrier in the K loop: 25 -> 13 us per block
                a.xres_nt = 1;
                rc = cmtts_launch_conv_xres(&a, E.wo_f, B, (void*)s);
                a.xres_nt = 0;
            }
            if (rc == -3) return fail(CMTTS_E_HIP, "conv_xres launch failed");
            if (rc != 0) CHK(launch(a, EPI_PLAIN, B, s));
        }
        if (t16) {      // LayerNorm2, FFN conv (+ k^-0.5, GELU), FFN linear (+ residual, mask): three launches instead of two
            k_layernorm_ct(w.x, w.h, E.ln2_g, E.ln2_b, 1e-12f, pad_lens, B, L, Lp, s);
            ConvArgs a = conv_args(E.ffn1, w.h, L, Lp, hs, w.f, Lp, 4 * hs, L);
            a.out[0].alpha = (float)pow((double)c.ffn_kernel, -0.5);
            a.out[0].act = ACT_GELU_ERF;
            a.text_epi = 1;
            int rc = cmtts_launch_conv16(&a, E.ffn1_f16[pm - 1], pm, B, (void*)s);
            if (rc == 0) {
                ConvArgs b = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.x, Lp, hs, L);
                b.out[0].res = w.x; b.out[0].r_zs0 = hs; b.out[0].ldr = Lp; b.out[0].lens = src_lens;
                b.text_epi = 1;
                rc = cmtts_launch_conv16(&b, E.ffn2_f16[pm - 1], pm, B, (void*)s);
                if (rc != 0) return fail(CMTTS_E_HIP, "text16: FFN linear launch failed");
                continue;
            }
            if (rc != -2) return fail(CMTTS_E_HIP, "text16: FFN conv launch failed");
        }
        const bool ffn2_seg = m->ffn2_split && E.ffn2.cin % FFN2_SEG == 0 && E.ffn2.taps == 1;
        bool ffn_fused = false;
        {   // gelu((conv_k9(LayerNorm2(x)) + b) * k^-0.5)      (model/blocks.py:539-546, 612-615)
            // X-resident kernel when it fills the chip; LayerNorm2 is then its prologue
            // round 5: with the F(4,3) form available the X-resident fused launch is taken at EVERY L and B (the Winograd and the direct form differ by fp32
            // rounding: one form for all shapes keeps the text side independent of the batch)
            const float* wqf = g_ffn_wino == 2 ? E.ffn1_q : E.ffn1_p;
            const bool wq = g_ffn_wino && g_ffn_xres && g_ffn_fused && (g_text_xres & 4) && wqf && E.ffn2_f && m->ffn2_split && E.ffn2.cin % FFN2_SEG == 0 &&
                            E.ffn2.taps == 1 && E.ffn1.cout == FFN2_SEG * 128 && H == 256;
            const bool xr = wq || (xres_cols && E.ffn1_f && ((long)t96 * ((E.ffn1.cout + 127) / 128) * B >= 128 || xres_small));
            const bool ln_ffn = xr && (g_text_xres & 4);
            if (!ln_ffn) k_layernorm_ct(w.x, w.h, E.ln2_g, E.ln2_b, 1e-12f, pad_lens, B, L, Lp, s);
            ConvArgs a = conv_args(E.ffn1, ln_ffn ? w.x : w.h, L, Lp, hs, w.f, Lp, 4 * hs, L);
            a.out[0].alpha = (float)pow((double)c.ffn_kernel, -0.5);
            a.out[0].act = ACT_GELU_ERF;
            if (ln_ffn) { a.ln_g = E.ln2_g; a.ln_b = E.ln2_b; a.ln_eps = 1e-12f; a.ln_lens = pad_lens; a.ln_skip_tiles = pad_lens != nullptr; }      // (reduce_partials and the k = 1 linear mask by select)
            int rc = -2;
            if (xr && g_ffn_fused && ffn2_seg && E.ffn2_f && E.ffn1.cout == FFN2_SEG * 128) {
                // ... and the FFN linear's partial products in the same launch: the activated rows never leave the CU
                a.w2frag = E.ffn2_f; a.part = w.part; a.part_zs0 = (long)FFN2_SEG * hs; a.part_zs1 = hs; a.part_ld = Lp; a.M2 = H;
                rc = wq ? cmtts_launch_conv_xresq(&a, wqf, B, (void*)s, g_ffn_wino == 2 ? 1 : 2) : -2;
                if (rc == -2) rc = cmtts_launch_conv_xres(&a, E.ffn1_f, B, (void*)s);
                if (rc == 0) ffn_fused = true;
                else { a.w2frag = nullptr; a.part = nullptr; }
            }
            if (xr && !ffn_fused) rc = cmtts_launch_conv_xres(&a, E.ffn1_f, B, (void*)s);
            if (rc == -3) return fail(CMTTS_E_HIP, "conv_xres launch failed");
            if (rc != 0) {
                if (ln_ffn) {
                    k_layernorm_ct(w.x, w.h, E.ln2_g, E.ln2_b, 1e-12f, pad_lens, B, L, Lp, s);
                    a.X = w.h; a.ln_g = a.ln_b = nullptr; a.ln_lens = nullptr;
                }
                CHK(launch(a, EPI_PLAIN, B, s));
            }
        }
        if (ffn_fused) {   // the partial products are in w.part already
            k_reduce_partials(w.part, FFN2_SEG, E.ffn2.bias, w.x, src_lens, w.x, B, H, L, Lp, s);
        } else if (ffn2_seg) {
            // x = (x + ffn_2(.)) * nonpad          (:551, :616-617) as FFN2_SEG independent partial GEMMs + one reduction
            const int kseg = E.ffn2.cin / FFN2_SEG;
            ConvArgs a = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.part, Lp, (long)FFN2_SEG * hs, L);
            a.K = kseg;
            a.zdiv = FFN2_SEG; a.a_zs0 = 0; a.a_zs1 = (long)kseg * a.a_ld; a.x_zs1 = (long)kseg * Lp;
            a.out[0].y_zs1 = hs; a.out[0].bias = nullptr;
            // (64x64 tiles for the 85-phoneme case — a 128-column tile is one third padding — were tried: 59 vs 44 us)
            CHK(launch(a, EPI_PLAIN, B * FFN2_SEG, s));
            k_reduce_partials(w.part, FFN2_SEG, E.ffn2.bias, w.x, src_lens, w.x, B, H, L, Lp, s);
        } else {   // x = (x + ffn_2(.)) * nonpad          (:551, :616-617)
            ConvArgs a = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.x, Lp, hs, L);
            a.out[0].res = w.x; a.out[0].r_zs0 = hs; a.out[0].ldr = Lp; a.out[0].lens = src_lens;
            CHK(launch(a, EPI_PLAIN, B, s));
        }
    }
    return 0;
}

int cmtts_text_forward(cmtts_model* m, const int64_t* texts, const int64_t* src_lens, const float* spker_embeds,
                       const int64_t* speakers, int B, int L, float d_control, float* log_d, float* d_rounded, int64_t* mel_len,
                       float* e_pred, int64_t* e_idx, float* enc_out_ct, float* speaker_emb,
                       void* text_ws, size_t text_ws_bytes, void* stream) {
    return cmtts_text_forward_ragged(m, texts, src_lens, nullptr, spker_embeds, speakers, B, L, d_control, log_d, d_rounded, mel_len, e_pred,
                                     e_idx, enc_out_ct, speaker_emb, text_ws, text_ws_bytes, stream);
}

// The phoneme-level half for a RAGGED batch: utterances of several padded groups (bucket groups of a shard, BASELINE.json configs[3])
// in one call, padded to the longest group's L.  pad_lens[b] = the padded phoneme count of utterance b's own group: columns
// l >= pad_lens[b] do not exist for it.  Where the padded length enters the reference's arithmetic — LayerNorm2 of every FFT block makes
// a masked column its bias vector, which the k = 9 FFN conv then reads (fft_stack); the speaker vector is added to every column of the
// padded batch (model/modules.py:349-352); the energy predictor runs unmasked over them (:520-554): the columns src_len <= l < L of a
// group feed the convolutions' halos and are returned — the kernels stop at pad_lens[b]; everything else on this path is column-local
// or masked by src_lens.  Every utterance therefore gets the bits of running its group alone
// (tests/test_gpu_parity.py::test_ragged_text_batch_bitwise), and ~60 latency-bound launches serve the whole shard instead of one
// group.  pad_lens == NULL: the uniform batch (= cmtts_text_forward).
int cmtts_text_forward_ragged(cmtts_model* m, const int64_t* texts, const int64_t* src_lens, const int64_t* pad_lens, const float* spker_embeds,
                              const int64_t* speakers, int B, int L, float d_control, float* log_d, float* d_rounded, int64_t* mel_len,
                              float* e_pred, int64_t* e_idx, float* enc_out_ct, float* speaker_emb,
                              void* text_ws, size_t text_ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!texts || !src_lens || !text_ws || B <= 0 || L <= 0) return fail(CMTTS_E_INVALID, "cmtts_text_forward: bad argument");
    const cmtts_config& c = m->cfg;
    if (c.multi_speaker && c.n_speaker > 0 && !speakers) return fail(CMTTS_E_INVALID, "speakers (ids into the speaker_emb table) are required (model/cmtts.py:78)");
    if (c.multi_speaker && c.n_speaker <= 0 && !spker_embeds) return fail(CMTTS_E_INVALID, "Speaker embedding should not be None (model/cmtts.py:80)");
    const cmtts_control_tables& ct = m->ct;
    if ((ct.d || ct.e || ct.p) && ct.ld != L)
        return fail(CMTTS_E_INVALID, "cmtts_text_forward: the control tables' row pitch ld must equal L (cmtts_set_control_tables)");
    if (ct.d && d_control != 1.0f)
        return fail(CMTTS_E_INVALID, "cmtts_text_forward: a duration table replaces d_control, which must then be 1");
    if (ct.e && m->vc.e_control != 1.0f)
        return fail(CMTTS_E_INVALID, "cmtts_text_forward: an energy table replaces e_control, which must then be 1");
    const cmtts_duration_targets& dt = m->dt;
    if (dt.target) {
        if (dt.ld != L)
            return fail(CMTTS_E_INVALID, "cmtts_text_forward: the duration targets' row pitch ld must equal L (cmtts_set_duration_targets)");
        if (m->vc.d_target)
            return fail(CMTTS_E_INVALID, "cmtts_text_forward: duration targets beside a teacher-forced d_target: absolute durations leave nothing to fit");
        if (k_duration_fit_lds_bytes(L) > 64 * 1024)
            return fail(CMTTS_E_INVALID, "cmtts_text_forward: duration targets take L up to 4096");
    }
    TextWs w = carve_text(c, B, L, text_ws);
    if (text_ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "text workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int H = c.hidden, Lp = round_up(L, 4);
    if (!log_d) log_d = w.logd;
    if (!d_rounded) d_rounded = w.dround;
    if (!mel_len) mel_len = w.mlen;
    if (!e_pred) e_pred = w.epred;
    if (!e_idx) e_idx = w.eidx;

    k_embed_tokens(texts, src_lens, m->embed, m->omega_h, m->pe_h, PE_ROWS, w.x, B, L, Lp, H, (float)sqrt((double)H), s);
    CHK(fft_stack(m, m->enc, w, src_lens, B, L, s, pad_lens));
    k_layernorm_ct(w.x, w.x, m->encln_g, m->encln_b, 1e-5f, src_lens, B, L, Lp, s);
    // the encoder output for the caller: a copy of x BEFORE the speaker vector is added; a single-speaker model never modifies x again, so its copy waits until
    // the duration predictor is through (round 6: in the shadow of the longer energy branch instead of in front of both predictors)
    if (enc_out_ct && c.multi_speaker)
        k_copy_rows(enc_out_ct, L, w.x, Lp, L, (long)B * H, s);
    if (c.multi_speaker) {
        if (c.n_speaker > 0) k_gather_rows(m->spk_table, speakers, w.spk, B, H, c.n_speaker, s);
        else k_dense_small(spker_embeds, c.external_speaker_dim, 1, m->spk_wt, m->spk_b, nullptr, w.spk, B,
                      c.external_speaker_dim, H, DENSE_NONE, s);
        k_add_rowvec(w.x, w.spk, B, H, L, Lp, s, pad_lens);
        if (speaker_emb) HIPCHK(hipMemcpyAsync(speaker_emb, w.spk, (size_t)B * H * 4, hipMemcpyDeviceToDevice, s));
    }
    // The duration and the energy predictor both read x and nothing of each other: the energy branch runs on the side
    // stream with its own scratch (the encoder's q/k buffer is free by now)
    SideStream* ss = side_for(s);
    hipStream_t se = ss ? ss->side : s;
    float* ec1 = ss ? w.qk : w.c1;
    float* ec2 = ss ? w.qk + (size_t)B * H * Lp : w.c2;
    if (ss) CHK(branch_fork(ss));
    // duration predictor (masked) -> log_d
    const int t16mode = (m->text16 && (m->precision == 1 || m->precision == 2)) ? m->precision : 0;
    CHK(predictor(m->dur, w.x, Lp, B, L, Lp, src_lens, src_lens, w.c1, w.c2, log_d, 1, s, t16mode));
    // durations -> cumulative frame counts, mel_len: they need log_d only and run here, in the shadow of the (longer) energy branch (round 6; they
    // sat behind the join, the energy embedding and the pitch predictor's input projection)
    if (m->vc.d_target) {   // teacher-forced durations (model/modules.py:365-367)
        HIPCHK(hipMemcpyAsync(d_rounded, m->vc.d_target, (size_t)B * L * 4, hipMemcpyDeviceToDevice, s));
        k_cumsum_durations(m->vc.d_target, w.cum, mel_len, B, L, s);
    } else if (ct.d) {      // per-phoneme duration factors (a target keeps its precedence)
        k_durations_table(log_d, ct.d, d_rounded, w.cum, mel_len, B, L, s);
    } else {
        k_durations(log_d, d_control, d_rounded, w.cum, mel_len, B, L, s);
    }
    // duration targets: the integers of each segment apportioned to its frame count; rewrites d_rounded, cum and mel_len, which is all that
    // anything downstream reads.  Without targets nothing is launched here.
    if (dt.target) k_duration_fit(d_rounded, w.cum, mel_len, src_lens, dt.seg, dt.target, dt.unmet, B, L, dt.n_seg, s);
    // the pitch table is read on the frame side, which may run on another rank: its rows become part of the text-side state
    if (ct.p) HIPCHK(hipMemcpyAsync(w.pctl, ct.p, (size_t)B * L * 4, hipMemcpyDeviceToDevice, s));
    if (enc_out_ct && !c.multi_speaker)
        k_copy_rows(enc_out_ct, L, w.x, Lp, L, (long)B * H, s);
    // energy predictor (unmasked, positions from x[...,0] != 0) -> bucketize -> embedding add
    k_pos_embed_add(w.x, w.h, m->energy.alpha, m->omega_h, m->pe_h, PE_ROWS, B, H, L, Lp, se);
    EnergyHead eh{w.x, m->vc.e_target, m->vc.e_control, m->energy_bins, c.energy_bins - 1, m->energy_emb, w.out1, e_idx, w.escaled, false, ct.e};
    CHK(predictor(m->energy, w.h, Lp, B, L, Lp, pad_lens, pad_lens, ec1, ec2, e_pred, 1, se, t16mode, false, H == 256 ? &eh : nullptr));
    if (ss) CHK(branch_join(ss));
    if (!eh.done)
        k_energy_embed(w.x, e_pred, w.escaled, m->vc.e_target, m->vc.e_control, m->energy_bins, c.energy_bins - 1, m->energy_emb,
                       w.out1, e_idx, B, H, L, Lp, s, ct.e);
    {   // cwt_predictor[0]: Linear(H -> cwt_hidden) (model/modules.py:204-205).  The reference applies it to the length-regulated frames;
        // a k = 1 contraction commutes with the gather (frame t copies phoneme mel2ph[t] - 1, a padding frame is W 0 + b = b), so it runs
        // over the L phonemes here and cmtts_frame_forward gathers its output: the same bits (tests/test_gpu_parity.py goldens,
        // test_cwt_in_phoneme_level_bitwise) for a sixth of the work, off the frame-level chain
        ConvArgs a = conv_args(m->cwt_in, w.out1, L, Lp, (long)H * Lp, w.h128, Lp, (long)c.cwt_hidden * Lp, L);
        int rc = -2;
        if (g_ffn_xres && g_pred_xres && m->cwt_in_f) {      // 128 rows = one m-block: 32-column tiles, no barrier in the K loop (same bits)
            a.xres_nt = 1;
            rc = cmtts_launch_conv_xres(&a, m->cwt_in_f, B, (void*)s);
            if (rc == -3) return fail(CMTTS_E_HIP, "conv_xres launch failed");
            a.xres_nt = 0;
        }
        if (rc != 0) CHK(launch(a, EPI_PLAIN, B, s));
    }
    if (!m->vc.e_target && (ct.e || m->vc.e_control != 1.0f))     // the reference returns prediction * control (:326)
        HIPCHK(hipMemcpyAsync(e_pred, w.escaled, (size_t)B * L * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipGetLastError());
    return 0;
}

int cmtts_frame_forward(cmtts_model* m, const void* text_ws, int B, int L, int T, float* cond_ct, int64_t* mel2ph,
                        float* cwt_out, float* f0_denorm, int64_t* p_idx, float* f0_stats, void* frame_ws,
                        size_t frame_ws_bytes, void* stream) {
    return cmtts_frame_forward_sub(m, text_ws, B, L, 0, B, T, cond_ct, mel2ph, cwt_out, f0_denorm, p_idx, f0_stats, nullptr, frame_ws, frame_ws_bytes, stream);
}

// The frame-level half for the sub-batch [b0, b0 + B) of a text workspace that cmtts_text_forward(_ragged) filled for B_all utterances
// padded to L_all phonemes: a bucket group of a ragged shard takes its own padded frame count T (results are defined per padded
// bucket, model/modules.py:429-430).  Every buffer of the text workspace is batch-major, so the sub-batch is a pointer offset.
// cond_p1 (optional, [B][res_layers * res_channels][L_all rounded up to 4]): the phoneme-level factor of the conditioner projections for
// cmtts_sample_factored / cmtts_sample_group — computed on the branch stream beside the frame-level predictors.
int cmtts_frame_forward_sub(cmtts_model* m, const void* text_ws, int B_all, int L_all, int b0, int B, int T, float* cond_ct, int64_t* mel2ph,
                            float* cwt_out, float* f0_denorm, int64_t* p_idx, float* f0_stats, float* cond_p1, void* frame_ws,
                            size_t frame_ws_bytes, void* stream) {
    return cmtts_frame_forward_sub_t(m, text_ws, B_all, L_all, b0, B, T, cond_ct, mel2ph, cwt_out, f0_denorm, p_idx, f0_stats, cond_p1, nullptr, frame_ws,
                                     frame_ws_bytes, stream);
}

// ... and the factor's channel-contiguous copy cond_p1t [B][res_layers][Lp][res_channels] (round 6): written on the branch stream right behind the
// GEMM that produces cond_p1, under the frame-level convs, instead of at the sampler's entry in front of the first evaluation.
int cmtts_frame_forward_sub_t(cmtts_model* m, const void* text_ws, int B_all, int L_all, int b0, int B, int T, float* cond_ct, int64_t* mel2ph,
                              float* cwt_out, float* f0_denorm, int64_t* p_idx, float* f0_stats, float* cond_p1, float* cond_p1t, void* frame_ws,
                              size_t frame_ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!text_ws || !frame_ws || !cond_ct || !mel2ph || B <= 0 || L_all <= 0 || T <= 0 || b0 < 0 || b0 + B > B_all)
        return fail(CMTTS_E_INVALID, "cmtts_frame_forward: bad argument");
    const cmtts_config& c = m->cfg;
    const int L = L_all;
    TextWs tw = carve_text(c, B_all, L_all, const_cast<void*>(text_ws));
    tw.out1 += (size_t)b0 * c.hidden * round_up(L_all, 4);
    tw.h128 += (size_t)b0 * c.cwt_hidden * round_up(L_all, 4);
    tw.cum += (size_t)b0 * L_all;
    tw.pctl += (size_t)b0 * L_all;
    if (m->ct.p && m->ct.ld != L_all)
        return fail(CMTTS_E_INVALID, "cmtts_frame_forward: the control tables' row pitch ld must equal L_all (cmtts_set_control_tables)");
    if (m->ct.p && m->vc.p_control != 1.0f)
        return fail(CMTTS_E_INVALID, "cmtts_frame_forward: a pitch table replaces p_control, which must then be 1");
    FrameWs w = carve_frame(c, B, T, frame_ws);
    if (frame_ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "frame workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int H = c.hidden, Lp = round_up(L, 4), O = c.use_uv ? 11 : 10, CH = c.cwt_hidden;
    if (!cwt_out) cwt_out = w.cwt;
    if (!f0_denorm) f0_denorm = w.f0;
    if (!p_idx) p_idx = w.pidx;
    if (!f0_stats) f0_stats = w.stats;

    // cwt_stats_layers on the first phoneme of output_1 (model/modules.py:212-215,279) read nothing of the frame-level
    // chain below: side stream, joined before pitch_index
    SideStream* ss = side_for(s);
    hipStream_t sst = ss ? ss->side : s;
    if (ss) CHK(branch_fork(ss));
    // the phoneme-level factor first: it fills the chip for ~40 us while the main stream runs its short, latency-bound launches
    // (mel2ph, length regulator, the 256 -> 128 projection, positions); behind the statistics MLP it ran beside the frame-level
    // k = 5 convs instead and both took twice as long (profiles/r04_text_side.md)
    // (a model without the pitch-table factor — odd res_layers at C = 256, hidden != 256, a failed finalize-time GEMM — leaves cond_p1 untouched:
    // CondFactors::usable() is false for it and the sampler takes the dense GEMM, as it did before the factors existed)
    if (cond_p1t && !cond_p1) return fail(CMTTS_E_INVALID, "cmtts_frame_forward_sub_t: cond_p1t needs cond_p1");
    if (cond_p1 && m->cond_p2) {
        CHK(cond_phoneme_factor(m, tw.out1, B, Lp, cond_p1, sst));
        if (cond_p1t) k_transpose(cond_p1, cond_p1t, B * c.res_layers, c.res_channels, Lp, sst);      // [B NL][C][Lp] -> [B NL][Lp][C]
    }
    if (!(g_stats_mlp && k_stats_mlp(tw.out1, (long)H * Lp, Lp, m->st0_wt, m->st0_b, m->st2_wt, m->st2_b, m->st4_wt, m->st4_b, f0_stats, B, H, CH, CH, 2, sst))) {
        k_dense_small(tw.out1, (long)H * Lp, Lp, m->st0_wt, m->st0_b, nullptr, w.s1, B, H, CH, DENSE_RELU, sst);
        k_dense_small(w.s1, CH, 1, m->st2_wt, m->st2_b, nullptr, w.s2, B, CH, CH, DENSE_RELU, sst);
        k_dense_small(w.s2, CH, 1, m->st4_wt, m->st4_b, nullptr, f0_stats, B, CH, 2, DENSE_NONE, sst);
    }
    k_mel2ph(tw.cum, mel2ph, B, L, T, s);
    // with the pitch predictor's input projection applied before the gather the length-regulated [B][H][T] tensor has ONE reader left, the pitch
    // embedding add at the end: that kernel gathers from out1 itself (k_lr_gather_add: the same values, one launch and 2 x 17 MB less)
    if (!g_cwt_in_phoneme) k_length_regulate(tw.out1, mel2ph, w.xlr, B, H, Lp, T, s);
    bool hp_done = false;
    if (g_cwt_in_phoneme) {   // cwt_predictor[0] was applied at the phoneme level (cmtts_text_forward): gather it; padding frames = its bias —
        // inside the position-embedding add that follows (one launch, no [B][128][T] intermediate)
        k_pos_embed_add_lr(tw.h128, Lp, mel2ph, m->cwt_in.bias, w.hp, m->cwt.alpha, m->omega_cwt, m->pe_cwt, PE_ROWS, B, CH, T, s);
        hp_done = true;
    } else {   // cwt_predictor[0]: Linear(H -> cwt_hidden) over the frames       (model/modules.py:204-205)
        ConvArgs a = conv_args(m->cwt_in, w.xlr, T, T, (long)H * T, w.h128, T, (long)CH * T, T);
        CHK(launch(a, EPI_PLAIN, B, s));
    }
    if (!hp_done) k_pos_embed_add(w.h128, w.hp, m->cwt.alpha, m->omega_cwt, m->pe_cwt, PE_ROWS, B, CH, T, T, s);
    CHK(predictor(m->cwt, w.hp, T, B, T, T, nullptr, nullptr, w.c1, w.c2, cwt_out, O, s, (m->text16 && (m->precision == 1 || m->precision == 2)) ? m->precision : 0, true));
    if (ss) CHK(branch_join(ss));
    if (m->ct.p) k_pitch_table_scale(cwt_out, mel2ph, tw.cum, tw.pctl, B, O, L, T, s);      // :270 per phoneme: the rows the text side (or cmtts_text_state_unpack) left in the workspace
    else if (m->vc.p_control != 1.0f) k_scale(cwt_out, cwt_out, (long)B * T * O, m->vc.p_control, s);   // :270
    if (m->vc.cwt_spec) {   // teacher-forced pitch: target spectrogram, statistics and uv (:379-390)
        k_pitch_index(m->vc.cwt_spec, 10, m->vc.f0_mean, m->vc.f0_std, 1, 1.0f, nullptr, 0, c.use_uv ? m->vc.uv : nullptr,
                      c.pitch_norm_eps, w.r, p_idx, f0_denorm, B, T, s);
    } else {
        k_pitch_index(cwt_out, O, f0_stats, f0_stats + 1, 2, c.cwt_std_scale, c.use_uv ? cwt_out + (O - 1) : nullptr, O, nullptr,
                      c.pitch_norm_eps, w.r, p_idx, f0_denorm, B, T, s);
    }
    if (g_cwt_in_phoneme) k_lr_gather_add(tw.out1, mel2ph, Lp, p_idx, m->pitch_emb, cond_ct, B, H, T, s);
    else k_gather_add(w.xlr, p_idx, m->pitch_emb, cond_ct, B, H, T, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- per-utterance text-side state records (text_state.hip): the regions of a text workspace that cmtts_frame_forward_sub reads —
// out1 [H][Lp], h128 [cwt_hidden][Lp], spk [H] (fp32), cum [L] (int32), and with a pitch control table installed its rows pctl [L] (fp32) —
// behind a 64-byte header, each region 16-byte aligned.
namespace {
struct TextStateLayout {
    long off[TEXT_STATE_MAX_REGIONS], bytes[TEXT_STATE_MAX_REGIONS], stride[TEXT_STATE_MAX_REGIONS];
    long rec_bytes;
    int n_regions;
};
// with_p: a pitch control table is installed (cmtts_set_control_tables) — the record gains its row as a fifth region and names layout
// revision 2; without one a record is byte for byte the revision-1 record
TextStateLayout text_state_layout(const cmtts_config& c, int L, bool with_p) {
    const int Lp = round_up(L, 4);
    TextStateLayout t;
    t.bytes[0] = (long)c.hidden * Lp * 4;       // out1
    t.bytes[1] = (long)c.cwt_hidden * Lp * 4;   // h128
    t.bytes[2] = (long)c.hidden * 4;            // spk
    t.bytes[3] = (long)L * 4;                   // cum
    t.bytes[4] = (long)L * 4;                   // pctl: the pitch control table's row (layout revision 2 only)
    t.n_regions = with_p ? 5 : 4;
    long off = TEXT_STATE_HEADER_BYTES;
    for (int g = 0; g < t.n_regions; ++g) {
        t.stride[g] = t.bytes[g];               // per-utterance stride in the workspace: the regions are [B][...] slabs
        t.off[g] = off;
        off += (t.bytes[g] + 15) / 16 * 16;
    }
    t.rec_bytes = off;
    return t;
}
TextStateCopy text_state_args(const cmtts_config& c, void* ws, int B_all, int L, void* records, int n, int unpack, bool with_p) {
    const TextStateLayout t = text_state_layout(c, L, with_p);
    TextWs tw = carve_text(c, B_all, L, ws);
    char* base[TEXT_STATE_MAX_REGIONS] = {(char*)tw.out1, (char*)tw.h128, (char*)tw.spk, (char*)tw.cum, (char*)tw.pctl};
    TextStateCopy a;
    memset(&a, 0, sizeof(a));
    int chunks = 0;
    for (int g = 0; g < t.n_regions; ++g) {
        TextStateRegion& R = a.reg[g];
        R.ws = base[g]; R.ws_stride = t.stride[g]; R.rec_off = t.off[g]; R.bytes = t.bytes[g];
        R.vec16 = ((uintptr_t)R.ws % 16 == 0 && R.ws_stride % 16 == 0 && R.bytes % 16 == 0 && (uintptr_t)records % 16 == 0) ? 1 : 0;
        R.chunk0 = chunks;
        chunks += (int)((R.bytes + TEXT_STATE_CHUNK - 1) / TEXT_STATE_CHUNK);
    }
    a.n_regions = t.n_regions; a.n_chunks = chunks; a.unpack = unpack;
    a.layout = with_p ? TEXT_STATE_LAYOUT_P : TEXT_STATE_LAYOUT;
    a.n = n; a.B_all = B_all; a.L_all = L; a.hidden = c.hidden; a.cwt_hidden = c.cwt_hidden;
    a.rec = (char*)records; a.rec_bytes = t.rec_bytes;
    a.cum = tw.cum;
    return a;
}
}  // namespace

size_t cmtts_text_state_record_bytes(const cmtts_model* m, int L_all) {
    if (!m || L_all <= 0) return 0;
    return (size_t)text_state_layout(m->cfg, L_all, m->ct.p != nullptr).rec_bytes;
}

int cmtts_text_state_pack(cmtts_model* m, const void* text_ws, int B_all, int L_all, const int32_t* rows, int n, const int64_t* global_idx,
                          const int64_t* src_lens, void* records, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!text_ws || !records || (n > 0 && !rows) || B_all <= 0 || L_all <= 0 || n < 0)
        return fail(CMTTS_E_INVALID, "cmtts_text_state_pack: bad argument");
    if ((uintptr_t)records % 16) return fail(CMTTS_E_INVALID, "cmtts_text_state_pack: records must be 16-byte aligned");
    if (m->ct.p && m->ct.ld != L_all)
        return fail(CMTTS_E_INVALID, "cmtts_text_state_pack: the control tables' row pitch ld must equal L_all (cmtts_set_control_tables)");
    TextStateCopy a = text_state_args(m->cfg, const_cast<void*>(text_ws), B_all, L_all, records, n, 0, m->ct.p != nullptr);
    a.rows = rows; a.index = global_idx; a.src_lens = src_lens;
    if (cmtts_launch_text_state_copy(&a, stream) != 0) return fail(CMTTS_E_HIP, "text-state pack launch failed");
    return 0;
}

int cmtts_text_state_unpack(cmtts_model* m, const void* records, int n, int L_all, void* text_ws, size_t text_ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!text_ws || !records || n <= 0 || L_all <= 0) return fail(CMTTS_E_INVALID, "cmtts_text_state_unpack: bad argument");
    if ((uintptr_t)records % 16) return fail(CMTTS_E_INVALID, "cmtts_text_state_unpack: records must be 16-byte aligned");
    if (text_ws_bytes < carve_text(m->cfg, n, L_all, nullptr).bytes) return fail(CMTTS_E_WORKSPACE, "text workspace too small");
    if (m->ct.p && m->ct.ld != L_all)
        return fail(CMTTS_E_INVALID, "cmtts_text_state_unpack: the control tables' row pitch ld must equal L_all (cmtts_set_control_tables)");
    TextStateCopy a = text_state_args(m->cfg, text_ws, n, L_all, const_cast<void*>(records), n, 1, m->ct.p != nullptr);
    if (cmtts_launch_text_state_copy(&a, stream) != 0) return fail(CMTTS_E_HIP, "text-state unpack launch failed");
    return 0;
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
// The sampler on one padded (B, T) batch whose workspace is already carved.  noise_stride = elements between consecutive noise tensors
// (B * T * n_mels for a whole batch; a sub-batch [b0, b0 + B) of a larger batch keeps the larger batch's stride).
// seeds (cmtts_sample_seeded): device int64 [B] — x_T is generated straight into w.xcur (noise_philox.hip, draw 0 scaled by sigma_max:
// the bits of a draw-0 tensor through k_scale) and `noise` is a buffer of n_steps tensors that takes the re-noise draws 1.. in one
// launch on the side stream, beside the conditioner branch.
int sample_core(cmtts_model* m, const DenWs& w, const float* noise, long noise_stride, const float* cond_ct, const float* speaker_emb, int B,
                int T, int n_steps, const float* sigmas, const float* renoise_std, float* mel, hipStream_t s, const CondFactors* cf = nullptr,
                const int64_t* seeds = nullptr) {
    const cmtts_config& c = m->cfg;
    const long nel = (long)B * T * c.n_mels;
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
        for (int i = 0; i < n_steps; ++i)
            if (renoise_std[i] >= 0.0f) n_re = i + 1;
        if (cmtts_launch_noise_fill(seeds, B, T, c.n_mels, 0, 1, 0, c.sigma_max, w.xcur, nullptr, (void*)s) != 0 ||
            (n_re && cmtts_launch_noise_fill(seeds, B, T, c.n_mels, 1, n_re, 0, 1.0f, const_cast<float*>(noise), nullptr, (void*)(ss ? ss->side : s)) != 0))
            return fail(CMTTS_E_HIP, "seeded noise launch failed");
    } else
        k_scale(noise, w.xcur, nel, c.sigma_max, s);        // x_T = randn * sigma_max (karras_diffusion.py:534)
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
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
        {"qkv_nt", &g_qkv_nt, 0, 3},
        {"cwt_in_phoneme", &g_cwt_in_phoneme, 0, 1},   // Linear(256 -> 128) of the pitch predictor before (1) or after (0) the length regulator
        {"pred_xres", &g_pred_xres, 0, 1},         // phoneme-level predictor convs on conv_xres with the LayerNorm prologue
        {"xres_small", &g_xres_small, 0, 1},       // FFT blocks of small batches on conv_xres with 32-column tiles
        {"cond_inkernel", &g_cond_inkernel, 0, 1}, // fp32 persistent denoiser gathers the conditioner factors itself (same bits as expanding them into cp first)
        {"cond_factored", &g_cond_factored, 0, 1}, // fp32 models: conditioner projections expanded from their phoneme-level / pitch-table factors when the caller hands them over (NOT bitwise the dense GEMM: W a + W b against W (a + b))
        {"cond_gemm16", &g_cond_gemm16, 0, 1},     // 16-bit models: conditioner GEMM with 16-bit operands (NOT bitwise: another operand precision)
        {"cond_gemm", &g_cond_gemm, 0, 2},         // stacked conditioner GEMM on cond_gemm.hip: 0 never, 1 when it pays, 2 whenever supported
        {"persist_tail", &g_persist_tail, 0, 1},   // skip head + post-scaling inside the persistent launch
        {"persist_wino", &g_persist_wino, 0, 3},   // fp32 persistent denoiser's k = 3 conv: 0 direct, 1 (and 2) Winograd F(2,3), 3 F(4,3) (NOT bitwise the direct form)
        {"inproj_fused", &g_inproj_fused, 0, 1},   // denoiser input as one launch
        {"ffn_xres", &g_ffn_xres, 0, 1},           // k = 9 FFN conv on conv_xres.hip
        {"ffn_wino", &g_ffn_wino, 0, 2},           // FFN conv as Winograd tap groups in the fused launch (fp32; NOT bitwise the direct form): 1 = F(2,3) pairs (default), 2 = F(4,3) quads
        {"ffn_fused", &g_ffn_fused, 0, 1},         // FFN linear's partial products inside the FFN conv's launch
        {"text_xres", &g_text_xres, 0, 15},        // bit mask: 1 LN1 + in-projection, 2 out-projection, 4 LN2 + FFN conv on conv_xres.hip
        {"attn_fused", &g_attn_fused, 0, 1},       // fused attention kernel vs three launches
        {"pred_xl", &g_pred_xl, 0, 1},             // frame-level predictor convs on conv_xl
        {"pred_head", &g_pred_head, 0, 1},         // LayerNorm + linear head in one launch
        {"pred_wino", &g_pred_wino, 0, 1},         // pitch predictor's k = 5 convs as F(4,3) tap groups (NOT bitwise the direct form)
        {"energy_head", &g_energy_head, 0, 1},     // energy bucketize + embedding add inside the energy predictor's head launch (same bits)
        {"stats_mlp", &g_stats_mlp, 0, 1},         // cwt_stats_layers as one launch (same bits)
        {"text_xt16", &g_conv_xt16, 0, 1},         // text16 convs with K = 256 on the X-resident 16-bit kernel (conv_xt16.hip) instead of the chunked one
    };
    if (!strcmp(name, "attn_qb")) return cmtts_attention_set_qb(value);       // attention.hip: queries split over workgroups (round 6; same bits)
    if (!strcmp(name, "xres_nt")) return cmtts_xres_set_nt(value);            // conv_xres tile width for launches that do not choose one (measurements)      // conv_xl: m-tiles over several workgroups for launches of a few column tiles
    bool found;
    int prev = vocoder_internal_set(name, value, &found);      // vocoder.hip: voc_*, post_v4
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

size_t cmtts_decoder_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_text(m->cfg, B, T, nullptr).bytes; }

// FastspeechDecoder.forward (model/modules.py:154-165 -> FFTBlocks.forward :80-105 with use_pos_embed=True):
// x + alpha * PE[positions(x[..., 0] != 0)], masked, 4 FFT blocks, final LayerNorm (eps 1e-5), masked.
int cmtts_decoder_forward(cmtts_model* m, const float* x_ct, const int64_t* lens, int B, int T, float* out_ct, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (m->dec.empty()) return fail(CMTTS_E_INVALID, "cmtts_decoder_forward: the state dict held no decoder.* tensors");
    if (!x_ct || !lens || !out_ct || !ws || B <= 0 || T <= 0) return fail(CMTTS_E_INVALID, "cmtts_decoder_forward: bad argument");
    if (T + 1 >= PE_ROWS) return fail(CMTTS_E_UNSUPPORTED, "cmtts_decoder_forward: T exceeds the position table");
    const cmtts_config& c = m->cfg;
    TextWs w = carve_text(c, B, T, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "decoder workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int H = c.hidden, Tp = round_up(T, 4);
    k_copy_rows(w.f, Tp, x_ct, T, T, (long)B * H, s);
    k_pos_embed_add(w.f, w.x, m->dec_alpha, m->omega_h, m->pe_h, PE_ROWS, B, H, T, Tp, s, lens);
    CHK(fft_stack(m, m->dec, w, lens, B, T, s));
    k_layernorm_ct(w.x, w.x, m->decln_g, m->decln_b, 1e-5f, lens, B, T, Tp, s);
    k_copy_rows(out_ct, T, w.x, Tp, T, (long)B * H, s);
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
