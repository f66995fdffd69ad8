// The denoiser and sampler's host side: the denoiser / sampler / retake / ragged-shard entry points of the C ABI (include/cmtts_hip.h), their
// workspaces, switches and profiling events, and the launch sequences they share — one network evaluation (denoiser_core: Denoiser.forward as
// prologue, join, residual layers in the first form that takes the shape, skip head, post-scaling), the conditioner branch beside it, and the
// sampler's step loops (sample_setup, then uniform_steps or mixed_steps).  Weight import: import.hip; handle: model.h; what this unit shares
// with cmtts_api.hip and text_side.hip: launch.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
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
#include "inproj.h"
#include "stream_windows.h"
#include "noise_philox.h"
#include "retake.h"

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

// The public options "step_cache" and "resblock_split": cmtts_set_option (cmtts_api.hip) keeps their rows of its table, launch.h declares them
int g_step_cache = 1;           // cmtts_sample: reuse the timestep-only part of the step embedding across calls (same bits); 0 = recompute every call
int g_split_resblock = 1;       // fp32 residual block as two launches over 4x the CUs (resblock_split.hip): 0 never, 1 small batches, 2 always

namespace {

// Optional HIP-event instrumentation of the dominant kernel (the gated k=3 conv of the denoiser
// residual block), recorded on the launch stream: bench.py's live roofline figure.
struct Profile {
    bool on = false;
    std::vector<hipEvent_t> ev;   // start/stop pairs
    size_t used = 0;
    int stride = 1;               // every stride-th launch is bracketed (event records cost launch-queue time)
    long seen = 0;
    bool room() const { return on && used + 2 <= ev.size(); }
    bool layer_due() { return room() && (seen++ % stride) == 0; }      // the per-layer sites: every stride-th layer that still finds a pair
} g_prof;
// The event pair around ONE launch on `s`: the start is recorded here, the stop by launched() once the launcher has taken the launch (a launcher
// that declines leaves the pair to the next launch).
struct Bracket {
    hipStream_t s;
    bool on;
    Bracket(bool due, hipStream_t s) : s(s), on(due) {
        if (on) (void)hipEventRecord(g_prof.ev[g_prof.used], s);
    }
    void launched() {
        if (!on) return;
        (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s);
        g_prof.used += 2;
    }
};

bool g_fused_resblock = true;
int g_persist_tail = 1;      // skip head + post-scaling inside the persistent denoiser launch (false: separate launches)
int g_inproj_fused = 1;         // denoiser input: c_in scaling + transpose + input projection + halo clearing in one launch (same bits); 0 = three launches
int g_persist_wino = 3;         // fp32 persistent denoiser: the k = 3 conv in a Winograd form (NOT bitwise the direct form): 3 = F(4,3), the 8-wave WINO == 2 instances
                                // of denoiser_persist.hip (default since round 5: half of the conv's MFMAs), 1 = F(2,3), the 8-wave WINO == 1 instances (2/3), 0 = direct
                                // (2 was round 5's one-wave-per-SIMD F(2,3) stack — same bits as 1, measured 4-10 % slower, out of the build since round 6: tools/attic/ — and runs as 1)
int g_cond_gemm16 = 1;          // bf16 / fp16 / fp16x3 models: conditioner GEMM with 16-bit operands (cond_gemm16.hip); 0 = fp32 operands as until round 3 (different numerics)
int g_cond_gemm = 1;            // stacked conditioner GEMM through cond_gemm.hip: 0 never (generic kernel), 1 when it pays, 2 whenever supported
int g_persist = 1;              // residual layers in one persistent launch (denoiser_persist.hip): 0 never, 1 when it pays, 2 whenever supported
                                // (written by cmtts_set_persistent_denoiser only; read through persist_mode)
// The persistent-stack mode of one call: a caller that keeps its batch off the stack (the ragged shard's set-aside groups) passes allow = false.
// The halo clearing of the prologue, the in-kernel-factor decision of the sampler and the layer forms of denoiser_core all ask here.
inline int persist_mode(bool allow) { return allow ? g_persist : 0; }
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
// The factors as an entry point receives them.  who: the entry point, whose call fails on incomplete factors; null (a group of a ragged shard,
// where incomplete factors mean the dense GEMM): no check.  No p1, no factors: p1t is ignored.
int factors_from(const char* who, const float* p1, const float* p1t, int ldp, int L, const int64_t* mel2ph, const int64_t* p_idx, CondFactors* f) {
    if (who && p1 && (!mel2ph || !p_idx || L <= 0 || ldp < L)) return fail(CMTTS_E_INVALID, std::string(who) + ": incomplete factors");
    f->p1 = p1; f->p1t = p1 ? p1t : nullptr; f->ldp = ldp; f->L = L; f->mel2ph = mel2ph; f->p_idx = p_idx;
    return 0;
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

// get_scalings_for_boundary_condition in fp32 (karras_diffusion.py:87-102) and the rescaled timestep the network is given.  The one place these
// are computed: the uniform loops, the mixed sampler's table and the ragged shard agree bit for bit because they all call it.
struct EvalScalings { float c_in, c_out, c_skip, t_resc; };
EvalScalings scalings(const cmtts_config& c, float sigma) {
    const float smin = c.sigma_min, sd2 = c.sigma_data * c.sigma_data;
    const float dm = sigma - smin;
    const float c_skip = sd2 / (dm * dm + sd2);
    const float rt = sqrtf(sigma * sigma + sd2);
    const float c_out = dm * c.sigma_data / rt;
    const float c_in = 1.0f / rt;
    const float t_resc = 250.0f * logf(sigma + 1e-44f);
    return {c_in, c_out, c_skip, t_resc};
}

// What one network evaluation is given besides its batch and its post-scaling
struct Eval {
    const float* x_src = nullptr;        // [B][T][80], read scaled by in_scale ...
    float in_scale = 1.0f;
    const float* in_scale_b = nullptr;   // ... or, device [B], by c_in per utterance (cmtts_sample_mixed)
    const float* timesteps = nullptr;    // device [B]
    bool embed = true;                   // false: the workspace already holds the step embedding of these timesteps
    float t_host = NAN;                  // the timestep every row of `timesteps` holds, when the caller knows it (step cache); NaN otherwise
    SideStream* pending = nullptr;       // a side branch (the conditioner GEMM, the first step embedding) to join before the layers
    const CondFactors* cfk = nullptr;    // w.cp was NOT filled: the persistent kernel gathers the factors (FACT) ...
    bool* cp_ready = nullptr;            // ... unless an earlier evaluation of the call had to expand them into w.cp after all
    bool allow_persist = true;           // persist_mode
    bool gathers() const { return cfk && !(cp_ready && *cp_ready); }
};

// What a form's launcher answered: 0 = it has taken the stage; -3 = the HIP launch failed, which fails the call with `what`; anything else
// (-2: the launcher does not cover the shape) = declined, nothing was launched and the caller goes on to its next form.
int taken(int rc, const char* what, bool* took) {
    *took = rc == 0;
    return rc == -3 ? fail(CMTTS_E_HIP, what) : 0;
}

// The part of an evaluation in front of the residual layers: c_in scaling + transpose + input projection (+ clearing of the persistent
// kernel's halo granules) and the step embedding.  *halo_zeroed: the granules of this (B, T) batch have been cleared on `s`.
int denoiser_prologue(cmtts_model* m, const DenWs& w, const Eval& ev, const float* spk, int B, int T, hipStream_t s, bool* halo_zeroed) {
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, M = c.n_mels;
    *halo_zeroed = false;
    bool took = false;
    if (g_inproj_fused && m->in_proj_f) {   // c_in scaling + transpose + input projection (+ halo clearing) in one launch: same bits
        InProjArgs ia;
        memset(&ia, 0, sizeof(ia));
        ia.x = ev.x_src; ia.scale = ev.in_scale; ia.scale_b = ev.in_scale_b; ia.wf = m->in_proj_f; ia.bias = m->in_proj.bias; ia.h = w.h;
        ia.B = B; ia.T = T; ia.M = M; ia.C = C;
        const bool persist_path = g_fused_resblock && persist_mode(ev.allow_persist) && NL <= PERSIST_MAX_LAYERS;
        if (persist_path) { ia.zero = w.halo; ia.zero_f4 = (long)(cmtts_persist_halo_bytes(B, T) / 16); }
        CHK(taken(cmtts_launch_inproj(&ia, (void*)s), "inproj launch failed", &took));
        *halo_zeroed = took && persist_path && cmtts_persist_halo_bytes(B, T) % 16 == 0;
    }
    if (!took) {
        k_mel_prep(ev.x_src, ev.in_scale_b, ev.in_scale, w.hin, B, T, M, s);
        ConvArgs a = conv_args(m->in_proj, w.hin, T, T, (long)M * T, w.h, T, (long)C * T, T);
        a.out[0].act = ACT_RELU;   // relu(relu(.)) == relu(.), model/modules.py:575-577,624
        CHK(launch(a, EPI_PLAIN, B, s));
    }
    if (ev.embed) CHK(step_embedding(m, w, ev.timesteps, spk, B, s, ev.t_host));
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

// The model-dependent part of a persistent launch's arguments: the layers' weights in the model's precision, the in-kernel tail's weights
// (the skip head + post-scaling run inside the launch: pa.tail) and the form of the fp32 k = 3 conv.  wino_state_present: every workspace of
// the launch carries the Winograd instances' private state.
void persist_model_args(PersistArgs& pa, const cmtts_model* m, bool wino_state_present) {
    const int NL = m->cfg.res_layers, prec = m->precision;
    if (g_persist_tail && m->skip_f && m->outp_f) {
        pa.tail = 1;
        pa.Wsf = m->skip_f; pa.bs = m->skip_proj.bias; pa.Wpf = m->outp_f; pa.bp = m->out_proj.bias;
        pa.skip_div = (float)sqrt((double)NL); pa.n_mels = m->cfg.n_mels;
    }
    pa.wino = g_persist_wino && m->winograd && !prec && m->res[0].w3w && wino_state_present;
    if (pa.wino && g_persist_wino == 3 && m->winograd == 1 && m->res[0].w3w43) pa.wino = 3;     // F(4,3) (model option "winograd" = 2 keeps F(2,3))
    for (int l = 0; l < NL; ++l) {
        const ResLayer& R = m->res[l];
        pa.W3f[l] = prec ? (const float*)R.w3f16[prec - 1] : (pa.wino == 3 ? R.w3w43 : pa.wino ? R.w3w : R.w3f);
        pa.Wof[l] = prec ? (const float*)R.wof16[prec - 1] : R.wof;
        pa.b3[l] = R.b3f; pa.bo[l] = R.outp.bias;
    }
}

// The residual layers of one evaluation (Denoiser.forward's layer loop, model/modules.py:626-633): what every form of a layer reads, and the
// ping-pong pair — x is in hcur, halt is free
struct Layers {
    cmtts_model* m;
    const DenWs& w;
    const float* cond_ct;
    const float* dp;          // the step (+ speaker) projections the layers add: [B][NL * C]
    int B, T;
    hipStream_t s;
    float *hcur, *halt;
    void swap() { std::swap(hcur, halt); }
};

// All layers as ONE persistent launch per utterance chunk (denoiser_persist.hip), with the skip head and the post-scaling inside it when the
// tail is on.  A launcher that declines the shape leaves both flags false and nothing launched.
int persistent_stack(const Layers& L, const Eval& ev, const MelPost& post, bool halo_zeroed, int mode, bool* layers_done, bool* tail_done) {
    const cmtts_model* m = L.m;
    const DenWs& w = L.w;
    const cmtts_config& c = m->cfg;
    const int C = c.res_channels, NL = c.res_layers, B = L.B, T = L.T;
    PersistArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.x0 = w.h; pa.cp = w.cp; pa.cp_bstride = (long)NL * C * T;
    pa.dp = L.dp; pa.d = w.dproj; pa.vec_stride = (long)NL * C;
    pa.skip = w.skip; pa.halo = w.halo; pa.tmo = g_tmo_host;
    pa.B = B; pa.T = T; pa.NL = NL;
    pa.halo_zeroed = halo_zeroed;
    if (ev.gathers()) {
        const CondFactors& f = *ev.cfk;
        pa.fact = 1; pa.p1 = f.p1; pa.p2 = m->cond_p2; pa.mel2ph = (const long long*)f.mel2ph; pa.pidx = (const long long*)f.p_idx;
        pa.ldp = f.ldp; pa.Lph = f.L; pa.ld2 = c.pitch_bins;
        pa.p1t = f.p1t; pa.p2t = m->cond_p2t;
    }
    persist_model_args(pa, m, w.pst != nullptr);
    if (pa.tail) {
        pa.xold = post.xold; pa.noise = post.noise; pa.c_out = post.c_out; pa.c_skip = post.c_skip; pa.nstd = post.nstd;
        pa.out = post.out;
        pa.post_rows = post.rows; pa.out_final = post.out_final;
    }
    pa.xst = w.pst;
    const int prec = m->precision, cap = persist_blocks();
    const bool due = g_prof.room();
    // fp16x3 exists as the persistent stack only: shapes that do not take it run the exact fp32 kernels
    const int need = cmtts_persist_plan(B, T, NL, cap, mode == 2);
    if (need) CHK(persist_admit(L.s, need, cap));
    Bracket prof(due, L.s);
    bool took;
    CHK(taken(prec ? cmtts_launch_denoiser_persist_lp(&pa, prec, cap, mode == 2, (void*)L.s) : cmtts_launch_denoiser_persist(&pa, cap, mode == 2, (void*)L.s),
              "persistent denoiser launch failed", &took));
    if (!took) return 0;
    CHK(persist_launched(L.s, need));
    prof.launched();
    *layers_done = true;
    *tail_done = pa.tail != 0;
    return 0;
}

// What the per-layer kernels of resblock_args.h are given by every route that reaches them
ResArgs res_args(const Layers& L, int l) {
    const cmtts_config& c = L.m->cfg;
    const int C = c.res_channels, NL = c.res_layers;
    const ResLayer& R = L.m->res[l];
    ResArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.x_in = L.hcur; ra.x_out = L.halt; ra.skip = L.w.skip;
    ra.dp = L.dp + (long)l * C; ra.d = L.w.dproj + (long)l * C;
    ra.W3f = R.w3f; ra.b3 = R.b3f; ra.Wof = R.wof; ra.bo = R.outp.bias;
    ra.vec_stride = (long)NL * C; ra.B = L.B; ra.T = L.T; ra.accum_skip = l > 0;
    return ra;
}

// ResidualBlock.forward (model/blocks.py:667-686) as one kernel (two for few tiles) on the stacked conditioner projections w.cp; x ping-pongs.
// w43 ("batch_invariant"): the persistent stack's F(4,3) form.
int fused_layer(Layers& L, int l, bool w43, bool prof_due) {
    const cmtts_model* m = L.m;
    const int C = m->cfg.res_channels, NL = m->cfg.res_layers, T = L.T;
    ResArgs ra = res_args(L, l);
    ra.cp = L.w.cp + (long)l * C * T; ra.cp_bstride = (long)NL * C * T; ra.flag = g_tmo_host;
    Bracket prof(prof_due, L.s);
    int rc;
    if (m->precision == 0 || m->precision == 3) {
        // few 32-frame tiles: one workgroup per tile leaves most of the chip idle for 83 us per layer; four
        // workgroups per tile in two launches finish sooner (measured crossover, tools/latency_bench.py)
        const long tiles32 = (long)((T + 31) / 32) * L.B;
        ra.z = L.w.zb;
        if (w43) {
            ra.W3f = m->res[l].w3w43;
            rc = cmtts_launch_resblock_w43(&ra, (void*)L.s);
        } else if (g_split_resblock == 2 || (g_split_resblock == 1 && tiles32 <= SPLIT_MAX_TILES)) rc = cmtts_launch_resblock_split(&ra, (void*)L.s);
        else rc = cmtts_launch_resblock(&ra, (void*)L.s);
    } else {
        ra.W3f = (const float*)m->res[l].w3f16[m->precision - 1];
        ra.Wof = (const float*)m->res[l].wof16[m->precision - 1];
        rc = cmtts_launch_resblock_lp(&ra, m->precision, (void*)L.s);
    }
    if (rc != 0) return fail(CMTTS_E_HIP, "fused residual block launch failed");
    prof.launched();
    L.swap();
    return 0;
}

// The same block on the generic conv kernel, three launches (cmtts_set_fused_resblock(0): A/B and bitwise tests); x stays in hcur.
// w43 ("batch_invariant"): the conditioner conv, then the F(4,3) conv and the split projection kernel on its u; x ping-pongs.
int three_launch_layer(Layers& L, int l, bool w43, bool prof_due) {
    const cmtts_config& c = L.m->cfg;
    const int C = c.res_channels, NL = c.res_layers, B = L.B, T = L.T;
    const long cs = (long)C * T;
    const ResLayer& R = L.m->res[l];
    const DenWs& w = L.w;
    {   // u = (x + d [+ p]) + conditioner_projection(cond)      (model/blocks.py:669-677)
        ConvArgs a = conv_args(R.cond, L.cond_ct, T, T, (long)c.hidden * T, L.halt, T, cs, T);
        a.out[0].bvec = L.dp + (long)l * C; a.out[0].bvec_zs = (long)NL * C;
        a.out[0].res = L.hcur; a.out[0].r_zs0 = cs; a.out[0].ldr = T;
        CHK(launch(a, EPI_PLAIN, B, L.s));
    }
    if (w43) {   // u is consumed first
        ResArgs ra = res_args(L, l);
        ra.u = L.halt; ra.z = w.zb; ra.cp = w.cp;
        ra.W3f = R.w3w43;
        if (cmtts_launch_resblock_w43(&ra, (void*)L.s) != 0) return fail(CMTTS_E_HIP, "F(4,3) residual block launch failed");
        L.swap();
        return 0;
    }
    {   // z = sigmoid(gate) * tanh(filter) of the k=3 conv        (:675-679)
        ConvArgs a = conv_args(R.conv3, L.halt, T, T, cs, w.zb, T, cs, T);
        Bracket prof(prof_due, L.s);
        CHK(launch(a, EPI_GATED, B, L.s));
        prof.launched();
    }
    {   // o = output_projection(z); x' = (o[:C] + (x + d)) / sqrt(2); skip += o[C:]   (:681-686)
        ConvArgs a = conv_args(R.outp, w.zb, T, T, cs, L.hcur, T, cs, T);
        a.split = C;
        a.out[0].res = L.hcur; a.out[0].r_zs0 = cs; a.out[0].ldr = T;
        a.out[0].bvec = w.dproj + (long)l * C; a.out[0].bvec_zs = (long)NL * C;
        a.out[0].rmul = 0.70710678118654752440f;      // every form of the block scales by the fp32 reciprocal of sqrt(2) (gate.h: CMTTS_RSQRT2)
        a.out[1].Y = w.skip; a.out[1].row_off = C; a.out[1].accum = l > 0;
        CHK(launch(a, EPI_PLAIN, B, L.s));
    }
    return 0;
}

// sum(skips)/sqrt(NL) -> skip_projection -> relu -> output_projection   (model/modules.py:634-637): F in w.hin [B][80][T]
int skip_head(const Layers& L) {
    const cmtts_model* m = L.m;
    const int T = L.T;
    const long cs = (long)m->cfg.res_channels * T;
    ConvArgs a = conv_args(m->skip_proj, L.w.skip, T, T, cs, L.halt, T, cs, T);
    a.pre_div = (float)sqrt((double)m->cfg.res_layers);
    a.out[0].act = ACT_RELU;
    CHK(launch(a, EPI_PLAIN, L.B, L.s));
    ConvArgs b = conv_args(m->out_proj, L.halt, T, T, cs, L.w.hin, T, (long)m->cfg.n_mels * T, T);
    return launch(b, EPI_PLAIN, L.B, L.s);
}

// Denoiser.forward (model/modules.py:600-639) on ev.x_src [B][T][80], then the sampler's post-scaling: prologue, join of the side branch,
// residual layers, skip head, post-scaling.  The layers: the persistent stack where the mode allows and the launcher takes the shape (with its
// tail, that launch ends the evaluation), else layer by layer — fused kernels, or the three-launch form with cmtts_set_fused_resblock(0).
int denoiser_core(cmtts_model* m, const DenWs& w, const Eval& ev, const float* cond_ct, const float* spk, int B, int T, const MelPost& post,
                  hipStream_t s) {
    CHK(check_device_flag(true));
    const int NL = m->cfg.res_layers, M = m->cfg.n_mels;
    bool halo_zeroed = false;
    CHK(denoiser_prologue(m, w, ev, spk, B, T, s, &halo_zeroed));
    if (ev.pending) CHK(branch_join(ev.pending));
    Layers L = {m, w, cond_ct, m->cfg.multi_speaker ? w.dp : w.dproj, B, T, s, w.h, w.u};
    const int mode = persist_mode(ev.allow_persist);
    bool layers_done = false, tail_done = false;
    if (g_fused_resblock && mode && NL <= PERSIST_MAX_LAYERS) CHK(persistent_stack(L, ev, post, halo_zeroed, mode, &layers_done, &tail_done));
    if (tail_done) return 0;
    if (!layers_done) {
        if (ev.gathers()) {
            // the persistent launch was expected to gather the factors and did not take this shape after all: expand them now
            CHK(cond_factored(m, w, *ev.cfk, B, T, s));
            if (ev.cp_ready) *ev.cp_ready = true;
        }
        const bool w43 = batch_invariant_form(m) > 0;      // every per-layer form takes the persistent stack's F(4,3) conv
        for (int l = 0; l < NL; ++l) {
            const bool prof_due = g_prof.layer_due();
            CHK(g_fused_resblock ? fused_layer(L, l, w43, prof_due) : three_launch_layer(L, l, w43, prof_due));
        }
    }
    CHK(skip_head(L));
    if (post.rows) k_mel_post_rows(w.hin, post.xold, post.noise, post.rows, post.out, post.out_final, B, T, M, g_tmo_host, s);
    else k_mel_post(w.hin, post.xold, post.noise, post.c_out, post.c_skip, post.nstd, post.out, B, T, M, g_tmo_host, s);
    return 0;
}

// ---------------------------------------------------------------- what the entry points share around an evaluation
// The conditioner projections of a call, once for all its evaluations: forked onto the side stream (public option "branch_streams"; in line
// without one) and joined by the first evaluation in front of its residual layers (Eval::pending).  Dense or 16-bit GEMM on the conditioning,
// or — factors the caller handed over — their expansion into w.cp, or nothing but the p1 transpose when the persistent launches will gather
// them (in_kernel: w.cp is free and takes p1 with the channels contiguous, [B][NL][ldp][C]: one transpose per call buys 16-byte gathers in
// every layer of every evaluation).  The three-launch block (cmtts_set_fused_resblock(0)) runs each layer's conditioner conv itself: no branch.
struct CondBranch {
    SideStream* ss = nullptr;
    hipStream_t side = nullptr;      // where the branch's launches go: ss->side, or the caller's stream
    bool in_kernel = false;
    CondFactors kf;                  // in_kernel: the factors as the persistent launches read them
    bool cp_ready = false;           // in_kernel: an evaluation had to expand them into w.cp after all (denoiser_core)
    const CondFactors* cfk() const { return in_kernel ? &kf : nullptr; }
};
int conditioner_branch(cmtts_model* m, const DenWs& w, const float* cond_ct, const CondFactors& cf, int B, int T, bool allow_persist, hipStream_t s,
                       CondBranch* br) {
    const cmtts_config& c = m->cfg;
    br->ss = g_fused_resblock ? side_for(s) : nullptr;
    br->side = br->ss ? br->ss->side : s;
    if (br->ss) CHK(branch_fork(br->ss));
    if (!g_fused_resblock) return 0;
    if (!cf.usable(m)) return cond_projections(m, w, cond_ct, B, T, br->side);
    const int mode = persist_mode(allow_persist);
    const bool inkernel = g_cond_inkernel && mode && g_persist_tail && m->skip_f && m->outp_f && c.res_layers <= PERSIST_MAX_LAYERS &&
                          cmtts_persist_plan(B, T, c.res_layers, persist_blocks(), mode == 2) > 0;
    if (!(inkernel && cf.ldp <= T && m->cond_p2t && C_IS_256(c))) return cond_factored(m, w, cf, B, T, br->side);
    br->in_kernel = true;
    br->kf = cf;
    if (!br->kf.p1t) {      // on the side stream: nothing before the first persistent launch reads it
        k_transpose(cf.p1, w.cp, B * c.res_layers, c.res_channels, cf.ldp, br->side);
        br->kf.p1t = w.cp;
    }
    return 0;
}

// The head of evaluation i of a uniform schedule (every utterance at sigmas[i]: the plain sampler's loop and cmtts_retake's): its scalings, w.tbuf
// and the step embedding brought up to its sigma, and the evaluation's parameters as far as the loops share them.  The first evaluation's step
// embedding reads only the timestep (and the speaker vector): side stream, beside x_T and the input projection, joined with the conditioner
// branch before the residual layers (same kernels, same bits).  Later evaluations embed in line, and only at a new sigma.
struct UniformEval { EvalScalings k; Eval ev; };
int uniform_head(cmtts_model* m, const DenWs& w, const float* spk, int B, const float* sigmas, int i, const CondBranch& br, hipStream_t s,
                 UniformEval* u) {
    u->k = scalings(m->cfg, sigmas[i]);
    const bool new_sigma = i == 0 || sigmas[i] != sigmas[i - 1];
    const bool embed_side = i == 0 && br.ss != nullptr;
    if (new_sigma) k_fill_float(w.tbuf, u->k.t_resc, B, embed_side ? br.side : s);
    if (embed_side) CHK(step_embedding(m, w, w.tbuf, spk, B, br.side, u->k.t_resc));
    u->ev = Eval();
    u->ev.x_src = w.xcur; u->ev.in_scale = u->k.c_in; u->ev.timesteps = w.tbuf;
    u->ev.embed = new_sigma && !embed_side; u->ev.t_host = u->k.t_resc;
    u->ev.pending = i == 0 ? br.ss : nullptr;
    return 0;
}

// ---------------------------------------------------------------- the sampler
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
size_t mixed_eval_bytes(int B) { return (size_t)B * (2 * sizeof(float) + sizeof(PostRow)); }
// The table of a (validated) plan, the scalings of every (evaluation, utterance) by scalings(): `host` takes max_steps blocks of
// mixed_eval_bytes(B), the copy the caller uploads to `dev`, where the plan's pointers point.
void mixed_plan(const cmtts_config& c, const cmtts_step_plan* plan, int B, char* host, const char* dev, MixedPlan* mx) {
    const int NS = plan->max_steps;
    const int32_t* ns = plan->n_steps;
    const size_t eb = mixed_eval_bytes(B);
    mx->ev.resize((size_t)NS);
    std::vector<float> held((size_t)B, NAN);      // the timestep whose embedding row b of the workspace holds
    for (int i = 0; i < NS; ++i) {
        float* c_in = reinterpret_cast<float*>(host + (size_t)i * eb);
        float* tt = c_in + B;
        PostRow* rows = reinterpret_cast<PostRow*>(tt + B);
        MixedEval& e = mx->ev[i];
        e.Bi = 0; e.embed = false; e.t_uniform = true; e.renoise = false;
        for (int b = 0; b < B; ++b) {
            if (i >= ns[b]) {      // left: the row is not evaluated; its timestep stays a valid one for the full-batch step embedding
                c_in[b] = 0.0f; tt[b] = held[b]; rows[b] = PostRow{0.0f, 0.0f, 0.0f, 0u};
                continue;
            }
            const EvalScalings k = scalings(c, plan->sigmas[(long)i * B + b]);
            const float nstd = plan->renoise_std[(long)i * B + b];
            c_in[b] = k.c_in;
            tt[b] = k.t_resc;
            const bool renoise = nstd >= 0.0f;
            rows[b] = PostRow{k.c_out, k.c_skip, renoise ? nstd : 0.0f, (renoise ? POSTROW_RENOISE : 0u) | (i + 1 == ns[b] ? POSTROW_FINAL : 0u)};
            e.Bi = b + 1;
            e.embed = e.embed || tt[b] != held[b];
            e.t_uniform = e.t_uniform && tt[b] == tt[0];
            e.renoise = e.renoise || renoise;
            if (renoise) mx->n_re = i + 1;
        }
        e.t_host = tt[0];
        if (e.embed)
            for (int b = 0; b < B; ++b) held[b] = e.t_uniform ? e.t_host : tt[b];
        e.c_in = reinterpret_cast<const float*>(dev + (size_t)i * eb);
        e.t = e.c_in + B;
        e.rows = reinterpret_cast<const PostRow*>(e.t + B);
    }
}
long g_sample_rows = 0;       // utterance-evaluations launched by the last sampler call (cmtts_internal_sample_rows)

// What a sampler entry point brings to sample_core besides its padded (B, T) batch and carved workspace
struct SampleIn {
    const float* noise = nullptr;        // x_T, then the re-noise draws; with seeds: a buffer that takes the re-noise draws 1 .. only
    long noise_stride = 0;               // elements between consecutive noise tensors (B * T * n_mels for a whole batch; a sub-batch [b0, b0 + B) of a
                                         // larger batch keeps the larger batch's stride)
    const float* cond_ct = nullptr;
    const float* speaker_emb = nullptr;
    CondFactors cf;                      // without p1: the dense conditioner GEMM
    const int64_t* seeds = nullptr;      // cmtts_sample_seeded: device int64 [B]
    bool allow_persist = true;           // persist_mode
};
struct Schedule {
    int n_steps = 0;                     // evaluations
    const float* sigmas = nullptr;       // [n_steps] for all utterances, or ...
    const float* renoise_std = nullptr;
    const MixedPlan* mx = nullptr;       // ... the table of per-utterance schedules (sigmas / renoise_std unused)
};
// What the evaluations of one call keep between them
struct SampleRun {
    CondBranch br;
    const float* renoise0 = nullptr;     // draw 1 + i at renoise0 + i * noise_stride
};

// Once per call: the conditioner branch, x_T = randn * sigma_max (karras_diffusion.py:534) into w.xcur, and with seeds both generated on the
// device (noise_philox.hip): draw 0 scaled by sigma_max — the bits of a draw-0 tensor through k_scale — and the re-noise draws 1 .. n_re in one
// launch on the side stream, beside the conditioner branch.
int sample_setup(cmtts_model* m, const DenWs& w, const SampleIn& in, int B, int T, int n_re, hipStream_t s, SampleRun* run) {
    const cmtts_config& c = m->cfg;
    g_sample_rows = 0;
    CHK(conditioner_branch(m, w, in.cond_ct, in.cf, B, T, in.allow_persist, s, &run->br));
    run->renoise0 = in.noise + in.noise_stride;
    if (!in.seeds) {
        k_scale(in.noise, w.xcur, (long)B * T * c.n_mels, c.sigma_max, s);
        return 0;
    }
    run->renoise0 = in.noise;
    if (cmtts_launch_noise_fill(in.seeds, B, T, c.n_mels, 0, 1, 0, c.sigma_max, w.xcur, nullptr, (void*)s) != 0 ||
        (n_re && cmtts_launch_noise_fill(in.seeds, B, T, c.n_mels, 1, n_re, 0, 1.0f, const_cast<float*>(in.noise), nullptr, (void*)run->br.side) != 0))
        return fail(CMTTS_E_HIP, "seeded noise launch failed");
    return 0;
}

int uniform_steps(cmtts_model* m, const DenWs& w, const SampleIn& in, SampleRun& run, int B, int T, const Schedule& sc, float* mel, hipStream_t s) {
    for (int i = 0; i < sc.n_steps; ++i) {
        UniformEval u;
        CHK(uniform_head(m, w, in.speaker_emb, B, sc.sigmas, i, run.br, s, &u));
        u.ev.cfk = run.br.cfk(); u.ev.cp_ready = &run.br.cp_ready; u.ev.allow_persist = in.allow_persist;
        const bool last = i + 1 == sc.n_steps;
        const bool renoise = sc.renoise_std[i] >= 0.0f;
        const MelPost post = {w.xcur, renoise ? run.renoise0 + (long)i * in.noise_stride : nullptr, u.k.c_out, u.k.c_skip,
                              renoise ? sc.renoise_std[i] : 0.0f, last ? mel : w.xcur};
        CHK(denoiser_core(m, w, u.ev, in.cond_ct, in.speaker_emb, B, T, post, s));
        g_sample_rows += B;
    }
    return 0;
}

// Per-utterance schedules: the same evaluation on the prefix of utterances that still have one to take — every buffer is batch-major, so the
// prefix is the same workspace with a smaller B.  The step embedding runs on all B rows (include/cmtts_hip.h: the K-slicing of its MLP is a
// function of the row count), on the side stream in front of the first evaluation as in uniform_head.
int mixed_steps(cmtts_model* m, const DenWs& w, const SampleIn& in, SampleRun& run, int B, int T, const Schedule& sc, float* mel, hipStream_t s) {
    SideStream* ss = run.br.ss;
    for (int i = 0; i < sc.n_steps; ++i) {
        const MixedEval& e = sc.mx->ev[i];
        if (e.embed) {
            hipStream_t es = i == 0 && ss ? ss->side : s;
            if (e.t_uniform) k_fill_float(w.tbuf, e.t_host, B, es);
            CHK(step_embedding(m, w, e.t_uniform ? w.tbuf : e.t, in.speaker_emb, B, es, e.t_uniform ? e.t_host : NAN));
        }
        MelPost post = {w.xcur, e.renoise ? run.renoise0 + (long)i * in.noise_stride : nullptr, 0.0f, 0.0f, 0.0f, w.xcur};
        post.rows = e.rows; post.out_final = mel;
        Eval ev;
        ev.x_src = w.xcur; ev.in_scale_b = e.c_in; ev.timesteps = w.tbuf; ev.embed = false;
        ev.pending = i == 0 ? ss : nullptr;
        ev.cfk = run.br.cfk(); ev.cp_ready = &run.br.cp_ready; ev.allow_persist = in.allow_persist;
        CHK(denoiser_core(m, w, ev, in.cond_ct, in.speaker_emb, e.Bi, T, post, s));
        g_sample_rows += e.Bi;
    }
    return 0;
}

// The sampler on one padded (B, T) batch whose workspace is already carved
int sample_core(cmtts_model* m, const DenWs& w, const SampleIn& in, int B, int T, const Schedule& sc, float* mel, hipStream_t s) {
    int n_re = sc.mx ? sc.mx->n_re : 0;
    for (int i = 0; i < sc.n_steps && !sc.mx; ++i)
        if (sc.renoise_std[i] >= 0.0f) n_re = i + 1;
    SampleRun run;
    CHK(sample_setup(m, w, in, B, T, n_re, s, &run));
    CHK(sc.mx ? mixed_steps(m, w, in, run, B, T, sc, mel, s) : uniform_steps(m, w, in, run, B, T, sc, mel, s));
    HIPCHK(hipGetLastError());
    return 0;
}
// What most entry points hand over: a whole batch's noise, its conditioning and (possibly empty) factors
SampleIn sample_in(const cmtts_config& c, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T, const CondFactors& cf) {
    SampleIn in;
    in.noise = noise; in.noise_stride = (long)B * T * c.n_mels; in.cond_ct = cond_ct; in.speaker_emb = speaker_emb; in.cf = cf;
    return in;
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

// The factors of utterances [b0, B) of a ragged shard's group; incomplete ones are not usable(): the dense GEMM
CondFactors group_factors(const cmtts_config& c, const cmtts_sample_group& G, int b0) {
    CondFactors cf;
    (void)factors_from(nullptr, G.cond_p1 ? G.cond_p1 + (long)b0 * c.res_layers * c.res_channels * G.p1_ld : nullptr, nullptr, G.p1_ld, G.L,
                       G.mel2ph ? G.mel2ph + (long)b0 * G.T : nullptr, G.p_idx ? G.p_idx + (long)b0 * G.T : nullptr, &cf);
    return cf;
}

// The denoiser workspace, then the re-noise draws 1 .. n_steps of the batch ([n_steps][B][1][T][n_mels], 256-byte aligned) ...
size_t seeded_tail_offset(const cmtts_config& c, int B, int T) { return (carve_den(c, B, T, nullptr).bytes + 255) & ~(size_t)255; }
// ... then (cmtts_sample_mixed) the table: per evaluation c_in [B], t [B], PostRow [B].
size_t mixed_table_offset(const cmtts_config& c, int B, int T, int max_steps) {
    return (seeded_tail_offset(c, B, T) + (size_t)max_steps * B * T * c.n_mels * sizeof(float) + 255) & ~(size_t)255;
}

// ---------------------------------------------------------------- retake
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

// What cmtts_api.hip needs back (launch.h): this unit's rows of cmtts_internal_set ...
int denoiser_internal_set(const char* name, int value, bool* found) {
    static const Knob tab[] = {
        {"cond_inkernel", &g_cond_inkernel, 0, 1}, // fp32 persistent denoiser gathers the conditioner factors itself (same bits as expanding them into cp first)
        {"cond_factored", &g_cond_factored, 0, 1}, // fp32 models: conditioner projections expanded from their phoneme-level / pitch-table factors when the caller hands them over (NOT bitwise the dense GEMM: W a + W b against W (a + b))
        {"cond_gemm16", &g_cond_gemm16, 0, 1},     // 16-bit models: conditioner GEMM with 16-bit operands (NOT bitwise: another operand precision)
        {"cond_gemm", &g_cond_gemm, 0, 2},         // stacked conditioner GEMM on cond_gemm.hip: 0 never, 1 when it pays, 2 whenever supported
        {"persist_tail", &g_persist_tail, 0, 1},   // skip head + post-scaling inside the persistent launch
        {"persist_wino", &g_persist_wino, 0, 3},   // fp32 persistent denoiser's k = 3 conv: 0 direct, 1 (and 2) Winograd F(2,3), 3 F(4,3) (NOT bitwise the direct form)
        {"inproj_fused", &g_inproj_fused, 0, 1},   // denoiser input as one launch
    };
    return knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, found);
}
// ... and the one pinned error word of the process, allocated by the first cmtts_finalize that succeeds
void denoiser_error_word_ready() {
    if (g_tmo_host) return;
    if (hipHostMalloc((void**)&g_tmo_host, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) g_tmo_host = nullptr;
    else *g_tmo_host = 0;
}

// =============================================================================== C ABI
extern "C" {

size_t cmtts_denoiser_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_den(m->cfg, B, T, nullptr).bytes; }

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
    CondBranch br;
    CHK(conditioner_branch(m, w, cond_ct, CondFactors(), B, T, true, s, &br));
    Eval ev;
    ev.x_src = x; ev.timesteps = timesteps; ev.pending = br.ss;
    const MelPost post = {nullptr, nullptr, 1.0f, 0.0f, 0.0f, out};
    CHK(denoiser_core(m, w, ev, cond_ct, speaker_emb, B, T, post, s));
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
    const Schedule sc = {n_steps, sigmas, renoise_std};
    return sample_core(m, w, sample_in(c, noise, cond_ct, speaker_emb, B, T, CondFactors()), B, T, sc, mel, (hipStream_t)stream);
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

// cond_p1t: the caller's channel-contiguous copy of the factor (cmtts_frame_forward_sub_t): no transpose at the sampler's entry
int cmtts_sample_factored_t(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb, int B, int T,
                            int n_steps, const float* sigmas, const float* renoise_std, float* mel, void* ws, size_t ws_bytes,
                            void* stream, const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx) {
    if (!m || !m->finalized) return fail(CMTTS_E_INVALID, "model not finalized");
    if (!noise || !cond_ct || !mel || !ws || !sigmas || !renoise_std || B <= 0 || T <= 0 || n_steps < 1)
        return fail(CMTTS_E_INVALID, "cmtts_sample_factored: bad argument");
    CondFactors cf;
    CHK(factors_from("cmtts_sample_factored", cond_p1, cond_p1t, p1_ld, L, mel2ph, p_idx, &cf));
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    DenWs w = carve_den(c, B, T, ws);
    if (ws_bytes < w.bytes) return fail(CMTTS_E_WORKSPACE, "denoiser workspace too small");
    const Schedule sc = {n_steps, sigmas, renoise_std};
    return sample_core(m, w, sample_in(c, noise, cond_ct, speaker_emb, B, T, cf), B, T, sc, mel, (hipStream_t)stream);
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
    CondFactors cf;
    CHK(factors_from("cmtts_sample_seeded", cond_p1, cond_p1t, p1_ld, L, mel2ph, p_idx, &cf));
    CHK(check_batch_invariant(m));
    const cmtts_config& c = m->cfg;
    if (B > 65535) return fail(CMTTS_E_UNSUPPORTED, "cmtts_sample_seeded: B > 65535");
    DenWs w = carve_den(c, B, T, ws);
    if (ws_bytes < cmtts_sample_seeded_workspace_bytes(m, B, T, n_steps)) return fail(CMTTS_E_WORKSPACE, "seeded sampler workspace too small");
    const float* tail = reinterpret_cast<const float*>(static_cast<char*>(ws) + seeded_tail_offset(c, B, T));
    SampleIn in = sample_in(c, tail, cond_ct, speaker_emb, B, T, cf);
    in.seeds = seeds;
    const Schedule sc = {n_steps, sigmas, renoise_std};
    return sample_core(m, w, in, B, T, sc, mel, (hipStream_t)stream);
}

// ---- mixed step counts in one batch (include/cmtts_hip.h; the definition: cmtts_amd/steps.py)
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
    CondFactors cf;
    CHK(factors_from("cmtts_sample_mixed", cond_p1, cond_p1t, p1_ld, L, mel2ph, p_idx, &cf));
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
    hipStream_t s = (hipStream_t)stream;
    SampleIn in = sample_in(c, seeds ? tail : noise, cond_ct, speaker_emb, B, T, cf);
    in.seeds = seeds;
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
        const Schedule sc = {NS, sg.data(), sd.data()};
        return sample_core(m, w, in, B, T, sc, mel, s);
    }
    // the table, uploaded once in front of the first launch
    std::vector<char> host((size_t)NS * mixed_eval_bytes(B));
    char* dev = static_cast<char*>(ws) + mixed_table_offset(c, B, T, NS);
    MixedPlan mx;
    mixed_plan(c, plan, B, host.data(), dev, &mx);
    HIPCHK(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, s));
    Schedule sc;
    sc.n_steps = NS; sc.mx = &mx;
    return sample_core(m, w, in, B, T, sc, mel, s);
}

// Test hook (internal_hooks.h): utterance-evaluations launched by the last sampler call
long cmtts_internal_sample_rows(void) { return g_sample_rows; }

// ---- re-taking spans of an utterance: the masked sampler on frame windows (retake.hip)

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
    // the uniform sampler's loop on the [N, Tw] batch, the dense conditioner GEMM on the side stream
    CondBranch br;
    CHK(conditioner_branch(m, d, w.cond, CondFactors(), N, Tw, true, s, &br));
    RetakeStepArgs st;
    memset(&st, 0, sizeof(st));
    st.x0 = w.x0; st.known = w.known; st.regen = w.regen; st.seeds = w.seeds; st.win = w.win;
    st.N = N; st.Tw = Tw; st.M = M; st.T = T;
    st.out = d.xcur; st.draw = 0; st.scale = c.sigma_max; st.mode = RETAKE_INIT;
    if (cmtts_launch_retake_step(&st, (void*)s) != 0) return fail(CMTTS_E_HIP, "cmtts_retake: first-draw launch failed");
    for (int i = 0; i < n_steps; ++i) {
        UniformEval u;
        CHK(uniform_head(m, d, spk, N, sigmas, i, br, s, &u));
        const bool last = i + 1 == n_steps;
        const MelPost post = {d.xcur, nullptr, u.k.c_out, u.k.c_skip, 0.0f, w.x0};      // x0 = c_out F + c_skip x, exactly as the plain sampler forms it
        CHK(denoiser_core(m, d, u.ev, w.cond, spk, N, Tw, post, s));
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
        if (!group_factors(c, groups[g], 0).usable(m) || groups[g].p1_ld > groups[g].T || !m->cond_p2t) fact_all = false;
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
        const CondFactors cf = group_factors(c, G, 0);
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
        for (int g = 0; g < n_groups; ++g)
            if (keep[g] < groups[g].B) {
                const cmtts_sample_group& G = groups[g];
                const int b0 = keep[g], nb = G.B - b0;
                const long per = (long)G.T * M;
                SampleIn in;
                in.noise = G.noise + b0 * per; in.noise_stride = (long)G.B * per;
                in.cond_ct = G.cond_ct + (long)b0 * c.hidden * G.T;
                in.speaker_emb = G.speaker_emb ? G.speaker_emb + (long)b0 * c.hidden : nullptr;
                in.cf = group_factors(c, G, b0);
                in.allow_persist = false;      // the per-layer / split kernels, whatever cmtts_set_persistent_denoiser says
                const Schedule sc = {n_steps, sigmas, renoise_std};
                CHK(sample_core(m, den_slice(c, ws[g], b0, G.T), in, nb, G.T, sc, G.mel + b0 * per, q));
            }
    }
    const int cap = cap_all;
    PersistArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.vec_stride = (long)NL * C; pa.tmo = g_tmo_host; pa.NL = NL; pa.halo_zeroed = 1;
    bool wino_state = true;
    for (int g = 0; g < n_groups; ++g)
        if (keep[g] > 0 && !ws[g].pst) wino_state = false;
    persist_model_args(pa, m, wino_state);      // fp32 with the in-kernel tail: one_launch
    pa.n_groups = n_groups;
    if (fact_all) { pa.fact = 1; pa.p2 = m->cond_p2; pa.p2t = m->cond_p2t; pa.ld2 = c.pitch_bins; }
    for (int i = 0; i < n_steps; ++i) {
        const EvalScalings k = scalings(c, sigmas[i]);
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
            if (new_sigma) k_fill_float(w.tbuf, k.t_resc, Bk, s);
            Eval ev;
            ev.x_src = w.xcur; ev.in_scale = k.c_in; ev.timesteps = w.tbuf; ev.embed = new_sigma; ev.t_host = k.t_resc;
            bool hz = false;
            CHK(denoiser_prologue(m, w, ev, G.speaker_emb, Bk, G.T, s, &hz));
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
        pa.c_out = k.c_out; pa.c_skip = k.c_skip; pa.nstd = renoise ? renoise_std[i] : 0.0f;
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
            const bool due = g_prof.room();
            CHK(persist_admit(s, n, persist_blocks()));
            Bracket prof(due, s);
            const int rc = cmtts_launch_denoiser_persist_ragged(&pa, (void*)s);
            if (rc != 0) return fail(rc == -2 ? CMTTS_E_UNSUPPORTED : CMTTS_E_HIP, "ragged persistent denoiser launch failed");
            CHK(persist_launched(s, n));
            prof.launched();
        }
    }
    if (any_aside && ss) { guard.armed = false; CHK(branch_join(ss)); }
    HIPCHK(hipGetLastError());
    return 0;
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
    (void)factors_from(nullptr, p1, nullptr, p1_ld, L, mel2ph, p_idx, &cf);      // the hook expands what it is given
    return cond_factored(m, w, cf, B, T, (hipStream_t)stream);
}

// Test hook (internal_hooks.h): scalings() on the host
void cmtts_internal_eval_scalings(float sigma, float sigma_min, float sigma_data, float* out4) {
    cmtts_config c{};
    c.sigma_min = sigma_min; c.sigma_data = sigma_data;
    const EvalScalings k = scalings(c, sigma);
    out4[0] = k.c_in; out4[1] = k.c_out; out4[2] = k.c_skip; out4[3] = k.t_resc;
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

int cmtts_set_resblock_tile(int frames) {
    if (frames != 0 && frames != 32 && frames != 64) return fail(CMTTS_E_INVALID, "cmtts_set_resblock_tile: 0, 32 or 64");
    cmtts_resblock_set_tile(frames);
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

}  // extern "C"
