// The phoneme-level and the frame-level half's host side: the text / frame / decoder entry points of the C ABI (include/cmtts_hip.h), their
// workspaces, the text-state records' host side, and the two launch sequences they share — the FFT blocks (fft_stack: per block the stages
// self_attention, out_projection, ffn_conv, ffn_linear) and the conv stacks of the duration / energy / pitch predictors (predictor) — each stage
// in the first form that takes its shape.  Weight import: import.hip; handle: model.h; what this unit shares with cmtts_api.hip: launch.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/cmtts_hip.h"
#include "model.h"
#include "launch.h"
#include "internal_hooks.h"
#include "kernels.h"
#include "resblock_pair.h"
#include "attention.h"
#include "text_state.h"

extern "C" int cmtts_launch_conv_xresq(const ConvArgs* a, const float* wq, int nbatch, void* stream, int form);      // conv_xres.hip

namespace {

// Internal switches (internal_hooks.h): a fused kernel against the path it replaces.  Same bits unless noted.
int g_ffn_wino = 1;             // FFT blocks, fp32: the k = 9 FFN conv of the fused launch as three Winograd tap groups (conv_xres.hip WQ instances; NOT bitwise the direct form: fp32
                                // rounding): 1 (default since round 6) = F(2,3) over output pairs, 2 = F(4,3) over output quads (round 5's default), 0 = direct.  Every fp32 FFN
                                // whose shape the X-resident kernel covers then takes it — whatever L and B — so that the text side's bits, and with them durations and lengths,
                                // still do not depend on the batch.
int g_ffn_fused = 1;            // FFT blocks: the FFN linear's K-segment partial products formed inside the k = 9 conv's launch (conv_xres.hip; same bits); 0 = its own launch
int g_ffn_xres = 1;             // encoder k=9 FFN conv through conv_xres.hip when the shape suits it (false: generic kernel)
int g_text_xres = 7;            // FFT blocks, bit mask: 1 = LayerNorm1 + in-projection in one X-resident launch, 2 = out-projection on that kernel (round 4: its 32-column instance, default on), 4 = LayerNorm2 as the prologue of the FFN conv; 0 = separate LayerNorm launches
int g_attn_fused = 1;           // FFT-block attention as QKV projection + ONE fused kernel (attention.hip; key-chunked with an online softmax above L = 192): 0 = three-launch path
int g_xres_small = 1;           // round 4: conv_xres with 32-column tiles for text-side launches that cannot fill the chip (same bits); 0 = the generic kernel there
int g_pred_xl = 1;              // frame-level 256 -> 256 predictor convs on the X-resident conv_xl kernel (bitwise equal); 0 = generic kernel
int g_pred_head = 1;            // predictors: last LayerNorm + linear head as one launch (ln_linear_kernel); 0 = layernorm_ct + chan_linear
int g_pred_wino = 1;            // round 6: the frame-level pitch predictor's k = 5 convs as F(4,3) tap groups (conv_k5q.hip; NOT bitwise the direct form: fp32 Winograd rounding), at every launch size
int g_pred_xres = 1;            // round 4: phoneme-level 256 -> 256 predictor convs on conv_xres (32-column tiles), the previous block's LayerNorm as its prologue (same bits); 0 = generic kernel + LayerNorm launches
int g_energy_head = 1;          // internal switch "energy_head": 1 = in the head's launch (same bits), 0 = energy_embed_kernel behind the join
int g_stats_mlp = 1;            // round 6: cwt_stats_layers as one launch (kernels.hip: stats_mlp_kernel; same bits); 0 = three dense_small launches
int g_cwt_in_phoneme = 1;       // round 4: the pitch predictor's input projection applied before the length regulator (same bits); 0 = over the frames

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

// ---------------------------------------------------------------- what the stages of both sequences share
// What a form's launcher answered: 0 = it has taken the stage; -3 = the HIP launch failed, which fails the call with `what`; anything else
// (-2: the launcher does not cover the shape) = declined, nothing was launched and the caller goes on to its next form.
int taken(int rc, const char* what, bool* took) {
    *took = rc == 0;
    return rc == -3 ? fail(CMTTS_E_HIP, what) : 0;
}

// The opt-in "text16" (cmtts_model_set_option; bf16 / fp16 models): the operand mode (1 = bf16, 2 = fp16) of the text side's contractions on
// conv_mfma16.hip — bias, activation, LayerNorm, softmax, residuals and masks stay fp32 — or 0
int text16_mode(const cmtts_model* m) { return (m->text16 && (m->precision == 1 || m->precision == 2)) ? m->precision : 0; }

// y = (y_conv + res) * nonpad(lens): the residual add and length mask of a contraction's epilogue
void residual_mask(ConvArgs& a, const float* res, long r_zs0, int ldr, const int64_t* lens) {
    a.out[0].res = res; a.out[0].r_zs0 = r_zs0; a.out[0].ldr = ldr; a.out[0].lens = lens;
}

// LayerNorm (eps 1e-12) over the input channels as the prologue of an X-resident launch, applied to the staged tile; columns from lens[b] on become 0
void ln_prologue(ConvArgs& a, const float* g, const float* b, const int64_t* lens, int skip_tiles) {
    a.ln_g = g; a.ln_b = b; a.ln_eps = 1e-12f; a.ln_lens = lens; a.ln_skip_tiles = skip_tiles;
}
void ln_prologue(ConvXlArgs& a, const float* g, const float* b) {
    a.ln_g = g; a.ln_b = b; a.ln_eps = 1e-12f;
}

// A bare batched contraction on the generic kernel, Y[z] = alpha * A[z]^T X[z]: A [K][M] (row stride a_ld, a_cols valid columns), X [K][N], Y [M][N]; no
// taps, bias or activation.  z = (z / zdiv, z % zdiv) steps the operands by (zs0, zs1).
struct GemmStrides { int zdiv; long a_zs0, a_zs1, x_zs0, x_zs1, y_zs0, y_zs1; };
ConvArgs gemm_args(const float* A, int a_ld, int a_cols, int M, int K, const float* X, int ldx, int N, float* Y, int ldy, const GemmStrides& z, float alpha = 1.f) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.a_ld = a_ld; a.a_cols = a_cols; a.M = M; a.K = K; a.taps = 1; a.dil = 1;
    a.X = X; a.ldx = ldx; a.Tin = N; a.N = N;
    a.zdiv = z.zdiv; a.a_zs0 = z.a_zs0; a.a_zs1 = z.a_zs1; a.x_zs0 = z.x_zs0; a.x_zs1 = z.x_zs1;
    a.pre_div = 1.f; a.pre_slope = 1.f; a.split = INT_MAX;
    ConvOut& o = a.out[0];
    o.Y = Y; o.y_zs0 = z.y_zs0; o.y_zs1 = z.y_zs1; o.ldy = ldy; o.Tout = N; o.ostride = 1; o.alpha = alpha; o.div = 1.f;
    return a;
}

// ---------------------------------------------------------------- predictors
struct EnergyHead {        // round 6: get_energy_embedding + the embedding add (model/modules.py:318-328,358-363) as the epilogue of the energy predictor's head (kernels.hip: ln_linear_kernel<1, true>)
    const float* xin; const float* e_target; float e_control; const float* bins; int nbins; const float* E; float* out1; int64_t* e_idx; float* e_scaled;
    bool done;
    const float* e_table = nullptr;      // control table [B][T] in place of e_control (ln_linear_kernel<1, 2>)
};

// One predictor call: [B][.][T] tensors of row pitch ld that ping-pong between bufA and bufB
struct PredRun {
    const Predictor& P;
    int B, T, ld;
    const int64_t* ln_lens;
    float *bufA, *bufB;
    hipStream_t s;
    int mode16;            // 0, or the 16-bit operand mode (text16_mode) of a model with the opt-in "text16": the convs on conv_mfma16.hip (bias + ReLU in fp32)
    bool frame_level;
    float* other(const float* p) const { return p == bufA ? bufB : bufA; }

    // The LayerNorm of block `ln` as its own launch: *cur moves to the other buffer.  The one place; the conv forms that take a pending LayerNorm as their
    // prologue never come here.
    void layernorm(int ln, const float** cur) const {
        float* nd = other(*cur);
        k_layernorm_ct(*cur, nd, P.ln_g[ln], P.ln_b[ln], 1e-12f, ln_lens, B, T, ld, s);
        *cur = nd;
    }

    // The X-resident kernels' argument block (conv_xl, conv_k5q) for conv + bias + ReLU of block li: x (row pitch ldc) -> y
    ConvXlArgs xl_args(size_t li, const float* wf, const float* x, int ldc, float* y) const {
        const PackedConv& w = P.convs[li];
        ConvXlArgs xa;
        memset(&xa, 0, sizeof(xa));
        xa.x = x; xa.y = y; xa.wf = wf; xa.bias = w.bias; xa.bstride = (long)w.cout * ld;
        xa.B = B; xa.C = 256; xa.T = T; xa.ld = ld; xa.k = w.taps; xa.dil = 1; xa.slope = 1.0f; xa.relu = 1;
        if (w.cin != 256) { xa.cin = w.cin; xa.xbstride = (long)w.cin * ldc; }
        return xa;
    }

    // Conv1d + ReLU of block li: *cur (row pitch ldc) -> the other buffer, which becomes *cur.  ln >= 0: `*cur` holds block ln's conv + ReLU output, its
    // LayerNorm not yet applied — the first two forms take it as their prologue, every other form runs behind layernorm().  Returns as soon as a form
    // has taken the conv.
    int conv(size_t li, const float** cur, int ldc, int ln) const {
        const PackedConv& w = P.convs[li];
        float* dst = other(*cur);
        bool took;
        // 1. frame-level k = 5 convs (the pitch predictor, round 6): F(4,3) tap groups over frame quads, the pending LayerNorm as the prologue — at
        // EVERY launch size (conv_k5q.hip splits a tile's rows over workgroups when there are few tiles; the bits do not depend on it).  Only the
        // frame-level predictor: the phoneme-level energy predictor (k = 5 too) feeds a bucketize, has 1/6 of the columns and stays in the direct form
        if (frame_level && !mode16 && g_pred_wino && !ln_lens && li < P.convs_q.size() && P.convs_q[li] && w.taps == 5 && w.cout == 256 &&
            (ln < 0 || w.cin == 256) && (ldc == ld || w.cin != 256)) {
            ConvXlArgs xa = xl_args(li, P.convs_q[li], *cur, ldc, dst);
            if (ln >= 0) ln_prologue(xa, P.ln_g[ln], P.ln_b[ln]);
            CHK(taken(cmtts_launch_conv_k5q(&xa, (void*)s), "conv_k5q launch failed", &took));
            if (took) { *cur = dst; return 0; }
        }
        // 2. phoneme-level 256 -> 256 convs (round 4): X-resident, one 32-column n-tile per wave, the pending LayerNorm (eps 1e-12, length
        // mask) applied to the staged tile.  (Round 2 tried this with 96-column tiles: 64 workgroups of ~45 us — slower; deleted in round 3.)
        const bool small = (long)((T + 63) / 64) * B < 192;
        if (!mode16 && g_pred_xres && small && P.convs_f[li] && w.cin == 256 && w.cout == 256 && ldc == ld) {
            ConvArgs a = conv_args(w, *cur, T, ldc, (long)w.cin * ldc, dst, ld, (long)w.cout * ld, T);
            a.out[0].act = ACT_RELU;
            a.xres_nt = 1;
            if (ln >= 0) ln_prologue(a, P.ln_g[ln], P.ln_b[ln], ln_lens, 1);      // (the next block's LayerNorm / ln_linear masks the same columns)
            CHK(taken(cmtts_launch_conv_xres(&a, P.convs_f[li], B, (void*)s), "conv_xres launch failed", &took));
            if (took) { *cur = dst; return 0; }
        }
        if (ln >= 0) {
            layernorm(ln, cur);
            dst = other(*cur);
        }
        ConvArgs a = conv_args(w, *cur, T, ldc, (long)w.cin * ldc, dst, ld, (long)w.cout * ld, T);
        a.out[0].act = ACT_RELU;
        // 3. "text16": 16-bit operands
        if (mode16 && li < P.convs_f16[mode16 - 1].size() && P.convs_f16[mode16 - 1][li]) {
            a.text_epi = 1;
            CHK(taken(cmtts_launch_conv16(&a, P.convs_f16[mode16 - 1][li], mode16, B, (void*)s), "text16: predictor conv launch failed", &took));
            if (took) { *cur = dst; return 0; }
            a.text_epi = 0;
        }
        // 4. frame-level 256 -> 256 conv: whole x tile + halo resident in LDS, weights streamed as A fragments (the HiFi-GAN
        // kernel, resblock_pair.hip; same accumulation order and epilogue expressions as the generic kernel => same bits)
        if (g_pred_xl && P.convs_f[li] && ldc == ld && !small) {
            ConvXlArgs xa = xl_args(li, P.convs_f[li], *cur, ldc, dst);
            CHK(taken(cmtts_launch_conv_xl(&xa, (void*)s), "conv_xl launch failed", &took));
            if (took) { *cur = dst; return 0; }
        }
        // 5. the generic kernel: every shape
        CHK(launch(a, EPI_PLAIN, B, s));
        *cur = dst;
        return 0;
    }
};

// conv stack of Duration/Pitch/Energy predictors (model/modules.py:477-487): Conv1d + ReLU ->
// LayerNorm over channels (eps 1e-12) [-> mask].  Result ends in bufB.
// conv -> ReLU -> LayerNorm blocks of a predictor followed by its linear head (model/modules.py:470-506, 520-554): the last
// block's LayerNorm and the head are one launch (ln_linear_kernel) unless cmtts_internal_set("pred_head", 0)
int predictor(const Predictor& P, const float* in, int ld_in, int B, int T, int ld, const int64_t* ln_lens,
              const int64_t* out_lens, float* bufA, float* bufB, float* out, int O, hipStream_t s, int mode16 = 0, bool frame_level = false,
              EnergyHead* eh = nullptr) {      // eh: the energy predictor — bucketize + embedding add inside the head's launch (eh->done reports it)
    const PredRun r{P, B, T, ld, ln_lens, bufA, bufB, s, mode16, frame_level};
    const float* cur = in;
    int ln = -1;                 // >= 0: `cur` holds block ln's conv + ReLU output, its LayerNorm not yet applied
    for (size_t li = 0; li < P.convs.size(); ++li) {
        CHK(r.conv(li, &cur, li == 0 ? ld_in : ld, ln));
        const bool last256 = li + 1 == P.convs.size() && P.convs[li].cout == 256;
        if (g_pred_head && eh && g_energy_head && O == 1 && last256) {
            k_ln_linear_energy(cur, P.ln_g[li], P.ln_b[li], 1e-12f, P.lin_w, P.lin_b, out, ln_lens, out_lens, B, T, ld, eh->xin, eh->e_target, eh->e_control,
                               eh->bins, eh->nbins, eh->E, eh->out1, eh->e_idx, eh->e_scaled, s, eh->e_table);
            eh->done = true;
            return 0;
        }
        if (g_pred_head && last256 && k_ln_linear(cur, P.ln_g[li], P.ln_b[li], 1e-12f, P.lin_w, P.lin_b, out, ln_lens, out_lens, B, T, ld, O, s))
            return 0;
        ln = (int)li;
    }
    if (ln >= 0) r.layernorm(ln, &cur);
    k_chan_linear(cur, P.lin_w, P.lin_b, out, out_lens, B, P.convs.back().cout, T, ld, O, s);
    return 0;
}

// ---------------------------------------------------------------- FFT blocks
// One of a block's two LayerNorms (eps 1e-12), w.x -> w.h.  A stage whose X-resident form covers the shape takes it as that launch's prologue on w.x (no
// normalised copy in HBM); a launcher that declines, and every other form, reads w.h behind FftRun::layernorm_to_h — the one place that launches it on its own.
struct BlockNorm {
    const float *g, *b;
    const int64_t* lens;
    bool in_h = false;
};

// Where ffn_conv left its result, which is what ffn_linear starts from
enum FfnForm {
    FFN_ROWS,        // the activated rows in w.f
    FFN_ROWS16,      // the same from the 16-bit kernel: the linear takes 16-bit operands too
    FFN_PARTIALS,    // the FFN linear's K-segment partial products in w.part already
};

// One call of fft_stack: what it decides once from its shape and the switches, and the stages of a block, which only read it.  Every stage returns as soon as
// a form has taken it.
struct FftRun {
    cmtts_model* m;
    const TextWs& w;
    const int64_t *src_lens, *pad_lens;
    int B, L, Lp, H, NH, dh;
    long hs;                   // batch stride H * Lp
    hipStream_t s;
    // X-resident kernel (conv_xres.hip) for the K = 256 contractions: with 96-column tiles (three n-tiles per wave) when they pad no more
    // than 64-column ones and give every CU a workgroup; round 4: with 32-column tiles (one n-tile per wave, a third of the X tile staged
    // per workgroup) for launches that cannot fill the chip anyway — one request, a few utterances: the LayerNorm prologue, the FFN
    // fusion and a K loop without barriers instead of LayerNorm + generic kernel (+ FFN linear); every path has the same bits
    int t96;                   // 96-column tiles per utterance
    bool xres_small;           // the FFN conv's 96-column grid leaves CUs idle
    bool xres_cols;
    bool fused_attn;           // L <= 192: all keys in registers; longer: key-chunked online softmax (attention.hip)
    int mode16;                // text16_mode(m)
    // the in-projection's tile width.  More workgroups than CUs with 96-column tiles (B = 64, or two column tiles per utterance): the 32-column instance packs two
    // per CU and overlaps their phases — 45-55 us less per text side at 64 x 85 and 32 x 171 phonemes, neutral at 32 x 85 (tools/text_xres_ab2.py)
    int qkv_nt;

    // a launch of `mblocks` 128-row blocks per column tile is worth the X-resident kernel: it gives every CU a workgroup, or takes the 32-column tiles
    bool xres_pays(long mblocks) const { return xres_cols && ((long)t96 * mblocks * B >= 128 || xres_small); }

    // opt-in "text16": the block's four K = 256 / 1024 contractions (in-projection, out-projection, FFN conv, FFN linear) with 16-bit MFMA operands and fp32
    // accumulate on conv_mfma16.hip; LayerNorm, softmax, bias, scale, GELU, residuals, masks fp32.  A block without all four fragment copies stays fp32.
    bool block16(const EncLayer& E) const {
        return mode16 && E.ffn1_f16[mode16 - 1] && E.ffn2_f16[mode16 - 1] && E.qkv_f16[mode16 - 1] && E.wo_f16[mode16 - 1];
    }

    void layernorm_to_h(BlockNorm& n) const {
        if (n.in_h) return;
        k_layernorm_ct(w.x, w.h, n.g, n.b, 1e-12f, n.lens, B, L, Lp, s);
        n.in_h = true;
    }

    // q, k, v = LayerNorm1(x) * W_in^T as ONE contraction: w.x -> w.qk [B][3H][Lp]
    int in_projection(const EncLayer& E, BlockNorm& ln1) const {
        bool took;
        const bool t16 = block16(E);
        // 1. LayerNorm1 as the prologue of the in-projection: one launch, no normalised copy in HBM
        if (!t16 && (g_text_xres & 1) && E.qkv_f && xres_pays(3 * H / 128)) {
            ConvArgs a = conv_args(E.qkv, w.x, L, Lp, hs, w.qk, Lp, 3 * hs, L);
            if (g_text_xres & 8) {   // debugging aid: the projection on the X-resident kernel behind a separate LayerNorm launch
                layernorm_to_h(ln1);
                a.X = w.h;
            } else {
                ln_prologue(a, ln1.g, ln1.b, nullptr, 0);
            }
            a.xres_nt = qkv_nt;
            CHK(taken(cmtts_launch_conv_xres(&a, E.qkv_f, B, (void*)s), "conv_xres launch failed", &took));
            if (took) return 0;
        }
        layernorm_to_h(ln1);
        ConvArgs a = conv_args(E.qkv, w.h, L, Lp, hs, w.qk, Lp, 3 * hs, L);
        if (t16) {      // 2. "text16"
            a.text_epi = 1;
            CHK(taken(cmtts_launch_conv16(&a, E.qkv_f16[mode16 - 1], mode16, B, (void*)s), "text16: in-projection launch failed", &took));
            if (took) return 0;
            a.text_epi = 0;
        }
        return launch(a, EPI_PLAIN, B, s);      // 3. the generic kernel
    }

    // softmax(q k^T / sqrt(dh) + mask) v as five launches of the generic kernels: LayerNorm1(x) in w.h -> w.o.
    // The V projection is needed only by the PV product: side stream, joined after the softmax
    int attention_three_launch(const EncLayer& E) const {
        SideStream* ss = side_for(s);
        hipStream_t sv = ss ? ss->side : s;
        if (ss) CHK(branch_fork(ss));
        {   // Q,K = h * W[0:2H]^T, channel-major [B][2H][Lp]
            ConvArgs a = conv_args(E.qk, w.h, L, Lp, hs, w.qk, Lp, 2 * hs, L);
            CHK(launch(a, EPI_PLAIN, B, s));
        }
        {   // V^T[b] = h[b]^T * Wv^T : [L][H]   (A operand = activation, X operand = weights)
            ConvArgs a = gemm_args(w.h, Lp, Lp, L, H, E.wvT, H, H, w.vt, H, {1, hs, 0, 0, 0, (long)Lp * H, 0});
            CHK(launch(a, EPI_PLAIN, B, sv));
        }
        {   // S^T[b,h][j][i] = sum_d K[d][j] Q[d][i] / sqrt(dh)
            ConvArgs a = gemm_args(w.qk + hs, Lp, Lp, L, dh, w.qk, Lp, L, w.st, Lp,
                                   {NH, 2 * hs, (long)dh * Lp, 2 * hs, (long)dh * Lp, (long)NH * Lp * Lp, (long)Lp * Lp}, (float)(1.0 / sqrt((double)dh)));
            CHK(launch(a, EPI_PLAIN, B * NH, s));
        }
        k_softmax_cols(w.st, src_lens, B * NH, NH, L, Lp, (long)Lp * Lp, s);
        if (ss) CHK(branch_join(ss));
        {   // O[b,h][d][i] = sum_j V^T[j][d] P^T[j][i]
            ConvArgs a = gemm_args(w.vt, H, dh, dh, L, w.st, Lp, L, w.o, Lp, {NH, (long)Lp * H, dh, (long)NH * Lp * Lp, (long)Lp * Lp, hs, (long)dh * Lp});
            CHK(launch(a, EPI_PLAIN, B * NH, s));
        }
        return 0;
    }

    // MultiheadAttention on LayerNorm1(x) without its out-projection (model/blocks.py:606-608): w.x -> w.o
    int self_attention(const EncLayer& E, BlockNorm& ln1) const {
        // 1. the in-projection, then softmax(q k^T / sqrt(dh) + mask) v in one launch per layer: scores and probabilities never leave the CU (attention.hip)
        if (fused_attn) {
            CHK(in_projection(E, ln1));
            AttnArgs at;
            memset(&at, 0, sizeof(at));
            at.qkv = w.qk; at.out = w.o; at.lens = src_lens; at.bstride = 3 * hs; at.obstride = hs;
            at.B = B; at.H = NH; at.dh = dh; at.L = L; at.ld = Lp; at.scale = (float)(1.0 / sqrt((double)dh));
            bool took;
            CHK(taken(cmtts_launch_attention(&at, (void*)s), "attention launch failed", &took));
            if (took) return 0;
        }
        // 2. the three-launch path, with projections of its own
        layernorm_to_h(ln1);
        return attention_three_launch(E);
    }

    // x = (x + out_proj(o)) * nonpad      (model/blocks.py:609-610)
    int out_projection(const EncLayer& E) const {
        ConvArgs a = conv_args(E.wo, w.o, L, Lp, hs, w.x, Lp, hs, L);
        residual_mask(a, w.x, hs, Lp, src_lens);
        bool took;
        if (block16(E)) {          // 1. "text16"
            a.text_epi = 1;
            CHK(taken(cmtts_launch_conv16(&a, E.wo_f16[mode16 - 1], mode16, B, (void*)s), "text16: out-projection launch failed", &took));
            if (took) return 0;
            a.text_epi = 0;
        } else if (E.wo_f && g_ffn_xres && (g_text_xres & 2)) {      // 2. the X-resident kernel
            // round 4: M = 256 is two m-blocks — with 96-column tiles 64 workgroups at B = 32 (measured slower than the generic kernel in round 2);
            // with 32-column tiles 192 workgroups of one short chain each, the tile staged once, no barrier in the K loop: 25 -> 13 us per block
            a.xres_nt = 1;
            CHK(taken(cmtts_launch_conv_xres(&a, E.wo_f, B, (void*)s), "conv_xres launch failed", &took));
            if (took) return 0;
            a.xres_nt = 0;
        }
        return launch(a, EPI_PLAIN, B, s);      // 3. the generic kernel
    }

    // gelu((conv_k9(LayerNorm2(x)) + b) * k^-0.5)      (model/blocks.py:539-546, 612-615): w.x -> w.f, or on to w.part
    int ffn_conv(const EncLayer& E, BlockNorm& ln2, FfnForm* form) const {
        bool took;
        ConvArgs a = conv_args(E.ffn1, w.h, L, Lp, hs, w.f, Lp, 4 * hs, L);
        a.out[0].alpha = (float)pow((double)m->cfg.ffn_kernel, -0.5);
        a.out[0].act = ACT_GELU_ERF;
        // 1. "text16": LayerNorm2, FFN conv (+ k^-0.5, GELU), FFN linear (+ residual, mask): three launches instead of two
        if (block16(E)) {
            layernorm_to_h(ln2);
            a.text_epi = 1;
            CHK(taken(cmtts_launch_conv16(&a, E.ffn1_f16[mode16 - 1], mode16, B, (void*)s), "text16: FFN conv launch failed", &took));
            if (took) { *form = FFN_ROWS16; return 0; }
            a.text_epi = 0;
        }
        *form = FFN_ROWS;
        // X-resident kernel when it fills the chip; LayerNorm2 is then its prologue
        // round 5: with the F(4,3) form available the X-resident fused launch is taken at EVERY L and B (the Winograd and the direct form differ by fp32
        // rounding: one form for all shapes keeps the text side independent of the batch)
        const bool fusable = g_ffn_fused && ffn2_seg(E) && E.ffn2_f && E.ffn1.cout == FFN2_SEG * 128;
        const float* wqf = g_ffn_wino == 2 ? E.ffn1_q : E.ffn1_p;
        const bool wq = g_ffn_wino && g_ffn_xres && fusable && (g_text_xres & 4) && wqf && H == 256;
        if (wq || (E.ffn1_f && xres_pays((E.ffn1.cout + 127) / 128))) {
            if (g_text_xres & 4) {
                a.X = w.x;
                ln_prologue(a, ln2.g, ln2.b, pad_lens, pad_lens != nullptr);      // (reduce_partials and the k = 1 linear mask by select)
            } else {
                layernorm_to_h(ln2);
            }
            if (fusable) {
                // 2. ... and the FFN linear's partial products in the same launch: the activated rows never leave the CU.  The conv as Winograd tap groups (wq), else direct
                a.w2frag = E.ffn2_f; a.part = w.part; a.part_zs0 = (long)FFN2_SEG * hs; a.part_zs1 = hs; a.part_ld = Lp; a.M2 = H;
                took = false;
                if (wq) CHK(taken(cmtts_launch_conv_xresq(&a, wqf, B, (void*)s, g_ffn_wino == 2 ? 1 : 2), "conv_xres launch failed", &took));
                if (!took) CHK(taken(cmtts_launch_conv_xres(&a, E.ffn1_f, B, (void*)s), "conv_xres launch failed", &took));
                if (took) { *form = FFN_PARTIALS; return 0; }
                a.w2frag = nullptr; a.part = nullptr;
            }
            // 3. the conv alone on the X-resident kernel
            CHK(taken(cmtts_launch_conv_xres(&a, E.ffn1_f, B, (void*)s), "conv_xres launch failed", &took));
            if (took) return 0;
            a.ln_g = a.ln_b = nullptr; a.ln_lens = nullptr;
        }
        // 4. the generic kernel behind a LayerNorm launch
        layernorm_to_h(ln2);
        a.X = w.h;
        return launch(a, EPI_PLAIN, B, s);
    }

    bool ffn2_seg(const EncLayer& E) const { return m->ffn2_split && E.ffn2.cin % FFN2_SEG == 0 && E.ffn2.taps == 1; }

    // x = (x + ffn_2(.)) * nonpad          (model/blocks.py:551, :616-617)
    int ffn_linear(const EncLayer& E, FfnForm from) const {
        if (from == FFN_PARTIALS) {
            k_reduce_partials(w.part, FFN2_SEG, E.ffn2.bias, w.x, src_lens, w.x, B, H, L, Lp, s);
            return 0;
        }
        if (from == FFN_ROWS16) {      // a 16-bit FFN conv is followed by the 16-bit linear: a launcher that declines here fails the call
            ConvArgs b = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.x, Lp, hs, L);
            residual_mask(b, w.x, hs, Lp, src_lens);
            b.text_epi = 1;
            if (cmtts_launch_conv16(&b, E.ffn2_f16[mode16 - 1], mode16, B, (void*)s) != 0) return fail(CMTTS_E_HIP, "text16: FFN linear launch failed");
            return 0;
        }
        if (ffn2_seg(E)) {      // as FFN2_SEG independent partial GEMMs + one reduction
            const int kseg = E.ffn2.cin / FFN2_SEG;
            ConvArgs a = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.part, Lp, (long)FFN2_SEG * hs, L);
            a.K = kseg;
            a.zdiv = FFN2_SEG; a.a_zs0 = 0; a.a_zs1 = (long)kseg * a.a_ld; a.x_zs1 = (long)kseg * Lp;
            a.out[0].y_zs1 = hs; a.out[0].bias = nullptr;
            // (64x64 tiles for the 85-phoneme case — a 128-column tile is one third padding — were tried: 59 vs 44 us)
            CHK(launch(a, EPI_PLAIN, B * FFN2_SEG, s));
            k_reduce_partials(w.part, FFN2_SEG, E.ffn2.bias, w.x, src_lens, w.x, B, H, L, Lp, s);
            return 0;
        }
        ConvArgs a = conv_args(E.ffn2, w.f, L, Lp, 4 * hs, w.x, Lp, hs, L);
        residual_mask(a, w.x, hs, Lp, src_lens);
        return launch(a, EPI_PLAIN, B, s);
    }
};

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
    const int t96 = (L + 95) / 96, t64 = (L + 63) / 64;
    const bool cols96 = t96 * 96 <= t64 * 64;
    const bool xres_small = g_ffn_xres && g_xres_small && (long)t96 * B * 8 < 128;
    const FftRun r{m, w, src_lens, pad_lens, B, L, Lp, H, NH, dh, (long)H * Lp, s,
                   t96, xres_small, g_ffn_xres && (cols96 || xres_small), g_attn_fused && dh == 128, text16_mode(m),
                   (long)t96 * (3 * H / 128) * B > persist_blocks() ? 1 : 0};
    for (const EncLayer& E : layers) {
        BlockNorm ln1{E.ln1_g, E.ln1_b, nullptr}, ln2{E.ln2_g, E.ln2_b, pad_lens};
        FfnForm f;
        CHK(r.self_attention(E, ln1));
        CHK(r.out_projection(E));
        CHK(r.ffn_conv(E, ln2, &f));
        CHK(r.ffn_linear(E, f));
    }
    return 0;
}

// ---- per-utterance text-side state records (text_state.hip): the regions of a text workspace that cmtts_frame_forward_sub reads —
// out1 [H][Lp], h128 [cwt_hidden][Lp], spk [H] (fp32), cum [L] (int32), and with a pitch control table installed its rows pctl [L] (fp32) —
// behind a 64-byte header, each region 16-byte aligned.
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

// The text / frame side's rows of cmtts_internal_set (launch.h)
int text_internal_set(const char* name, int value, bool* found) {
    static const Knob tab[] = {
        {"cwt_in_phoneme", &g_cwt_in_phoneme, 0, 1},   // Linear(256 -> 128) of the pitch predictor before (1) or after (0) the length regulator
        {"pred_xres", &g_pred_xres, 0, 1},         // phoneme-level predictor convs on conv_xres with the LayerNorm prologue
        {"xres_small", &g_xres_small, 0, 1},       // FFT blocks of small batches on conv_xres with 32-column tiles
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
    return knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, found);
}

// =============================================================================== C ABI
extern "C" {

size_t cmtts_text_workspace_bytes(const cmtts_model* m, int B, int L) { return carve_text(m->cfg, B, L, nullptr).bytes; }
size_t cmtts_frame_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_frame(m->cfg, B, T, nullptr).bytes; }
size_t cmtts_decoder_workspace_bytes(const cmtts_model* m, int B, int T) { return carve_text(m->cfg, B, T, nullptr).bytes; }

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
    const int t16mode = text16_mode(m);
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
        bool took = false;
        if (g_ffn_xres && g_pred_xres && m->cwt_in_f) {      // 128 rows = one m-block: 32-column tiles, no barrier in the K loop (same bits)
            a.xres_nt = 1;
            CHK(taken(cmtts_launch_conv_xres(&a, m->cwt_in_f, B, (void*)s), "conv_xres launch failed", &took));
            a.xres_nt = 0;
        }
        if (!took) CHK(launch(a, EPI_PLAIN, B, s));
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
    CHK(predictor(m->cwt, w.hp, T, B, T, T, nullptr, nullptr, w.c1, w.c2, cwt_out, O, s, text16_mode(m), true));
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

}  // extern "C"
