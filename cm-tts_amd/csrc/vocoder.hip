// The HiFi-GAN vocoder's host side: the vocoder entry points of the C ABI (include/cmtts_hip.h) and the generator's launch sequence —
// per stage an upsampler and three ResBlocks (hifigan/models.py:149-165), each ResBlock in the first form that takes its shape.
// Weight import: import.hip; handle: model.h; what this unit shares with cmtts_api.hip and text_side.hip: launch.h.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cmtts_hip.h"
#include "model.h"
#include "launch.h"
#include "internal_hooks.h"
#include "kernels.h"
#include "resblock_pair.h"
#include "stream_windows.h"

namespace {

// Internal switches (internal_hooks.h): a fused kernel against the path it replaces.  Same bits unless noted.
int g_voc_pair = 1;             // ResBlock pairs (conv1, LeakyReLU, conv2, + x) as one launch (resblock_pair{,16}.hip, resblock_pairw16.hip, resblock_pair16x3.hip): 0 never, 1 / 2 yes
int g_voc_pair3 = 1;            // fp16x3: pairs at C <= 128 as ONE X-resident launch (resblock_pair16x3.hip) and C = 256 convs on conv_xl16x3; 0 = two conv16 launches per pair
int g_voc_pairw = 1;            // 16-bit, C = 128: pair as ONE launch with one in-place LDS image, two workgroups per CU (resblock_pairw16.hip); 0 = two conv_xl16 launches
int g_voc_rb16 = 1;             // 16-bit, C <= 64: a whole ResBlock (three pairs) per launch (resblock16.hip): 0 never, 1 where it pays, 2 always
int g_voc_xl = 1;               // fp32 ResBlock convs of the C >= 128 stages on the X-resident kernel (conv_xl); 0 = generic kernel
int g_voc_xl16 = 1;             // 16-bit ResBlock convs at C >= 128 on the X-resident conv_xl16 kernel; 0 = chunked conv_mfma16 kernel
int g_voc_upsT = 1;             // upsamplers: all phases of a ConvTranspose1d in one X-resident launch; 0 = generic kernel, one z per phase
int g_voc_wino = 1;             // fp32, C >= 128: ResBlock convs in their Winograd form (conv_xlw_kernel; NOT bitwise the direct form): 0 never, 1 launches of >= 1024 column tiles, 2 always (tests)
int g_voc_wino43 = 1;           // fp32: convs of the Winograd path in the F(4,3) form (conv_xlq_kernel) instead of F(2,3) tap groups (NOT bitwise either): 1 = dilation 1 and 3 everywhere
                                // + dilation 5 at C = 256 or k = 3 (default), 2 = only dilation 1, 3 = every dilation, 0 = none
int g_voc_qpair = 1;            // fp32, k = 3 pairs at C = 64 / 128 of the Winograd path: both convs F(4,3) in ONE launch, xt on the CU (conv_xlq_pair.hip; NOT bitwise the two conv_xlq
                                // launches: the quads of its conv1 start one frame earlier): 0 never, 1 launches of >= 1024 column tiles, 2 always (tests)
int g_voc_wino64 = 1;           // fp32, C = 64, k >= voc_wino64_k: two Winograd launches per pair instead of the pair kernel
int g_voc_wino64_k = 7;         // smallest kernel size of the C = 64 stage that takes the two-launch Winograd form

// The three ResBlocks of an MRF stage are independent until their sum: they run on three streams (own xt / residual
// buffers, + 4 stage buffers of workspace).  Small batches, whose convs cannot fill the chip (stage 2 has B*T/2
// workgroups), gain most — one 150-frame utterance 4.1 -> 2.7 ms — and 32 x 512 frames still 1 % (tails of one ResBlock's
// launches under the next one's).  Above this many mel frames per call the extra workspace (4 x 32 KB per frame) is not
// spent and the ResBlocks run in line.
constexpr long VOC_PAR_FRAMES = 65536;

struct Stage {               // what the three ResBlocks of stage i share
    const cmtts_vocoder* v;
    int i, B, co, To;        // channels and row length (= row stride) of the ResBlocks' tensors
    long cs;                 // batch stride co * To
    const float* x;          // the upsampled input
    bool big_launch;         // the launch-size gate of the fp32 Winograd forms (xw64, qpair; conv_xlq / conv_xlw through wino_force), per stage from its To.  Vocoder option
                             // "batch_invariant": the large-launch branch at every size, so that a row's bits do not depend on the batch (every other size-dependent choice of this
                             // unit — conv_xl's m-tile split "voc_xl_split", the generic conv's tile configurations, the upsamplers' phase split — only divides the same work)
};

// ResBlock j of a stage: its stream and buffers, and the one place that orders the MRF sum.  The sum accumulates in ResBlock order (bit-identical to the
// in-line order): wait for chain j - 1 directly before the launch that writes bufS — not earlier, the launches before it overlap chain j - 1 — and record directly after it.
struct Chain {
    SideStream* ss;          // null: everything runs in line on one stream
    int j;
    hipStream_t q;
    float *bT, *bR, *bufS;   // xt, running residual, MRF sum
    int before_sum() const {
        if (ss && j > 0) HIPCHK(hipStreamWaitEvent(q, j == 1 ? ss->done0 : ss->done1, 0));
        return 0;
    }
    int after_sum() const {
        if (ss && j < 2) HIPCHK(hipEventRecord(j == 0 ? ss->done0 : ss->done1, q));
        return 0;
    }
};

// x = ups[i](leaky_relu(x, 0.1)) (hifigan/models.py:152-153); pre_div: x = xs / num_kernels of the previous stage (:160)
int upsample(const cmtts_vocoder* v, int i, const float* x, float* y, int B, int ch, int Ti, hipStream_t s) {
    const int st = v->up_rate[i], K = v->up_kernel[i], co = ch / 2, To = Ti * st, p = v->precision;
    const PackedConv& U = v->ups[i];
    const float pre_div = i > 0 ? 3.0f : 1.0f;
    int rt = -2;
    if (v->ups16 && p >= 1 && p <= 3 && v->ups_f16[i][p - 1] && K == 2 * st)      // 16-bit modes: 16-bit operands here too (fp16x3: (hi, lo) pairs like the ResBlock convs)
        rt = cmtts_launch_convT16(x, y, v->ups_f16[i][p - 1], U.bias, (long)ch * Ti, (long)co * To, B, ch, co, Ti, To, Ti, To, st, pre_div, 0.1f, p, (void*)s);
    if (rt == -3) return fail(CMTTS_E_HIP, "convT16 launch failed");
    if (rt != 0 && g_voc_upsT && v->ups_f[i] && K == 2 * st)      // all phases in one X-resident launch (same bits)
        rt = cmtts_launch_convT(x, y, v->ups_f[i], U.bias, (long)ch * Ti, (long)co * To, B, ch, co, Ti, To, Ti, To, st, pre_div, 0.1f, (void*)s);
    if (rt == -3) return fail(CMTTS_E_HIP, "convT launch failed");
    if (rt == 0) return 0;
    // generic kernel: `st` polyphase sub-convolutions, one z per phase
    ConvArgs a = conv_args(U, x, Ti, Ti, (long)ch * Ti, y, To, (long)co * To, Ti + 1);
    a.dil = -1; a.pad = 0;
    a.zdiv = st; a.a_zs0 = 0; a.a_zs1 = U.phase_stride; a.x_zs0 = (long)ch * Ti; a.x_zs1 = 0;
    a.pre_slope = 0.1f;
    a.pre_div = pre_div;
    ConvOut& o = a.out[0];
    o.Tout = To; o.ostride = st; o.ooff_base = -((K - st) / 2); o.ooff_mul = 1; o.y_zs0 = (long)co * To; o.y_zs1 = 0;
    return launch(a, EPI_PLAIN, B * st, s);
}

// The three (conv1 at dilation 1 / 3 / 5, conv2) pairs of ResBlock r, one launch per pair.  declined != null: the launcher may turn the shape
// down (-2), then nothing has been launched and *declined is set.
template <class F>
int pair_chain(const Stage& g, const Chain& c, int r, const void* const* w1, const void* const* w2, F launch_pair, const char* what, bool* declined) {
    const cmtts_vocoder* v = g.v;
    const float* xr = g.x;
    for (int mi = 0; mi < 3; ++mi) {
        const bool lastm = mi == 2;
        PairArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.x = xr; pa.y = lastm ? c.bufS : (mi == 0 ? c.bR : c.bT);      // ping-pong: a pair's output must not alias its input; the last pair writes the MRF sum
        pa.b1 = v->c1[r][mi].bias; pa.b2 = v->c2[r][mi].bias;
        pa.w1f = w1[mi]; pa.w2f = w2[mi];
        pa.bstride = g.cs; pa.B = g.B; pa.C = g.co; pa.T = g.To; pa.ld = g.To; pa.k = v->rb_kernel[c.j]; pa.dil = v->rb_dil[mi];
        pa.accum = lastm && c.j > 0; pa.slope = 0.1f;
        if (lastm) CHK(c.before_sum());
        const int rc = launch_pair(&pa, (void*)c.q);
        if (rc == -2 && mi == 0 && declined) {      // -2 is honoured only here, before anything has been launched for this ResBlock; later it is an error
            *declined = true;
            return 0;
        }
        if (rc != 0) return fail(CMTTS_E_HIP, what);
        if (lastm) CHK(c.after_sum());
        xr = pa.y;
    }
    return 0;
}

// One pair on an X-resident per-conv kernel: conv1 x -> xt, conv2 xt (+ x) -> y.  run(xa, 1 | 2) launches conv 1 | 2 and returns the launcher's code;
// *taken = false: conv1's shape is not covered (-2) and nothing has been launched.
template <class F>
int xl_pair(const Stage& g, const Chain& c, int r, int mi, const float* xr, const void* w1, const void* w2, F run, const char* what, bool* taken) {
    const cmtts_vocoder* v = g.v;
    const bool lastm = mi == 2;
    ConvXlArgs xa;
    memset(&xa, 0, sizeof(xa));
    xa.x = xr; xa.y = c.bT; xa.wf = (const float*)w1; xa.bias = v->c1[r][mi].bias;
    xa.bstride = g.cs; xa.B = g.B; xa.C = g.co; xa.T = g.To; xa.ld = g.To; xa.k = v->rb_kernel[c.j]; xa.dil = v->rb_dil[mi]; xa.slope = 0.1f;
    const int rc1 = run(xa, 1);
    if (rc1 == -3) return fail(CMTTS_E_HIP, what);
    *taken = rc1 == 0;
    if (!*taken) return 0;
    if (lastm) CHK(c.before_sum());      // between conv1 and conv2: conv1 of chain j overlaps chain j - 1
    // the residual operand is read at the positions this launch writes when y == res (in place: safe, every output element
    // reads only its own residual); the INPUT must not alias the output
    xa.x = c.bT; xa.y = lastm ? c.bufS : c.bR; xa.wf = (const float*)w2; xa.bias = v->c2[r][mi].bias;      // two-launch forms always write bR
    xa.res = xr; xa.dil = 1; xa.accum = lastm && c.j > 0;
    if (run(xa, 2) != 0) return fail(CMTTS_E_HIP, what);
    if (lastm) CHK(c.after_sum());
    return 0;
}

// One generic conv of a pair at the handle's precision.  bf16 / fp16: xt — conv1's output, conv2's input — crosses HBM as
// convert(leaky_relu(xt)) in 16 bits; fp16x3: fp32 xt in HBM, operands split into hi + lo fp16 while staged.
int conv_at_precision(const cmtts_vocoder* v, ConvArgs& a, const void* w16, bool writes_xt, int B, hipStream_t q) {
    const int p = v->precision;
    if (!p) return launch(a, EPI_PLAIN, B, q);
    if (p != 3 && writes_xt) { a.y16 = 1; a.y16_slope = 0.1f; }
    if (p != 3 && !writes_xt) a.x16 = 1;
    if (cmtts_launch_conv16(&a, w16, p, B, (void*)q) != 0) return fail(CMTTS_E_HIP, "conv16 launch failed");
    return 0;
}

// One pair as two launches of the generic kernels (conv_mfma.hip / conv_mfma16.hip): covers every shape
int generic_pair(const Stage& g, const Chain& c, int r, int mi, const float* xr, const void* w1, const void* w2) {
    const cmtts_vocoder* v = g.v;
    const int rk = v->rb_kernel[c.j], dil = v->rb_dil[mi], To = g.To;
    const bool lastm = mi == 2;
    ConvArgs a = conv_args(v->c1[r][mi], xr, To, To, g.cs, c.bT, To, g.cs, To);
    a.dil = dil; a.pad = (rk * dil - dil) / 2; a.pre_slope = 0.1f;
    CHK(conv_at_precision(v, a, w1, true, g.B, c.q));
    if (lastm) CHK(c.before_sum());      // between conv1 and conv2: conv1 of chain j overlaps chain j - 1
    ConvArgs b = conv_args(v->c2[r][mi], c.bT, To, To, g.cs, lastm ? c.bufS : c.bR, To, g.cs, To);      // two-launch forms always write bR
    b.pre_slope = 0.1f;
    b.out[0].res = xr; b.out[0].r_zs0 = g.cs; b.out[0].ldr = To;
    b.out[0].accum = lastm && c.j > 0;
    CHK(conv_at_precision(v, b, w2, false, g.B, c.q));
    if (lastm) CHK(c.after_sum());
    return 0;
}

// ResBlock j of stage i (hifigan/models.py:96-103) on chain c: bufS (+)= resblock(x).  Returns as soon as a form has taken the ResBlock.
int resblock(const Stage& g, const Chain& c) {
    const cmtts_vocoder* v = g.v;
    const int r = g.i * 3 + c.j, rk = v->rb_kernel[c.j], co = g.co, p = v->precision;
    const bool mode16 = p == 1 || p == 2;
    const void *w1[3], *w2[3];      // the direct-form fragments at the handle's precision
    for (int mi = 0; mi < 3; ++mi) {
        w1[mi] = p ? v->c1f[r][mi][p - 1] : (const void*)v->c1f32[r][mi];
        w2[mi] = p ? v->c2f[r][mi][p - 1] : (const void*)v->c2f32[r][mi];
    }

    // 1. narrow stages, 16-bit operands: the WHOLE ResBlock (three pairs) in one launch — x in, MRF sum out: 2 tensor passes instead of 6
    // (resblock16_kernel; bitwise equal to three pair launches).  Measured per ResBlock (bf16, 32 x 512 frames): C = 32: 0.51 / 0.83 / 1.10 ms
    // (k = 3 / 7 / 11) against 1.21 / 1.30 / 1.40 for three pair launches; C = 64 (8 waves, one 118-KB workgroup per CU): 0.76 / 1.31 / 1.91
    // against 1.15 / 1.40 / 1.66 — at k = 11 the halo recompute (+45 % MFMAs) costs more than the four tensor passes saved (voc_rb16 = 2: always)
    const bool rb_pays = co == 32 || rk <= 7 || g_voc_rb16 == 2;
    if (g_voc_rb16 && rb_pays && mode16 && co <= 64 && w1[0]) {
        const float *bb1[3], *bb2[3];
        for (int mi = 0; mi < 3; ++mi) { bb1[mi] = v->c1[r][mi].bias; bb2[mi] = v->c2[r][mi].bias; }
        CHK(c.before_sum());
        const int rc = cmtts_launch_resblock16(g.x, c.bufS, w1, w2, bb1, bb2, g.cs, g.B, co, g.To, g.To, rk, c.j > 0, 0.1f, p, (void*)c.q);
        if (rc == -3) return fail(CMTTS_E_HIP, "resblock16 launch failed");
        if (rc == 0) return c.after_sum();
        // -2 (shape not covered) is ignored: the pair forms below
    }

    // fp32, C = 64, k >= 7, chip-filling launches: the pair as two Winograd launches (conv_xlw_kernel<64>: one wave per workgroup with both m-tiles, eight workgroups
    // per CU) instead of the fused pair kernel — 10 / 15 products per output pair instead of 14 / 22 outweigh xt's trip through HBM (k = 11: 2 x 1225 against 3217 us;
    // k = 7: -0.3 ms per batch).  xw64 takes these ResBlocks off the pair kernels and into the fp32 X-resident chain of form 4.
    const bool xw64 = g_voc_wino64 && g_voc_wino && v->winograd && !p && co == 64 && rk >= g_voc_wino64_k && v->c1w32[r][0] && v->c2w32[r][0] &&
                      (g_voc_wino == 2 || g.big_launch);

    // 2. fp32, k = 3 pairs at C = 64 / 128 with both convs in the F(4,3) form and xt kept on the CU (conv_xlq_pair.hip): at C = 128 the two conv_xlq launches of form 4
    // without xt's trip through HBM and the residual's second read (five tensor passes -> two; the same products on quads one frame apart: fp32 Winograd rounding
    // between the two); at C = 64 half the MFMAs of the direct pair kernel.  64.4 -> 62.9 ms per 32 x 512-frame batch
    // (known slip, kept: g_voc_wino43 is tested for any non-zero value, so voc_wino43 = 2 also takes the dilation 3 / 5 pairs in this form)
    bool qpair = g_voc_qpair && g_voc_wino && g_voc_wino43 && v->winograd && !p && rk == 3 && (co == 64 || co == 128) &&
                 (g_voc_qpair == 2 || g_voc_wino == 2 || g.big_launch);
    for (int mi = 0; mi < 3 && qpair; ++mi) qpair = v->c1q32[r][mi] && v->c2q32[r][mi];
    if (qpair) {
        const void *q1[3], *q2[3];
        for (int mi = 0; mi < 3; ++mi) { q1[mi] = v->c1q32[r][mi]; q2[mi] = v->c2q32[r][mi]; }
        return pair_chain(g, c, r, q1, q2, cmtts_launch_conv_xlq_pair, "conv_xlq_pair launch failed", nullptr);
    }

    // 3. conv1 -> LeakyReLU -> conv2 -> + x of a pair in ONE launch, xt never leaves the CU: fp32 at C <= 64 (resblock_pair.hip); 16-bit at C <= 64
    // (resblock_pair16.hip: with the weight ring issued by hand the pair kernel wins for every (C, k): 0.37-0.55 ms per pair against 0.60-0.64 for two
    // launches, profiles/r02_vocoder_bf16.md) and at C = 128 with a single in-place image (resblock_pairw16.hip: 81 KB, two workgroups per CU, 2 x 4
    // tiles per wave; 379.8 us per k = 3 pair against 527 for two conv_xl16 launches); fp16x3 at C <= 128 with (hi, lo) images (resblock_pair16x3.hip)
    const bool pairw = g_voc_pairw && co == 128 && mode16;
    const bool pair3 = g_voc_pair3 && p == 3 && co <= 128;
    if (g_voc_pair && !xw64 && (co <= 64 || pairw || pair3) && (p != 3 || pair3) && w1[0]) {
        auto launch_pair = [&](const PairArgs* pa, void* q) {
            if (!p) return cmtts_launch_resblock_pair(pa, q);
            if (pair3) return cmtts_launch_resblock_pair16x3(pa, q);
            return pairw ? cmtts_launch_resblock_pairw16(pa, p, q) : cmtts_launch_resblock_pair16(pa, p, q);
        };
        bool declined = false;
        CHK(pair_chain(g, c, r, w1, w2, launch_pair, "resblock_pair launch failed", &declined));
        if (!declined) return 0;      // declined: this (C, k, dilation) is not covered by the pair kernels — per conv below
    }

    // 4. per conv: ResBlock.forward pair by pair, each on the first kernel that covers it
    const float* xr = g.x;
    for (int mi = 0; mi < 3; ++mi) {
        const int dil = v->rb_dil[mi];
        bool taken = false;
        if (g_voc_xl && !p && (co >= 128 || xw64) && w1[mi]) {
            // fp32, wide stages: X-resident single convs.  Winograd form of both convs (conv_xlw_kernel: 4 / 10 / 15 products per output pair instead of 6 / 14 / 22);
            // F(4,3) (conv_xlq_kernel: 6 / 16 / 24 products per quad of outputs where the F(2,3) tap groups take 8 / 20 / 30) for every conv2 (dilation 1) and for
            // conv1 at dilation 1, at dilation 3 everywhere and at dilation 5 only at C = 256 or k = 3: the five-class tiles of C = 128 / 64 (one workgroup fewer
            // per CU, 15 of 16 quad lanes, strided stores) are slower than the F(2,3) pair tiles at k = 7 / 11 — 3.63 vs 2.44 ms at C = 128, k = 11 (voc_wino43 = 3
            // forces them for tests).  A launcher's -2 (launch too small or shape not covered) falls back F(4,3) -> F(2,3) -> direct.
            const bool xw = g_voc_wino && v->winograd && v->c1w32[r][mi] && v->c2w32[r][mi];
            const bool q1 = xw && g_voc_wino43 && (dil == 1 || (g_voc_wino43 == 1 && (co == 256 || dil == 3 || rk == 3)) || g_voc_wino43 == 3) && v->c1q32[r][mi];
            bool xw1 = false;      // conv1 ran in a Winograd form: conv2 follows it
            auto run = [&](ConvXlArgs& xa, int which) {
                xa.wino_force = g_voc_wino == 2 || v->batch_invariant;
                int rc = -2;
                if (which == 1) {
                    if (q1) { xa.wf = v->c1q32[r][mi]; rc = cmtts_launch_conv_xlq(&xa, (void*)c.q); }
                    if (rc == -2 && xw) { xa.wf = v->c1w32[r][mi]; rc = cmtts_launch_conv_xlw(&xa, (void*)c.q); }
                    xw1 = rc == 0;
                    if (rc == -2) { xa.wf = v->c1f32[r][mi]; rc = cmtts_launch_conv_xl(&xa, (void*)c.q); }      // -2 again: not taken, the generic pair below
                    return rc;
                }
                if (xw1 && g_voc_wino43 && v->c2q32[r][mi]) { xa.wf = v->c2q32[r][mi]; rc = cmtts_launch_conv_xlq(&xa, (void*)c.q); }
                if (rc == -2 && xw1) { xa.wf = v->c2w32[r][mi]; rc = cmtts_launch_conv_xlw(&xa, (void*)c.q); }
                else if (rc == -2) { xa.wf = v->c2f32[r][mi]; rc = cmtts_launch_conv_xl(&xa, (void*)c.q); }
                return rc;
            };
            CHK(xl_pair(g, c, r, mi, xr, w1[mi], w2[mi], run, "conv_xl launch failed", &taken));
        } else if (g_voc_xl16 && mode16 && co >= 128 && w1[mi]) {
            // 16-bit, wide stages: X-resident single convs (conv_xl16_kernel); xt crosses HBM in 16 bits
            auto run = [&](ConvXlArgs& xa, int which) { return cmtts_launch_conv_xl16(&xa, p, which, (void*)c.q); };
            CHK(xl_pair(g, c, r, mi, xr, w1[mi], w2[mi], run, "conv_xl16 launch failed", &taken));
        } else if (g_voc_pair3 && p == 3 && co == 256 && w1[mi]) {
            // fp16x3, C = 256: X-resident single convs with (hi, lo) images (conv_xl16x3_kernel); xt crosses HBM in fp32
            auto run = [&](ConvXlArgs& xa, int) { return cmtts_launch_conv_xl16x3(&xa, (void*)c.q); };
            CHK(xl_pair(g, c, r, mi, xr, w1[mi], w2[mi], run, "conv_xl16x3 launch failed", &taken));
        }
        if (!taken) CHK(generic_pair(g, c, r, mi, xr, w1[mi], w2[mi]));
        xr = c.bR;
    }
    return 0;
}

size_t stage_buffer_floats(int B, int T) { return (size_t)B * T * 8192; }      // B * max_i(C_i * T_i): C_i * T_i = T * {512, 2048, 8192, 8192, 8192}

// The generator up to (not including) its last layer (hifigan/models.py:150-160): mel_ct [B,80,T] -> the last MRF sum [B][ch][Ti], Ti = 256 T
// (*x_out, still to be divided by the ResBlock count), in the workspace of cmtts_vocoder_workspace_bytes(v, B, T).
// Shared by cmtts_vocoder_forward (whole mels) and the two window entry points (a batch of mel windows).
int vocoder_generator(const cmtts_vocoder* v, const float* mel_ct, int B, int T, void* ws, hipStream_t s, const float** x_out, int* ch_out, int* Ti_out) {
    Carver cv(ws);
    const size_t nbuf = stage_buffer_floats(B, T);
    float* x = cv.take<float>(nbuf);        // stage input
    float* bufU = cv.take<float>(nbuf);     // upsampled
    float* bufT = cv.take<float>(nbuf);     // xt
    float* bufR = cv.take<float>(nbuf);     // running residual inside a ResBlock
    float* xs = cv.take<float>(nbuf);       // MRF sum
    // side streams only for small batches, and only if both could be had; otherwise everything runs in line on s and no further buffers are carved
    SideStream* ss = (long)B * T <= VOC_PAR_FRAMES ? side_for(s) : nullptr;
    if (ss && !side2_ready(ss)) ss = nullptr;
    Chain chain[3] = {{ss, 0, s, bufT, bufR, nullptr}, {ss, 1, s, bufT, bufR, nullptr}, {ss, 2, s, bufT, bufR, nullptr}};
    if (ss) {      // own xt / residual buffers and streams for the second and third ResBlock
        for (int j = 1; j < 3; ++j) { chain[j].bT = cv.take<float>(nbuf); chain[j].bR = cv.take<float>(nbuf); }
        chain[1].q = ss->side; chain[2].q = ss->side2;
    }
    CHK(launch(conv_args(v->conv_pre, mel_ct, T, T, (long)80 * T, x, T, (long)512 * T, T), EPI_PLAIN, B, s));      // x = conv_pre(x)
    int Ti = T, ch = 512;
    for (int i = 0; i < 4; ++i) {
        const int co = ch / 2, To = Ti * v->up_rate[i];
        CHK(upsample(v, i, x, bufU, B, ch, Ti, s));      // x = ups[i](leaky_relu(x))
        const Stage g = {v, i, B, co, To, (long)co * To, bufU, v->batch_invariant || (long)((To + 63) / 64) * B >= 1024};
        if (ss) {      // fork: the three chains see the upsampled input
            HIPCHK(hipEventRecord(ss->fork, s));
            HIPCHK(hipStreamWaitEvent(ss->side, ss->fork, 0));
            HIPCHK(hipStreamWaitEvent(ss->side2, ss->fork, 0));
        }
        for (int j = 0; j < 3; ++j) {      // xs (+)= resblocks[3 i + j](x)
            chain[j].bufS = xs;
            CHK(resblock(g, chain[j]));
        }
        if (ss) {      // join: the next stage (and conv_post) read the sum: chain 2's last conv is the last writer; chain 1 is
                       // ordered before it, but its stream must also be idle before its buffers are reused
            HIPCHK(hipEventRecord(ss->join, ss->side));
            HIPCHK(hipEventRecord(ss->join2, ss->side2));
            HIPCHK(hipStreamWaitEvent(s, ss->join, 0));
            HIPCHK(hipStreamWaitEvent(s, ss->join2, 0));
        }
        std::swap(x, xs);      // x = xs (/ num_kernels: folded into the next layer's pre_div)
        Ti = To; ch = co;
    }
    *x_out = x; *ch_out = ch; *Ti_out = Ti;
    return 0;
}

int hop_of(const cmtts_vocoder* v) { return v->up_rate[0] * v->up_rate[1] * v->up_rate[2] * v->up_rate[3]; }

// What the two window entry points share, all but their own check (own_bad: reported in its place among the argument checks) and their last layer
// (last_layer: its launch).  The window table is validated on the host before anything launches: a page-locked host table is read in place and copied
// into the workspace on `s` (no synchronisation; the caller keeps it unchanged until the call's work has completed), a device table is read back
// first, which synchronises `s`.  Then the windows are gathered into a batch and the generator runs on it.  A rejected call writes nothing.
template <class F>
int forward_windows(const char* who, cmtts_vocoder* v, const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, int core, const void* out,
                    const char* own_bad, void* ws, size_t ws_bytes, hipStream_t s, F last_layer) {
    auto bad_call = [who](int code, const char* what) { return fail(code, std::string(who) + ": " + what); };      // the message is built only when a check fails
    if (!v || !v->finalized) return fail(CMTTS_E_INVALID, "vocoder not finalized");
    if (!mel_ct || !windows || !out || !ws) return bad_call(CMTTS_E_INVALID, "null argument");
    if (B <= 0 || T <= 0 || N <= 0 || Tw <= 0 || core <= 0) return bad_call(CMTTS_E_INVALID, "B, T, N, Tw and core must be positive");
    if (Tw > T) return bad_call(CMTTS_E_INVALID, "Tw > T");
    if (own_bad) return bad_call(CMTTS_E_INVALID, own_bad);
    if (ws_bytes < cmtts_vocoder_windows_workspace_bytes(v, N, Tw)) return bad_call(CMTTS_E_WORKSPACE, "workspace too small");
    std::vector<StreamWindow> tab(N);
    bool on_host = false;
    CHK(fetch_table(who, windows, tab.data(), (size_t)N * sizeof(StreamWindow), s, &on_host));
    for (int n = 0; n < N; ++n) {
        const StreamWindow& w = tab[n];
        const char* bad = w.b < 0 || w.b >= B                                   ? "utterance outside [0, B)"
                          : w.start < 0 || (long)w.start + Tw > T              ? "window outside [0, T)"
                          : w.core_len <= 0 || w.core_len > core               ? "core_len outside [1, core]"
                          : w.core_off < 0 || (long)w.core_off + w.core_len > Tw ? "core_off + core_len > Tw"
                                                                                  : nullptr;
        if (bad) {
            char msg[200];
            snprintf(msg, sizeof msg, "%s: window %d (%d, %d, %d, %d): %s", who, n, w.b, w.start, w.core_off, w.core_len, bad);
            return fail(CMTTS_E_INVALID, msg);
        }
    }
    Carver cv(ws);
    float* mel_w = cv.take<float>((size_t)N * 80 * Tw);
    StreamWindow* win = cv.take<StreamWindow>(N);
    void* gws = cv.base + ((cv.off + 255) & ~(size_t)255);
    HIPCHK(hipMemcpyAsync(win, windows, (size_t)N * sizeof(StreamWindow), on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    if (cmtts_launch_mel_window_gather(mel_ct, 80, T, win, N, Tw, mel_w, (void*)s) != 0) return fail(CMTTS_E_HIP, "mel window gather launch failed");
    const float* x = nullptr;
    int ch = 0, Ti = 0;
    CHK(vocoder_generator(v, mel_w, N, Tw, gws, s, &x, &ch, &Ti));
    const int rc = last_layer(x, win, ch, Ti, hop_of(v));
    if (rc == -2) return bad_call(CMTTS_E_UNSUPPORTED, "conv_post kernel wider than 7");
    if (rc != 0) return fail(CMTTS_E_HIP, "conv_post windows launch failed");
    return 0;
}

}  // namespace

int fetch_table(const char* who, const void* table, void* host_copy, size_t bytes, hipStream_t s, bool* on_host) {
    hipPointerAttribute_t at{};
    const bool known = hipPointerGetAttributes(&at, table) == hipSuccess;
    if (!known) (void)hipGetLastError();
    *on_host = known && at.type == hipMemoryTypeHost;
    const bool on_dev = known && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeUnified);
    if (!*on_host && !on_dev) return fail(CMTTS_E_INVALID, std::string(who) + ": the table must be device or page-locked host memory");
    if (*on_host) {
        memcpy(host_copy, table, bytes);
    } else {
        HIPCHK(hipMemcpyAsync(host_copy, table, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}

int vocoder_internal_set(const char* name, int value, bool* found) {
    static const Knob tab[] = {
        {"voc_pair", &g_voc_pair, 0, 2}, {"voc_pair3", &g_voc_pair3, 0, 1}, {"voc_pairw", &g_voc_pairw, 0, 1}, {"voc_rb16", &g_voc_rb16, 0, 2},
        {"voc_xl", &g_voc_xl, 0, 1}, {"voc_xl16", &g_voc_xl16, 0, 1}, {"voc_upsT", &g_voc_upsT, 0, 1}, {"voc_wino", &g_voc_wino, 0, 2},
        {"voc_wino43", &g_voc_wino43, 0, 3}, {"voc_qpair", &g_voc_qpair, 0, 2}, {"voc_wino64", &g_voc_wino64, 0, 1}, {"voc_wino64_k", &g_voc_wino64_k, 3, 99},
        {"post_v4", &g_post_v4, 0, 1},             // conv_post with 16-byte loads (kernels.hip)
    };
    if (!strcmp(name, "voc_xl_split")) {           // conv_xl: m-tiles over several workgroups for launches of a few column tiles
        *found = true;
        return cmtts_xl_set_split(value);
    }
    return knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, found);
}

extern "C" {

int cmtts_vocoder_create(cmtts_vocoder** out) {
    if (!out) return fail(CMTTS_E_INVALID, "cmtts_vocoder_create: null argument");
    *out = new cmtts_vocoder();
    return 0;
}
int cmtts_vocoder_set_tensor(cmtts_vocoder* v, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    if (!v || v->finalized) return fail(CMTTS_E_INVALID, "cmtts_vocoder_set_tensor: null or finalized");
    return set_tensor(v->host, name, host_data, shape, ndim);
}
int cmtts_vocoder_finalize(cmtts_vocoder* v) {
    if (!v || v->finalized) return fail(CMTTS_E_INVALID, "cmtts_vocoder_finalize: null or finalized");
    const int r = finalize_vocoder(v);
    if (r != 0) v->al.release();
    return r;
}
void cmtts_vocoder_destroy(cmtts_vocoder* v) {
    if (!v) return;
    v->al.release();
    delete v;
}

int cmtts_vocoder_set_precision(cmtts_vocoder* v, int mode) {
    if (!v || mode < 0 || mode > 3) return fail(CMTTS_E_INVALID, "cmtts_vocoder_set_precision: mode 0 (fp32), 1 (bf16), 2 (fp16) or 3 (fp16x3)");
    v->precision = mode;
    return 0;
}

// Per-handle NUMERICS choices: properties of a model, not of the process (the option tiers: cmtts_api.hip)
int cmtts_vocoder_set_option(cmtts_vocoder* v, const char* name, int value) {
    if (!v || !name) return fail(CMTTS_E_INVALID, "cmtts_vocoder_set_option: null argument");
    const Knob tab[] = {
        {"ups16", &v->ups16, 0, 1},                      // 16-bit modes: 16-bit operands in the upsamplers too (1) or fp32 upsamplers (0)
        {"winograd", &v->winograd, 0, 1},                // fp32 generator: the ResBlock convs of the C >= 128 stages in their Winograd form (default 1; 0 = the direct form)
        {"batch_invariant", &v->batch_invariant, 0, 1},  // fp32 generator: the large-launch forms at every launch size (default 0)
    };
    bool found;
    const int prev = knob_set(tab, sizeof(tab) / sizeof(tab[0]), name, value, &found);
    if (found) return prev;
    return fail(CMTTS_E_INVALID, "cmtts_vocoder_set_option: unknown option");
}

size_t cmtts_vocoder_workspace_bytes(const cmtts_vocoder* v, int B, int T) {
    (void)v;
    // five stage buffers + four more (xt / running residual of the second and third ResBlock) when the batch is small enough for the
    // three ResBlocks of a stage to run side by side (VOC_PAR_FRAMES)
    const int nb = (long)B * T <= VOC_PAR_FRAMES ? 9 : 5;
    return (size_t)nb * (stage_buffer_floats(B, T) * sizeof(float) + 256) + 256;
}

int cmtts_vocoder_forward(cmtts_vocoder* v, const float* mel_ct, int B, int T, float* wav, void* ws, size_t ws_bytes, void* stream) {
    if (!v || !v->finalized) return fail(CMTTS_E_INVALID, "vocoder not finalized");
    if (!mel_ct || !wav || !ws || B <= 0 || T <= 0) return fail(CMTTS_E_INVALID, "cmtts_vocoder_forward: bad argument");
    if (ws_bytes < cmtts_vocoder_workspace_bytes(v, B, T)) return fail(CMTTS_E_WORKSPACE, "vocoder workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const float* x = nullptr;
    int ch = 0, Ti = 0;
    CHK(vocoder_generator(v, mel_ct, B, T, ws, s, &x, &ch, &Ti));
    // x = leaky_relu(xs / 3) [slope 0.01] -> conv_post -> tanh (hifigan/models.py:161-163)
    k_conv_post(x, v->post_w, v->post_b, 3.0f, 0.01f, wav, B, ch, Ti, Ti, v->post_k, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- streaming: a batch of mel windows through the generator, the window cores out (stream_windows.hip)
int cmtts_vocoder_halo_frames(const cmtts_vocoder* v) {
    // output frame f depends on mel frames [f - H, f + H]: the samples of frame f propagated backwards through conv_post,
    // every MRF (widest ResBlock: a (conv1 dilation d, conv2) pair widens by (d + 1)(k - 1) / 2), every ConvTranspose1d and
    // conv_pre (config.HifiGanConfig.halo_frames walks the same chain)
    if (!v) return fail(CMTTS_E_INVALID, "cmtts_vocoder_halo_frames: null argument");
    const long hop = hop_of(v);
    const long f = 1L << 20;
    long lo = f * hop - v->post_k / 2, hi = (f + 1) * hop - 1 + v->post_k / 2;
    int w = 0;
    for (int j = 0; j < 3; ++j) w = std::max(w, (v->rb_dil[0] + v->rb_dil[1] + v->rb_dil[2] + 3) * (v->rb_kernel[j] - 1) / 2);
    for (int i = 3; i >= 0; --i) {
        const long u = v->up_rate[i], k = v->up_kernel[i], p = (k - u) / 2;
        lo -= w; hi += w;
        const long a = lo + p - (k - 1), b = hi + p;          // y[t] = sum over i u + j - p = t (j in [0, k)) of x[i] w[j]
        lo = a >= 0 ? (a + u - 1) / u : -((-a) / u);
        hi = b >= 0 ? b / u : -((-b + u - 1) / u);
    }
    lo -= 3; hi += 3;                                          // conv_pre k = 7
    return (int)std::max(f - lo, hi - f);
}
size_t cmtts_vocoder_windows_workspace_bytes(const cmtts_vocoder* v, int N, int Tw) {
    if (N <= 0 || Tw <= 0) return 0;
    // the gathered windows [N][80][Tw] and the validated table [N][4], then the generator's workspace for (N, Tw)
    return (((size_t)N * 80 * Tw * sizeof(float) + 255) & ~(size_t)255) + (((size_t)N * sizeof(StreamWindow) + 255) & ~(size_t)255) +
           cmtts_vocoder_workspace_bytes(v, N, Tw);
}
int cmtts_vocoder_forward_windows(cmtts_vocoder* v, const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, int core,
                                  int16_t* pcm, float max_wav_value, void* ws, size_t ws_bytes, void* stream) {
    const char* own_bad = max_wav_value > 0.f && max_wav_value <= 32768.f ? nullptr : "max_wav_value outside (0, 32768]";
    return forward_windows("cmtts_vocoder_forward_windows", v, mel_ct, B, T, windows, N, Tw, core, pcm, own_bad, ws, ws_bytes, (hipStream_t)stream,
                           [&](const float* x, const StreamWindow* win, int ch, int Ti, int hop) {
        // x = leaky_relu(xs / 3) [slope 0.01] -> conv_post -> tanh -> int16, core columns only
        return cmtts_launch_conv_post_windows(x, v->post_w, v->post_b, 3.0f, 0.01f, win, N, ch, Ti, Ti, v->post_k, hop, core, max_wav_value, pcm, stream);
    });
}
int cmtts_vocoder_forward_windows_f32(cmtts_vocoder* v, const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, int core,
                                      int margin_frames, float* wav_rows, void* ws, size_t ws_bytes, void* stream) {
    const char* own_bad = margin_frames < 0 || (Tw != T && (long)core + 2L * margin_frames > Tw)
                              ? "margin_frames outside [0, (Tw - core) / 2] of a window narrower than T" : nullptr;
    return forward_windows("cmtts_vocoder_forward_windows_f32", v, mel_ct, B, T, windows, N, Tw, core, wav_rows, own_bad, ws, ws_bytes, (hipStream_t)stream,
                           [&](const float* x, const StreamWindow* win, int ch, int Ti, int hop) {
        // x = leaky_relu(xs / 3) [slope 0.01] -> conv_post -> tanh, core and margin columns only, fp32
        return cmtts_launch_conv_post_windows_f32(x, v->post_w, v->post_b, 3.0f, 0.01f, win, N, ch, Ti, Ti, v->post_k, hop, core, margin_frames, wav_rows, stream);
    });
}

// internal_hooks.h
int cmtts_internal_mel_window_gather(const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, float* out, void* stream) {
    (void)B;
    if (!mel_ct || !windows || !out || N <= 0 || Tw <= 0 || Tw > T) return fail(CMTTS_E_INVALID, "cmtts_internal_mel_window_gather: bad argument");
    return cmtts_launch_mel_window_gather(mel_ct, 80, T, (const StreamWindow*)windows, N, Tw, out, stream) == 0 ? 0
                                                                                                              : fail(CMTTS_E_HIP, "gather launch failed");
}

}  // extern "C"
