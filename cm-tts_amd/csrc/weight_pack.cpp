// Host-only weight packers (weight_pack.h).  The layout comments are the specification the kernels are written against; the lane maps
// and the Winograd weight transforms are each written once below, and a packer is its kernel's loop nest over them.
#include "weight_pack.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/cmtts_hip.h"
#include "internal_hooks.h"
#include "resblock_pair.h"

namespace {

// Taps tau .. tau + 2 of a k-major array as [K][M] planes; g(k, row)[i] is tap tau + i of that element in double, read only when a transform asks for it
struct Taps3 {
    const float* t[3];
    int M;
    Taps3 operator()(int k, int row) const { const size_t o = (size_t)k * M + row; return {{t[0] + o, t[1] + o, t[2] + o}, M}; }
    double operator[](int i) const { return (double)*t[i]; }
};
// P[tap][k][row] of a k-major array [taps][K][M]
struct KMajor {
    const float* p;
    int taps, K, M;
    std::vector<float> zeros;   // a tap beyond the kernel is a plane of zeros: made when the first group of three that overhangs the kernel asks for it
    KMajor(const std::vector<float>& w, int taps_, int K_, int M_) : p(w.data()), taps(taps_), K(K_), M(M_) {}
    float at(int tap, int k, int row) const { return p[((size_t)tap * K + k) * M + row]; }
    const float* plane(int tap) {
        if (tap < taps) return p + (size_t)tap * K * M;
        if (zeros.empty()) zeros.assign((size_t)K * M, 0.0f);
        return zeros.data();
    }
    Taps3 taps3(int tau) { return {{plane(tau), plane(tau + 1), plane(tau + 2)}, M}; }
};

// A operand of v_mfma_f32_32x32x2_f32: lane l supplies A[m = l & 31][k = l >> 5]; element j of a lane's vector is k-step j of its k-group
inline int k32(int base, int lane, int j) { return base + 2 * j + (lane >> 5); }
// A operand of v_mfma_f32_32x32x16_{bf16,f16}: lane l supplies A[m = l & 31][k = 8 (l >> 5) + j], j = 0 .. 7
inline int k32h(int base, int lane, int j) { return base + 8 * (lane >> 5) + j; }
inline int row32(int mt, int lane) { return 32 * mt + (lane & 31); }
// A operand of v_mfma_f32_16x16x4_f32: lane l supplies A[m = l & 15][k = l >> 4]; element i of a lane's vector is the i-th 16-row tile above `base`
inline int k16(int ks, int lane) { return 4 * ks + (lane >> 4); }
inline int row16(int base, int lane, int i) { return base + 16 * i + (lane & 15); }

// [M/32 m-tiles][64 lanes][E]: the 32-row fragments of the 2 E input channels from `base` for every m-tile, element = val(k, row); E = 4: fp32 (32x32x2), E = 8: 16-bit (32x32x16)
template <int E, class T, class V>
inline void emit32(T*& o, int M, int base, V val) {
    for (int mt = 0; mt < M / 32; ++mt)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < E; ++j) *o++ = val(E == 4 ? k32(base, lane, j) : k32h(base, lane, j), row32(mt, lane));
}
// The taps themselves as fragments, element = cvt(P[tap][k][row]): [K/chunk][taps][chunk/2E k-groups][M/32][64 lanes][E] — chunk = K is the tap-major order
// [taps][K/2E][..], chunk = 4 E the ITERATION order [K/4E][taps][2 halves][..] of the kernels whose K loop walks (chunk, tap, half)
template <int E, class T, class C>
std::vector<T> plain_fragments(const std::vector<float>& p, int taps, int K, int M, int chunk, C cvt) {
    std::vector<T> f((size_t)taps * K * M);
    KMajor P(p, taps, K, M);
    T* o = f.data();
    for (int c = 0; c < K / chunk; ++c)
        for (int tap = 0; tap < taps; ++tap)
            for (int g = 0; g < chunk / (2 * E); ++g) emit32<E>(o, M, chunk * c + 2 * E * g, [&](int k, int row) { return cvt(P.at(tap, k, row)); });
    return f;
}

// Winograd weight transforms of three taps, formed in double (the caller rounds to float once).
// F(2,3): G0 = g0, G1 = (g0 + g1 + g2) / 2, G2 = (g0 - g1 + g2) / 2, G3 = g2
inline double wino23_weight(int tr, const Taps3& g) {
    return tr == 0 ? g[0] : tr == 1 ? 0.5 * (g[0] + g[1] + g[2]) : tr == 2 ? 0.5 * (g[0] - g[1] + g[2]) : g[2];
}
// F(4,3) (points 0, +-1, +-2, inf): U0 = g0 / 4, U1 = -(g0 + g1 + g2) / 6, U2 = -(g0 - g1 + g2) / 6, U3 = g0 / 24 + g1 / 12 + g2 / 6,
// U4 = g0 / 24 - g1 / 12 + g2 / 6, U5 = g2
inline double wino43_weight(int tr, const Taps3& g) {
    switch (tr) {
        case 0: return g[0] / 4.0;
        case 1: return -(g[0] + g[1] + g[2]) / 6.0;
        case 2: return -(g[0] - g[1] + g[2]) / 6.0;
        case 3: return g[0] / 24.0 + g[1] / 12.0 + g[2] / 6.0;
        case 4: return g[0] / 24.0 - g[1] / 12.0 + g[2] / 6.0;
        default: return g[2];
    }
}

}  // namespace

// k-major packed weights [taps][K][M] -> MFMA A-fragment order [taps][K/8][M/32][64 lanes][4]:
// element (lane, j) of k-group g, m-tile mt is P[tap][8g + 2j + (lane >> 5)][32 mt + (lane & 31)], i.e. the A
// operand of v_mfma_f32_32x32x2_f32 for k-step j of that group (lane l supplies A[m = l & 31][k = l >> 5]).
std::vector<float> to_fragment_order(const std::vector<float>& p, int taps, int K, int M) {
    return plain_fragments<4, float>(p, taps, K, M, K, [](float v) { return v; });
}

// The same fragments in the ITERATION order of the fused ResBlock pair kernels (resblock_pair.hip): the K loop walks
// (16-channel chunk, tap, 8-channel half), so [K/16][taps][2][M/32][64 lanes][4] makes the weight stream one linear walk.
std::vector<float> to_fragment_iter_order(const std::vector<float>& p, int taps, int K, int M) {
    return plain_fragments<4, float>(p, taps, K, M, 16, [](float v) { return v; });
}

// Winograd F(2,3) form of a k = 3 conv for the persistent denoiser's WINO instances (denoiser_persist.hip): k-major packed weights
// [3][K][M] -> transformed weights G0 = g0, G1 = (g0 + g1 + g2) / 2, G2 = (g0 - g1 + g2) / 2, G3 = g2 (formed in double, rounded once) as MFMA
// A fragments [K/4 half-groups][M/32][2][64 lanes][4]: element q of fragment (hg, mt, ps) at lane l is transform 2 ps + (q >> 1) of
// input channel 4 hg + 2 (q & 1) + (l >> 5), output row 32 mt + (l & 31).  WINO_PAD_HG half-groups of zeros follow.
std::vector<float> to_wino_fragments(const std::vector<float>& p, int K, int M) {
    std::vector<float> f((size_t)4 * K * M + (size_t)WINO_PAD_HG * (M / 32) * 2 * 64 * 4, 0.0f);
    KMajor P(p, 3, K, M);
    const Taps3 g = P.taps3(0);
    float* o = f.data();
    for (int hg = 0; hg < K / 4; ++hg)
        for (int mt = 0; mt < M / 32; ++mt)
            for (int ps = 0; ps < 2; ++ps)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 4; ++q) *o++ = (float)wino23_weight(2 * ps + (q >> 1), g(k32(4 * hg, lane, q & 1), row32(mt, lane)));
    return f;
}

// Winograd form of a k-tap conv for conv_xlw_kernel (resblock_pair.h: WinoTab<KT>): the transformed weights of every table entry (formed in
// double, rounded once) as A fragments in the kernel's iteration order [K/16 chunks][entries][2 halves][M/32][64 lanes][4].
// wkind 0 .. 3 are the F(2,3) transforms of taps tau .. tau + 2; 4 = -g[tau], 5 = g[tau] + g[tau+1], 6 = g[tau+1] (F(2,2) and single-tap remainders).
static std::vector<float> wino_iter(const WinoEntry* tab, int n, const std::vector<float>& p, int taps, int K, int M) {
    std::vector<float> f((size_t)n * K * M);
    KMajor P(p, taps, K, M);
    float* o = f.data();
    for (int c = 0; c < K / 16; ++c)
        for (int e = 0; e < n; ++e)
            for (int h = 0; h < 2; ++h) {
                const int kind = tab[e].wkind;
                const Taps3 g3 = P.taps3(tab[e].tau);
                emit32<4>(o, M, 16 * c + 8 * h, [&](int k, int row) {
                    const Taps3 g = g3(k, row);
                    switch (kind) {
                        case 4: return (float)-g[0];
                        case 5: return (float)(g[0] + g[1]);
                        case 6: return (float)g[1];
                        default: return (float)wino23_weight(kind, g);
                    }
                });
            }
    return f;
}
std::vector<float> to_wino_iter_fragments(const std::vector<float>& p, int taps, int K, int M) {
    if (taps == 3) return wino_iter(WinoTab<3>::e, WinoTab<3>::N, p, taps, K, M);
    if (taps == 7) return wino_iter(WinoTab<7>::e, WinoTab<7>::N, p, taps, K, M);
    if (taps == 11) return wino_iter(WinoTab<11>::e, WinoTab<11>::N, p, taps, K, M);
    return {};
}

// F(4,3) form of a k-tap, dilation-1 conv for conv_xlq_kernel (conv_xlq.hip: QTab<KT>): per k-step of four input channels the transformed weights of
// every group of three taps (U0 = g0/4, U1 = -(g0+g1+g2)/6, U2 = -(g0-g1+g2)/6, U3 = g0/24 + g1/12 + g2/6, U4 = g0/24 - g1/12 + g2/6, U5 = g2; a tap beyond the
// kernel is zero) and, for k = 7, of the seventh tap on its own (g, g/2, g/2, g) — formed in double, rounded once — as A fragments of v_mfma_f32_16x16x4_f32 in
// the kernel's iteration order [K/4 k-steps][M/64 waves][points][64 lanes][4]: element i at lane l = input channel 4 ks + (l >> 4), output row 64 w + 16 i + (l & 15).
// pad_ks k-steps of zeros follow.
static std::vector<float> wino43_iter(const std::vector<float>& p, int taps, int K, int M, int pad_ks) {
    if ((taps != 3 && taps != 5 && taps != 7 && taps != 11) || K % 4 || M % 64) return {};
    const int ngrp = taps == 3 ? 1 : taps <= 7 ? 2 : 4, npt = ngrp * 6 + (taps == 7 ? 4 : 0), NWV = M / 64;
    std::vector<float> f((size_t)(K / 4 + pad_ks) * NWV * npt * 256, 0.0f);
    KMajor P(p, taps, K, M);
    float* o = f.data();
    for (int ks = 0; ks < K / 4; ++ks)
        for (int w = 0; w < NWV; ++w)
            for (int pt = 0; pt < npt; ++pt) {
                const int q = pt - ngrp * 6;                 // >= 0: point q of k = 7's seventh tap
                const Taps3 g = P.taps3(q < 0 ? 3 * (pt / 6) : 6);
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 4; ++i) {
                        const Taps3 gi = g(k16(ks, lane), row16(64 * w, lane, i));
                        *o++ = (float)(q < 0 ? wino43_weight(pt % 6, gi) : (q == 1 || q == 2) ? 0.5 * gi[0] : gi[0]);
                    }
            }
    return f;
}
std::vector<float> to_wino43_iter_fragments(const std::vector<float>& p, int taps, int K, int M) { return wino43_iter(p, taps, K, M, 0); }

// Winograd F(4,3) form of the k = 3 conv for the persistent denoiser's WINO == 2 instances (points 0, +-1, +-2, inf): transformed weights
// U0 .. U5 as above (formed in double, rounded once) as A fragments of v_mfma_f32_16x16x4_f32 in the kernel's iteration order
// [K/4 k-steps][M/64 waves][6 transforms][64 lanes][4]: element e at lane l is input channel 4 ks + (l >> 4), output row 64 w + 16 e + (l & 15) —
// the k = 3 stream of to_wino43_iter_fragments with WINO43_PAD_KS k-steps of zeros behind it.
std::vector<float> to_wino43_fragments(const std::vector<float>& p, int K, int M) { return wino43_iter(p, 3, K, M, WINO43_PAD_KS); }

// The FFT blocks' k = 9 FFN conv as three Winograd tap groups for conv_xres.hip, NT transforms per group, as A fragments of v_mfma_f32_16x16x4_f32 in the kernel's
// iteration order [K/4 k-steps][M/32 m-tiles][3 NT / 2][64 lanes][4]: with pt = NT * group + transform, vector pt / 2 of a (k-step, m-tile) holds points pt and pt + 1 for
// the m-tile's two 16-row halves — element (pt & 1) * 2 + i at lane l = input channel 4 ks + (l >> 4), output row 32 mt + 16 i + (l & 15).
template <int NT>
static std::vector<float> xres_fragments(const std::vector<float>& p, int taps, int K, int M) {
    if (taps != 9 || K % 4 || M % 32) return {};
    const int MTn = M / 32, npt = 3 * NT;
    std::vector<float> f((size_t)(K / 4) * MTn * npt * 128);
    KMajor P(p, taps, K, M);
    for (int ks = 0; ks < K / 4; ++ks)
        for (int mt = 0; mt < MTn; ++mt)
            for (int pt = 0; pt < npt; ++pt) {
                const Taps3 g = P.taps3(3 * (pt / NT));
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 2; ++i) {
                        const Taps3 gi = g(k16(ks, lane), row16(32 * mt, lane, i));
                        f[((((size_t)ks * MTn + mt) * (npt / 2) + pt / 2) * 64 + lane) * 4 + (pt & 1) * 2 + i] = (float)(NT == 6 ? wino43_weight(pt % NT, gi) : wino23_weight(pt % NT, gi));
                    }
            }
    return f;
}
// F(4,3) over output quads (conv_xres_kernel<.., WQ = true>): six transforms per group (U0 .. U5 as in to_wino43_fragments), [K/4][M/32][9][64 lanes][4]
std::vector<float> to_wino43_xres_fragments(const std::vector<float>& p, int taps, int K, int M) { return xres_fragments<6>(p, taps, K, M); }
// F(2,3) over output PAIRS (WQ == 2 instances; round 6): the four transformed weights U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 per group,
// [K/4][M/32][3][2][64 lanes][4]: element (tr & 1) * 2 + i of vector tr / 2 of group g at lane l = transform tr
std::vector<float> to_wino23_xres_fragments(const std::vector<float>& p, int taps, int K, int M) { return xres_fragments<4>(p, taps, K, M); }

unsigned short host_cvt16(float f, int mode) {   // mode 1 = bf16 (round to nearest even), 2 = fp16
    if (mode == 1) {
        unsigned u;
        memcpy(&u, &f, 4);
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    const _Float16 h = (_Float16)f;
    unsigned short r;
    memcpy(&r, &h, 2);
    return r;
}

// k-major packed weights [taps][K][M] -> 16-bit MFMA A-fragment order for v_mfma_f32_32x32x16_{bf16,f16}:
// [taps][K/16][M/32][64 lanes][8]: element (lane, j) = P[tap][16g + 8 (lane >> 5) + j][32 mt + (lane & 31)].
std::vector<unsigned short> to_fragment16(const std::vector<float>& p, int taps, int K, int M, int mode) {
    return plain_fragments<8, unsigned short>(p, taps, K, M, K, [mode](float v) { return host_cvt16(v, mode); });
}

// The same fragments in the ITERATION order of conv_mfma16.hip's deep-ring variant: its K loop walks (32-channel chunk, tap,
// k-group of the chunk), so [K/32][taps][2][M/32][64 lanes][8] makes the weight stream one linear walk (K % 32 == 0).
std::vector<unsigned short> to_fragment16_iter(const std::vector<float>& p, int taps, int K, int M, int mode) {
    return plain_fragments<8, unsigned short>(p, taps, K, M, 32, [mode](float v) { return host_cvt16(v, mode); });
}

// fp16x3 operands: every weight as hi = fp16(w) and lo = fp16(w - hi); the lo fragment set follows the hi set
std::vector<unsigned short> to_fragment16_split(const std::vector<float>& p, int taps, int K, int M) {
    std::vector<float> hi(p.size()), lo(p.size());
    for (size_t i = 0; i < p.size(); ++i) {
        const _Float16 h = (_Float16)p[i];
        hi[i] = (float)h;
        lo[i] = p[i] - (float)h;
    }
    std::vector<unsigned short> f = to_fragment16(hi, taps, K, M, 2);
    const std::vector<unsigned short> fl = to_fragment16(lo, taps, K, M, 2);
    f.insert(f.end(), fl.begin(), fl.end());
    return f;
}

// The speaker encoder's Conv2D (speaker_encoder.hip: conv2d_mfma_kernel) contracts over k = tap * K + input channel in chunks of 16: A fragments of
// v_mfma_f32_16x16x4_f32 as [ceil(taps K / 16) chunks][M/16 m-tiles][64 lanes][4]: element j at lane l is k = 16 chunk + 4 (l >> 4) + j, output row 16 mt + (l & 15)
// — MFMA j of a chunk sums k = 16 chunk + 4 kk + j over its four lane groups kk, so that a lane's four elements are one 16-byte load on the activation side too
// (four consecutive channels of one pixel).  k beyond taps K is zero.  The row's scale enters in double, one rounding.
std::vector<float> to_conv2d_fragments(const std::vector<float>& p, int taps, int K, int M, const double* scale) {
    if (taps < 1 || K < 1 || M < 16 || M % 16) return {};
    const int ktot = taps * K, nchunk = (ktot + 15) / 16;
    std::vector<float> f((size_t)nchunk * M * 16);
    float* o = f.data();
    for (int c = 0; c < nchunk; ++c)
        for (int mt = 0; mt < M / 16; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int k = 16 * c + 4 * (lane >> 4) + j, row = 16 * mt + (lane & 15);
                    const double w = k < ktot ? (double)p[(size_t)k * M + row] : 0.0;
                    *o++ = (float)(scale ? w * scale[row] : w);
                }
    return f;
}

std::vector<float> pack_conv2d_bn(const std::vector<float>& p, int taps, int K, int M, const float* bias, const float* bn, std::vector<float>* bias_out) {
    std::vector<double> s((size_t)M, 1.0);
    bias_out->assign((size_t)M, 0.0f);
    for (int r = 0; r < M; ++r) {
        double b = bias ? (double)bias[r] : 0.0;
        if (bn) {
            s[r] = (double)bn[r] / sqrt((double)bn[3 * (size_t)M + r] + 1e-3);
            b = (b - (double)bn[2 * (size_t)M + r]) * s[r] + (double)bn[(size_t)M + r];
        }
        (*bias_out)[r] = (float)b;
    }
    return to_conv2d_fragments(p, taps, K, M, s.data());
}

// The GE2E encoder's LSTM matrices (ge2e.hip: W_ih for the projection GEMM, W_hh for the recurrence): p = the PyTorch matrix [4 H gate rows][K] handed
// over k-major [K][M = 1024], gate rows in torch's order i, f, g, o (row = gate * 256 + unit).  A fragments of v_mfma_f32_16x16x4_f32 as
// [ceil(K / 16) chunks][64 row tiles][64 lanes][4] like to_conv2d_fragments, over PACKED rows q = 64 (unit / 16) + 16 gate + unit % 16: the row tiles
// 4 g .. 4 g + 3 are i, f, g, o of hidden units 16 g .. 16 g + 15, so the wave that owns them holds all four gates of a unit in one lane.
int lstm_packed_row(int q) { return ((q % 64) / 16) * 256 + 16 * (q / 64) + q % 16; }

std::vector<float> to_lstm_fragments(const std::vector<float>& p, int K, int M) {
    if (K < 1 || M != 1024) return {};
    const int nchunk = (K + 15) / 16;
    std::vector<float> f((size_t)nchunk * M * 16);
    float* o = f.data();
    for (int c = 0; c < nchunk; ++c)
        for (int rt = 0; rt < M / 16; ++rt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int k = 16 * c + 4 * (lane >> 4) + j, row = lstm_packed_row(16 * rt + (lane & 15));
                    *o++ = k < K ? p[(size_t)k * M + row] : 0.0f;
                }
    return f;
}

// internal_hooks.h: the speaker encoder's packer with its BatchNorm fold, host memory only
extern "C" int cmtts_internal_spkenc_pack(const float* kernel, int taps, int cin, int cout, const float* bias, const float* bn, float* frag,
                                          size_t frag_floats, float* bias_out, size_t* need) {
    if (!kernel || !need || taps < 1 || cin < 1 || cout < 16 || cout % 16) return CMTTS_E_INVALID;
    *need = (size_t)((taps * cin + 15) / 16) * cout * 16;
    if (!frag) return 0;
    if (frag_floats < *need || !bias_out) return CMTTS_E_INVALID;
    std::vector<float> b;
    const std::vector<float> f = pack_conv2d_bn(std::vector<float>(kernel, kernel + (size_t)taps * cin * cout), taps, cin, cout, bias, bn, &b);
    memcpy(frag, f.data(), f.size() * sizeof(float));
    memcpy(bias_out, b.data(), b.size() * sizeof(float));
    return 0;
}

// internal_hooks.h: every packer by name, host memory only
extern "C" int cmtts_internal_pack_weights(const char* layout, const float* kmajor, int taps, int K, int M, int mode, void* out, size_t out_bytes,
                                           size_t* need) {
    if (!layout || !kmajor || !need || taps < 1 || K < 1 || M < 1) return CMTTS_E_INVALID;
    const std::string name = layout;
    const std::vector<float> p(kmajor, kmajor + (size_t)taps * K * M);
    const bool m16 = mode == 1 || mode == 2;
    std::vector<float> f;
    std::vector<unsigned short> h;
    if (name == "fragment_order" && K % 8 == 0 && M % 32 == 0) f = to_fragment_order(p, taps, K, M);
    else if (name == "fragment_iter_order" && K % 16 == 0 && M % 32 == 0) f = to_fragment_iter_order(p, taps, K, M);
    else if (name == "wino_fragments" && taps == 3 && K % 4 == 0 && M % 32 == 0) f = to_wino_fragments(p, K, M);
    else if (name == "wino_iter_fragments" && K % 16 == 0 && M % 32 == 0) f = to_wino_iter_fragments(p, taps, K, M);
    else if (name == "wino43_fragments" && taps == 3) f = to_wino43_fragments(p, K, M);
    else if (name == "wino43_iter_fragments") f = to_wino43_iter_fragments(p, taps, K, M);
    else if (name == "wino43_xres_fragments") f = to_wino43_xres_fragments(p, taps, K, M);
    else if (name == "wino23_xres_fragments") f = to_wino23_xres_fragments(p, taps, K, M);
    else if (name == "conv2d_fragments") f = to_conv2d_fragments(p, taps, K, M, nullptr);
    else if (name == "lstm_fragments" && taps == 1) f = to_lstm_fragments(p, K, M);
    else if (name == "fragment16" && m16 && K % 16 == 0 && M % 32 == 0) h = to_fragment16(p, taps, K, M, mode);
    else if (name == "fragment16_iter" && m16 && K % 32 == 0 && M % 32 == 0) h = to_fragment16_iter(p, taps, K, M, mode);
    else if (name == "fragment16_split" && K % 16 == 0 && M % 32 == 0) h = to_fragment16_split(p, taps, K, M);
    const void* src = f.empty() ? (const void*)h.data() : (const void*)f.data();
    const size_t bytes = f.empty() ? h.size() * sizeof(unsigned short) : f.size() * sizeof(float);
    if (!bytes) return CMTTS_E_INVALID;      // unknown layout or a shape the packer does not cover
    *need = bytes;
    if (!out) return 0;
    if (out_bytes < bytes) return CMTTS_E_INVALID;
    memcpy(out, src, bytes);
    return 0;
}
