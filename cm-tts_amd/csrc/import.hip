// Weight import of the C ABI (include/cmtts_hip.h): cmtts_set_tensor's host copies -> the k-major device arrays and the MFMA
// fragment streams (weight_pack.h) every kernel reads.  Runs once per handle, inside cmtts_finalize / cmtts_vocoder_finalize.
#include <math.h>
#include <string.h>

#include "model.h"
#include "weight_pack.h"
#include "cond_gemm.h"
#include "kernels.h"

// W [Cout][Cin][K] -> k-major [K][Cin][ld] with ld = round_up(Cout, 4); perm[p] = original row of packed row p
static std::vector<float> kmajor(const HostTensor& W, const std::vector<int>* perm) {
    const int Cout = (int)W.dim(0), Cin = (int)W.dim(1), K = (int)W.dim(2);
    const int ld = round_up(Cout, 4);
    std::vector<float> p((size_t)K * Cin * ld, 0.f);
    for (int k = 0; k < K; ++k)
        for (int ci = 0; ci < Cin; ++ci)
            for (int r = 0; r < Cout; ++r) {
                const int co = perm ? (*perm)[r] : r;
                p[((size_t)k * Cin + ci) * ld + r] = W.data[((size_t)co * Cin + ci) * K + k];
            }
    return p;
}

int pack_conv(Allocs& al, const HostTensor& W, const HostTensor* bias, const std::vector<int>* perm, PackedConv* out,
              std::vector<float>* host_copy) {
    const int Cout = (int)W.dim(0), Cin = (int)W.dim(1), K = (int)W.dim(2);
    const int ld = round_up(Cout, 4);
    std::vector<float> p = kmajor(W, perm);
    CHK(al.upload(p, &out->w));
    if (host_copy) host_copy->swap(p);
    out->bias = nullptr;
    if (bias) {
        std::vector<float> b(Cout);
        for (int r = 0; r < Cout; ++r) b[r] = bias->data[perm ? (*perm)[r] : r];
        CHK(al.upload(b, &out->bias));
    }
    out->cout = Cout; out->cin = Cin; out->taps = K; out->ld = ld;
    out->tap_stride = (long)Cin * ld;
    out->phase_stride = 0;
    return 0;
}

int set_tensor(std::map<std::string, HostTensor>& host, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!name || !data || ndim < 0 || ndim > 4) return fail(CMTTS_E_INVALID, "set_tensor: bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] <= 0) return fail(CMTTS_E_INVALID, std::string("set_tensor: bad shape for ") + name);
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(data, data + n);
    host[name] = std::move(t);
    return 0;
}

namespace {

// ConvTranspose1d W [Cin][Cout][K], stride s -> polyphase [s][K/s][Cin][ld]: phase r uses taps k = r + s*q
int pack_conv_transpose(Allocs& al, const HostTensor& W, const HostTensor& bias, int s, PackedConv* out,
                        std::vector<float>* two_tap = nullptr) {
    const int Cin = (int)W.dim(0), Cout = (int)W.dim(1), K = (int)W.dim(2);
    const int Q = K / s, ld = round_up(Cout, 4);
    if (two_tap && Q == 2) {   // the same weights as ONE two-tap conv with s * Cout stacked rows (row = phase * Cout + co): [2][Cin][s * Cout]
        two_tap->assign((size_t)2 * Cin * s * Cout, 0.f);
        for (int q = 0; q < 2; ++q)
            for (int ci = 0; ci < Cin; ++ci)
                for (int r = 0; r < s; ++r)
                    for (int co = 0; co < Cout; ++co)
                        (*two_tap)[((size_t)q * Cin + ci) * s * Cout + (size_t)r * Cout + co] = W.data[((size_t)ci * Cout + co) * K + (r + s * q)];
    }
    std::vector<float> p((size_t)s * Q * Cin * ld, 0.f);
    for (int r = 0; r < s; ++r)
        for (int q = 0; q < Q; ++q)
            for (int ci = 0; ci < Cin; ++ci)
                for (int co = 0; co < Cout; ++co)
                    p[(((size_t)r * Q + q) * Cin + ci) * ld + co] = W.data[((size_t)ci * Cout + co) * K + (r + s * q)];
    CHK(al.upload(p, &out->w));
    CHK(al.upload(bias.data, &out->bias));
    out->cout = Cout; out->cin = Cin; out->taps = Q; out->ld = ld;
    out->tap_stride = (long)Cin * ld;
    out->phase_stride = (long)Q * Cin * ld;
    return 0;
}

// nn.Linear weight [N][K] -> transposed [K][N] (dense_small operand / X operand of a GEMM)
std::vector<float> transpose2d(const float* w, int N, int K) {
    std::vector<float> t((size_t)K * N);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) t[(size_t)k * N + n] = w[(size_t)n * K + k];
    return t;
}

std::vector<float> omega_table(int C) {
    // SinusoidalPositionalEmbedding.get_embedding (model/blocks.py:50-54): exp(arange(half) * -ln(1e4)/(half-1)) in fp32
    const int half = C / 2;
    const float e = (float)(log(10000.0) / (half - 1));
    std::vector<float> w(half);
    for (int j = 0; j < half; ++j) w[j] = (float)exp((double)((float)j * -e));
    return w;
}

// Sinusoid table rows 0..rows-1 (row 0 = padding = zeros): fp32 argument p*w_j, sine/cosine in f64 rounded to
// fp32 — the same recipe the kernels use on the fly beyond the table.
std::vector<float> pe_table(int C, int rows) {
    const std::vector<float> w = omega_table(C);
    const int half = C / 2;
    std::vector<float> t((size_t)rows * C, 0.f);
    for (int p = 1; p < rows; ++p)
        for (int c = 0; c < C; ++c) {
            const float arg = (float)p * w[c < half ? c : c - half];
            t[(size_t)p * C + c] = c < half ? (float)sin((double)arg) : (float)cos((double)arg);
        }
    return t;
}

struct Getter {
    const std::map<std::string, HostTensor>& host;
    std::string missing;
    const HostTensor* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = host.find(name);
        if (it == host.end()) {
            if (missing.empty()) missing = "missing tensor " + name;
            return nullptr;
        }
        if (it->second.shape != std::vector<int64_t>(shape)) {
            if (missing.empty()) missing = "wrong shape for tensor " + name;
            return nullptr;
        }
        return &it->second;
    }
};

// 16-bit fragment-order copies of a k-major array [taps][K][M] (weight_pack.h): dst[0] bf16, dst[1] fp16 and, with n = 3, dst[2] fp16x3 (hi | lo)
int upload16(Allocs& al, const std::vector<float>& hp, int taps, int K, int M, void** dst, int n) {
    for (int i = 0; i < n; ++i) {
        const std::vector<unsigned short> f = i < 2 ? to_fragment16(hp, taps, K, M, i + 1) : to_fragment16_split(hp, taps, K, M);
        CHK(al.upload_bytes(f.data(), f.size() * 2, &dst[i]));
    }
    return 0;
}

#define GET(var, name, ...)                                     \
    const HostTensor* var = g.get(name, {__VA_ARGS__});          \
    if (!var) return fail(CMTTS_E_INVALID, g.missing)
#define UP(dst, t) CHK(al.upload((t)->data, &(dst)))

}  // namespace

int finalize_model(cmtts_model* m) {
    const cmtts_config& c = m->cfg;
    if (c.hidden != 256 || c.res_channels != 256 || c.pred_filter != 256)
        return fail(CMTTS_E_UNSUPPORTED, "kernels are specialised for hidden = residual_channels = filter_size = 256");
    if (c.hidden % c.enc_heads) return fail(CMTTS_E_INVALID, "hidden not divisible by heads (model/blocks.py:209)");
    const int H = c.hidden, C = c.res_channels;
    Getter g{m->host, ""};
    Allocs& al = m->al;

    CHK(al.upload(omega_table(H), &m->omega_h));
    CHK(al.upload(omega_table(c.cwt_hidden), &m->omega_cwt));
    CHK(al.upload(omega_table(C), &m->omega_res));
    CHK(al.upload(pe_table(H, PE_ROWS), &m->pe_h));
    CHK(al.upload(pe_table(c.cwt_hidden, PE_ROWS), &m->pe_cwt));

    const std::string enc = "duration_pitch_energy_net.text_encoder.";
    GET(emb, enc + "embed_tokens.weight", c.n_symbols, H);
    UP(m->embed, emb);
    // one EncSALayer (model/blocks.py:560-618): shared by the text encoder and the optional FastspeechDecoder
    auto load_fft_layer = [&](const std::string& p, EncLayer& L) -> int {
        GET(l1g, p + "layer_norm1.weight", H); GET(l1b, p + "layer_norm1.bias", H);
        GET(l2g, p + "layer_norm2.weight", H); GET(l2b, p + "layer_norm2.bias", H);
        UP(L.ln1_g, l1g); UP(L.ln1_b, l1b); UP(L.ln2_g, l2g); UP(L.ln2_b, l2b);
        GET(inw, p + "self_attn.in_proj_weight", 3 * H, H);
        HostTensor qk; qk.shape = {2 * H, H, 1};
        qk.data.assign(inw->data.begin(), inw->data.begin() + (size_t)2 * H * H);
        CHK(pack_conv(al, qk, nullptr, nullptr, &L.qk));
        HostTensor qkv = *inw; qkv.shape = {3 * H, H, 1};
        std::vector<float> hp;      // k-major host copy of the contraction packed last
        // where a contraction's gate holds: its fp32 iteration-order fragments and their bf16 / fp16 copies
        auto frags = [&](const PackedConv& w, bool gate, float** f32, void** f16) -> int {
            if (!gate) return 0;
            CHK(al.upload(to_fragment_iter_order(hp, w.taps, w.cin, w.cout), f32));
            return upload16(al, hp, w.taps, w.cin, w.cout, f16, 2);
        };
        CHK(pack_conv(al, qkv, nullptr, nullptr, &L.qkv, &hp));
        CHK(frags(L.qkv, H % 32 == 0 && L.qkv.ld == L.qkv.cout, &L.qkv_f, L.qkv_f16));
        CHK(al.upload(transpose2d(inw->data.data() + (size_t)2 * H * H, H, H), &L.wvT));
        GET(ow, p + "self_attn.out_proj.weight", H, H);
        HostTensor ow3 = *ow; ow3.shape = {H, H, 1};
        CHK(pack_conv(al, ow3, nullptr, nullptr, &L.wo, &hp));
        CHK(frags(L.wo, H % 32 == 0 && L.wo.ld == L.wo.cout, &L.wo_f, L.wo_f16));
        GET(f1w, p + "ffn.ffn_1.weight", 4 * H, H, c.ffn_kernel); GET(f1b, p + "ffn.ffn_1.bias", 4 * H);
        CHK(pack_conv(al, *f1w, f1b, nullptr, &L.ffn1, &hp));
        CHK(frags(L.ffn1, L.ffn1.cin % 32 == 0 && L.ffn1.cout % 32 == 0 && L.ffn1.ld == L.ffn1.cout, &L.ffn1_f, L.ffn1_f16));
        if (L.ffn1.taps == 9 && L.ffn1.cin == 256 && L.ffn1.cout % 128 == 0 && L.ffn1.ld == L.ffn1.cout) {
            CHK(al.upload(to_wino43_xres_fragments(hp, L.ffn1.taps, L.ffn1.cin, L.ffn1.cout), &L.ffn1_q));
            CHK(al.upload(to_wino23_xres_fragments(hp, L.ffn1.taps, L.ffn1.cin, L.ffn1.cout), &L.ffn1_p));
        }
        GET(f2w, p + "ffn.ffn_2.weight", H, 4 * H); GET(f2b, p + "ffn.ffn_2.bias", H);
        HostTensor f2 = *f2w; f2.shape = {H, 4 * H, 1};
        CHK(pack_conv(al, f2, f2b, nullptr, &L.ffn2, &hp));      // (the fp32 and the 16-bit forms of this one have gates of their own)
        if (H == 256 && L.ffn2.cin % 128 == 0 && L.ffn2.ld == L.ffn2.cout) CHK(al.upload(to_fragment_iter_order(hp, 1, L.ffn2.cin, H), &L.ffn2_f));
        if (L.ffn2.cin % 32 == 0 && H % 32 == 0 && L.ffn2.ld == L.ffn2.cout) CHK(upload16(al, hp, 1, L.ffn2.cin, H, L.ffn2_f16, 2));
        return 0;
    };
    m->enc.resize(c.enc_layers);
    for (int i = 0; i < c.enc_layers; ++i) CHK(load_fft_layer(enc + "layers." + std::to_string(i) + ".op.", m->enc[i]));
    GET(eg, enc + "layer_norm.weight", H); GET(eb, enc + "layer_norm.bias", H);
    UP(m->encln_g, eg); UP(m->encln_b, eb);
    {   // optional FastspeechDecoder: as many layers as the state dict holds under "decoder.layers.N.op."
        int nd = 0;
        while (m->host.count("decoder.layers." + std::to_string(nd) + ".op.layer_norm1.weight")) ++nd;
        if (nd > 0) {
            m->dec.resize(nd);
            for (int i = 0; i < nd; ++i) CHK(load_fft_layer("decoder.layers." + std::to_string(i) + ".op.", m->dec[i]));
            GET(dg, "decoder.layer_norm.weight", H); GET(db, "decoder.layer_norm.bias", H);
            UP(m->decln_g, dg); UP(m->decln_b, db);
            GET(da, "decoder.pos_embed_alpha", 1);
            UP(m->dec_alpha, da);
        }
    }

    if (c.multi_speaker && c.n_speaker > 0) {   // speaker_embedder "none": nn.Embedding(n_speaker, hidden) (model/cmtts.py:26-38)
        GET(sw, "duration_pitch_energy_net.speaker_emb.weight", c.n_speaker, H);
        UP(m->spk_table, sw);
    } else if (c.multi_speaker) {
        GET(sw, "duration_pitch_energy_net.speaker_emb.weight", H, c.external_speaker_dim);
        GET(sb, "duration_pitch_energy_net.speaker_emb.bias", H);
        CHK(al.upload(transpose2d(sw->data.data(), H, c.external_speaker_dim), &m->spk_wt));
        UP(m->spk_b, sb);
    }

    const std::string va = "duration_pitch_energy_net.variance_adaptor.";
    auto load_pred = [&](Predictor& P, const std::string& p, int idim, int n_layers, int k, int odim, bool alpha) -> int {
        P.convs.resize(n_layers); P.ln_g.resize(n_layers); P.ln_b.resize(n_layers); P.odim = odim;
        P.convs_f.resize(n_layers, nullptr); P.convs_q.resize(n_layers, nullptr); P.convs_f16[0].resize(n_layers, nullptr); P.convs_f16[1].resize(n_layers, nullptr);
        for (int li = 0; li < n_layers; ++li) {
            const int cin = li == 0 ? idim : c.pred_filter;
            const std::string q = p + "conv." + std::to_string(li);
            GET(w, q + ".1.weight", c.pred_filter, cin, k); GET(b, q + ".1.bias", c.pred_filter);
            std::vector<float> hp;
            CHK(pack_conv(al, *w, b, nullptr, &P.convs[li], &hp));
            if ((cin == 256 || (cin == 128 && k == 5)) && c.pred_filter == 256 && P.convs[li].ld == 256)
                CHK(al.upload(to_fragment_iter_order(hp, k, cin, c.pred_filter), &P.convs_f[li]));
            if (k == 5 && (cin == 256 || cin == 128) && c.pred_filter == 256 && P.convs[li].ld == 256) {
                const std::vector<float> wq = to_wino43_iter_fragments(hp, k, cin, c.pred_filter);
                if (!wq.empty()) CHK(al.upload(wq, &P.convs_q[li]));
            }
            void* f16[2] = {nullptr, nullptr};
            if (cin % 32 == 0 && c.pred_filter % 32 == 0 && P.convs[li].ld == c.pred_filter) CHK(upload16(al, hp, k, cin, c.pred_filter, f16, 2));
            P.convs_f16[0][li] = f16[0]; P.convs_f16[1][li] = f16[1];
            GET(lg, q + ".3.weight", c.pred_filter); GET(lb, q + ".3.bias", c.pred_filter);
            UP(P.ln_g[li], lg); UP(P.ln_b[li], lb);
        }
        GET(lw, p + "linear.weight", odim, c.pred_filter); GET(lb2, p + "linear.bias", odim);
        UP(P.lin_w, lw); UP(P.lin_b, lb2);
        if (alpha) { GET(a, p + "pos_embed_alpha", 1); UP(P.alpha, a); }
        return 0;
    };
    CHK(load_pred(m->dur, va + "duration_predictor.", H, c.dur_layers, c.dur_kernel, 1, false));
    CHK(load_pred(m->energy, va + "energy_predictor.", H, c.pred_layers, c.pred_kernel, 1, true));
    const int cwt_out = c.use_uv ? 11 : 10;
    CHK(load_pred(m->cwt, va + "cwt_predictor.1.", c.cwt_hidden, c.pred_layers, c.pred_kernel, cwt_out, true));
    {
        GET(w, va + "cwt_predictor.0.weight", c.cwt_hidden, H); GET(b, va + "cwt_predictor.0.bias", c.cwt_hidden);
        HostTensor w3 = *w; w3.shape = {c.cwt_hidden, H, 1};
        std::vector<float> hp;
        CHK(pack_conv(al, w3, b, nullptr, &m->cwt_in, &hp));
        if (H % 32 == 0 && c.cwt_hidden % 32 == 0 && m->cwt_in.ld == c.cwt_hidden)
            CHK(al.upload(to_fragment_iter_order(hp, 1, H, c.cwt_hidden), &m->cwt_in_f));
        GET(bins, va + "energy_bins", c.energy_bins - 1); UP(m->energy_bins, bins);
        GET(ee, va + "energy_embedding.weight", c.energy_bins, H); UP(m->energy_emb, ee);
        GET(pe, va + "pitch_embed.weight", c.pitch_bins, H); UP(m->pitch_emb, pe);
        GET(s0w, va + "cwt_stats_layers.0.weight", c.cwt_hidden, H); GET(s0b, va + "cwt_stats_layers.0.bias", c.cwt_hidden);
        GET(s2w, va + "cwt_stats_layers.2.weight", c.cwt_hidden, c.cwt_hidden); GET(s2b, va + "cwt_stats_layers.2.bias", c.cwt_hidden);
        GET(s4w, va + "cwt_stats_layers.4.weight", 2, c.cwt_hidden); GET(s4b, va + "cwt_stats_layers.4.bias", 2);
        CHK(al.upload(transpose2d(s0w->data.data(), c.cwt_hidden, H), &m->st0_wt)); UP(m->st0_b, s0b);
        CHK(al.upload(transpose2d(s2w->data.data(), c.cwt_hidden, c.cwt_hidden), &m->st2_wt)); UP(m->st2_b, s2b);
        CHK(al.upload(transpose2d(s4w->data.data(), 2, c.cwt_hidden), &m->st4_wt)); UP(m->st4_b, s4b);
    }

    // ---- denoiser
    {
        GET(w, "net.input_projection.0.conv.weight", C, c.n_mels, 1); GET(b, "net.input_projection.0.conv.bias", C);
        std::vector<float> hp;
        CHK(pack_conv(al, *w, b, nullptr, &m->in_proj, &hp));
        if (c.n_mels % 8 == 0 && C % 32 == 0 && m->in_proj.ld == C) CHK(al.upload(to_fragment_order(hp, 1, c.n_mels, C), &m->in_proj_f));
        GET(m0, "net.mlp.0.linear.weight", 4 * C, C); GET(m2, "net.mlp.2.linear.weight", C, 4 * C);
        CHK(al.upload(transpose2d(m0->data.data(), 4 * C, C), &m->mlp0_wt));
        CHK(al.upload(transpose2d(m2->data.data(), C, 4 * C), &m->mlp2_wt));
    }
    const int NL = c.res_layers;
    m->res.resize(NL);
    std::vector<float> dproj((size_t)C * NL * C), sproj;
    if (c.multi_speaker) sproj.resize((size_t)H * NL * C);
    HostTensor cond_w, cond_b;      // the conditioner projections of all layers stacked: [NL * C][H][1] and its bias
    cond_w.shape = {(int64_t)NL * C, H, 1};
    cond_b.shape = {(int64_t)NL * C};
    // gate permutation: packed 2n-row group g = [rows g*n.. of the sigmoid half | rows C + g*n.. of the tanh half]
    auto gate_perm = [C](int n) {
        std::vector<int> perm(2 * C);
        for (int r = 0; r < 2 * C; ++r) perm[r] = (r / n % 2) * C + r / (2 * n) * n + r % n;
        return perm;
    };
    // n = 32: the per-layer kernels' 64-row groups; n = 16, fused kernel: every 32-row tile = [16 sigmoid rows | 16 tanh rows] of the same 16 channels
    const std::vector<int> perm = gate_perm(32), perm16 = gate_perm(16);
    for (int l = 0; l < NL; ++l) {
        const std::string p = "net.residual_layers." + std::to_string(l) + ".";
        GET(w3, p + "conv_layer.conv.weight", 2 * C, C, 3); GET(b3, p + "conv_layer.conv.bias", 2 * C);
        CHK(pack_conv(al, *w3, b3, &perm, &m->res[l].conv3));
        std::vector<float> hp = kmajor(*w3, &perm16);      // the fused kernels read fragments only: no device copy of this k-major form
        CHK(al.upload(to_fragment_order(hp, 3, C, 2 * C), &m->res[l].w3f));
        if (C == 256) CHK(al.upload(to_wino_fragments(hp, C, 2 * C), &m->res[l].w3w));
        if (C == 256) CHK(al.upload(to_wino43_fragments(hp, C, 2 * C), &m->res[l].w3w43));
        CHK(upload16(al, hp, 3, C, 2 * C, m->res[l].w3f16, 3));
        std::vector<float> bperm(2 * C);
        for (int r = 0; r < 2 * C; ++r) bperm[r] = b3->data[perm16[r]];
        CHK(al.upload(bperm, &m->res[l].b3f));
        GET(wc, p + "conditioner_projection.conv.weight", C, H, 1); GET(bc, p + "conditioner_projection.conv.bias", C);
        CHK(pack_conv(al, *wc, bc, nullptr, &m->res[l].cond));
        cond_w.data.insert(cond_w.data.end(), wc->data.begin(), wc->data.end());
        cond_b.data.insert(cond_b.data.end(), bc->data.begin(), bc->data.end());
        GET(wo, p + "output_projection.conv.weight", 2 * C, C, 1); GET(bo, p + "output_projection.conv.bias", 2 * C);
        CHK(pack_conv(al, *wo, bo, nullptr, &m->res[l].outp, &hp));
        CHK(al.upload(to_fragment_order(hp, 1, C, 2 * C), &m->res[l].wof));
        CHK(upload16(al, hp, 1, C, 2 * C, m->res[l].wof16, 3));
        GET(wd, p + "diffusion_projection.linear.weight", C, C);
        for (int n = 0; n < C; ++n)
            for (int k = 0; k < C; ++k) dproj[(size_t)k * NL * C + l * C + n] = wd->data[(size_t)n * C + k];
        if (c.multi_speaker) {
            GET(ws, p + "speaker_projection.linear.weight", C, H);
            for (int n = 0; n < C; ++n)
                for (int k = 0; k < H; ++k) sproj[(size_t)k * NL * C + l * C + n] = ws->data[(size_t)n * H + k];
        }
    }
    {   // stacked conditioner projections (one GEMM for all layers; cond does not depend on the step)
        std::vector<float> hp;
        CHK(pack_conv(al, cond_w, &cond_b, nullptr, &m->cond_all, &hp));
        if (H % 8 == 0 && (NL * C) % 32 == 0 && m->cond_all.ld == NL * C)
            CHK(al.upload(to_fragment_order(hp, 1, H, NL * C), &m->cond_all_f));
        if (H % 16 == 0 && (NL * C) % 32 == 0 && m->cond_all.ld == NL * C) CHK(upload16(al, hp, 1, H, NL * C, m->cond_all_f16, 3));
    }
    CHK(al.upload(dproj, &m->dproj_wt));
    if (c.multi_speaker) CHK(al.upload(sproj, &m->sproj_wt));
    {
        GET(w, "net.skip_projection.conv.weight", C, C, 1); GET(b, "net.skip_projection.conv.bias", C);
        std::vector<float> hp;
        CHK(pack_conv(al, *w, b, nullptr, &m->skip_proj, &hp));
        if (C % 32 == 0 && m->skip_proj.ld == C) CHK(al.upload(to_fragment_order(hp, 1, C, C), &m->skip_f));
        GET(w2, "net.output_projection.conv.weight", c.n_mels, C, 1); GET(b2, "net.output_projection.conv.bias", c.n_mels);
        CHK(pack_conv(al, *w2, b2, nullptr, &m->out_proj, &hp));
        {   // rows padded to a multiple of 32 with zeros for the MFMA tiles of the fused tail
            const int ld = m->out_proj.ld, Mp = round_up(c.n_mels, 32);
            std::vector<float> padded((size_t)C * Mp, 0.f);
            for (int k = 0; k < C; ++k)
                for (int n = 0; n < c.n_mels; ++n) padded[(size_t)k * Mp + n] = hp[(size_t)k * ld + n];
            CHK(al.upload(to_fragment_order(padded, 1, C, Mp), &m->outp_f));
        }
    }
    if (m->cond_all_f && (NL * C) % 512 == 0) {
        // the pitch-table factor of the conditioner projections: the stacked GEMM on pitch_embed^T [H][pitch_bins] (one "utterance" of
        // pitch_bins "frames"), bias included
        GET(pe, va + "pitch_embed.weight", c.pitch_bins, H);
        float* peT = nullptr;
        void* p2 = nullptr;
        CHK(al.upload(transpose2d(pe->data.data(), c.pitch_bins, H), &peT));
        CHK(al.upload(std::vector<float>((size_t)NL * C, 0.f), &m->cond_zero_bias));
        HIPCHK(hipMalloc(&p2, (size_t)NL * C * c.pitch_bins * sizeof(float) + 256));
        al.ptrs.push_back(p2);
        CondGemmArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.X = peT; ga.Wf = m->cond_all_f; ga.bias = m->cond_all.bias; ga.Y = (float*)p2;
        ga.B = 1; ga.T = c.pitch_bins; ga.M = NL * C; ga.K = H; ga.force = 1; ga.row_split = NL * C / 512;
        if (cmtts_launch_cond_gemm(&ga, nullptr) == 0) {
            void* p2t = nullptr;
            HIPCHK(hipMalloc(&p2t, (size_t)NL * C * c.pitch_bins * sizeof(float) + 256));
            al.ptrs.push_back(p2t);
            k_transpose((const float*)p2, (float*)p2t, NL, C, c.pitch_bins, nullptr);      // [NL][C][bins] -> [NL][bins][C]
            HIPCHK(hipStreamSynchronize(nullptr));
            m->cond_p2 = (float*)p2;
            m->cond_p2t = (float*)p2t;
        }
    }
    m->host.clear();
    m->finalized = true;
    return 0;
}

int finalize_vocoder(cmtts_vocoder* v) {
    Getter g{v->host, ""};
    Allocs& al = v->al;
    GET(pw, "conv_pre.weight", 512, 80, 7); GET(pb, "conv_pre.bias", 512);
    CHK(pack_conv(al, *pw, pb, nullptr, &v->conv_pre));
    int ch = 512;
    for (int i = 0; i < 4; ++i) {
        const int co = ch / 2;
        GET(uw, "ups." + std::to_string(i) + ".weight", ch, co, v->up_kernel[i]);
        GET(ub, "ups." + std::to_string(i) + ".bias", co);
        {
            std::vector<float> tt;
            CHK(pack_conv_transpose(al, *uw, *ub, v->up_rate[i], &v->ups[i], &tt));
            const int mrows = v->up_rate[i] * co;
            if (!tt.empty() && ch % 16 == 0 && mrows % 32 == 0) {
                CHK(al.upload(to_fragment_iter_order(tt, 2, ch, mrows), &v->ups_f[i]));
                CHK(upload16(al, tt, 2, ch, mrows, v->ups_f16[i], 3));
            }
        }
        for (int j = 0; j < 3; ++j) {
            const int r = i * 3 + j, k = v->rb_kernel[j];
            for (int mi = 0; mi < 3; ++mi) {
                // one conv of a ResBlock: k-major + iteration-order fragments, the Winograd forms where a kernel takes them, the three 16-bit copies
                auto load_conv = [&](const std::string& name, PackedConv* pc, float** f32, float** w32, float** q32, void** f16) -> int {
                    GET(w, name + ".weight", co, co, k);
                    GET(b, name + ".bias", co);
                    std::vector<float> hp;
                    CHK(pack_conv(al, *w, b, nullptr, pc, &hp));
                    CHK(al.upload(to_fragment_iter_order(hp, k, co, co), f32));
                    if (co >= 128 || (co == 64 && k >= 7)) { const std::vector<float> wf = to_wino_iter_fragments(hp, k, co, co); if (!wf.empty()) CHK(al.upload(wf, w32)); }
                    if (co >= 64) { const std::vector<float> wf = to_wino43_iter_fragments(hp, k, co, co); if (!wf.empty()) CHK(al.upload(wf, q32)); }     // (C = 64, k = 3: the fused F(4,3) pair, conv_xlq_pair.hip)
                    return upload16(al, hp, k, co, co, f16, 3);
                };
                const std::string p = "resblocks." + std::to_string(r);
                CHK(load_conv(p + ".convs1." + std::to_string(mi), &v->c1[r][mi], &v->c1f32[r][mi], &v->c1w32[r][mi], &v->c1q32[r][mi], v->c1f[r][mi]));
                CHK(load_conv(p + ".convs2." + std::to_string(mi), &v->c2[r][mi], &v->c2f32[r][mi], &v->c2w32[r][mi], &v->c2q32[r][mi], v->c2f[r][mi]));
            }
        }
        ch = co;
    }
    GET(qw, "conv_post.weight", 1, ch, 7); GET(qb, "conv_post.bias", 1);
    CHK(al.upload(qw->data, &v->post_w));
    CHK(al.upload(qb->data, &v->post_b));
    v->post_cin = ch;
    v->host.clear();
    v->finalized = true;
    return 0;
}
