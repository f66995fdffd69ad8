// The model and vocoder handles of the C ABI (include/cmtts_hip.h) and what their weight import (import.hip) and their launch
// sequences (the denoiser and sampler's: denoiser_side.hip; the text and frame side's: text_side.hip; the vocoder's: vocoder.hip; the rest of the C ABI: cmtts_api.hip; what those share beyond the handles: launch.h) share: host tensors, packed convs, the device allocation list, the per-layer weight structs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/cmtts_hip.h"

int fail(int code, const std::string& msg);     // cmtts_api.hip: sets cmtts_last_error()'s thread-local message, returns code
#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) return fail(CMTTS_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define CHK(x)                 \
    do {                       \
        int r_ = (x);          \
        if (r_ != 0) return r_; \
    } while (0)

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    int64_t dim(int i) const { return i < (int)shape.size() ? shape[i] : 1; }
};

struct PackedConv {
    float* w = nullptr;     // device, [phase][tap][cin][ld]
    float* bias = nullptr;  // device, [cout] (packed row order)
    int cout = 0, cin = 0, taps = 0, ld = 0;
    long tap_stride = 0, phase_stride = 0;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct Allocs {
    std::vector<void*> ptrs;
    int upload(const std::vector<float>& h, float** out) {
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, h.size() * sizeof(float) + 256));
        HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        ptrs.push_back(p);
        *out = (float*)p;
        return 0;
    }
    int upload_bytes(const void* h, size_t nbytes, void** out) {
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, nbytes + 256));
        HIPCHK(hipMemcpy(p, h, nbytes, hipMemcpyHostToDevice));
        ptrs.push_back(p);
        *out = p;
        return 0;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

constexpr int PE_ROWS = 4096;     // rows of the sinusoid tables (import.hip: pe_table)

struct EncLayer {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    PackedConv qk, qkv, wo, ffn1, ffn2;     // qkv: the whole in_proj_weight as one [3H][H] contraction (fused attention path)
    float* ffn1_f = nullptr;   // ffn1 as MFMA A fragments in iteration order (conv_xres.hip)
    float* ffn1_q = nullptr;   // ffn1 (k = 9, 256 input channels) as F(4,3) fragments (conv_xres.hip, WQ == 1 instances: to_wino43_xres_fragments), else null
    float* ffn1_p = nullptr;   // ... as F(2,3) fragments (WQ == 2 instances: to_wino23_xres_fragments), else null
    float* qkv_f = nullptr;    // the same for the in-projection and the out-projection (round 2: LayerNorm + projection in one launch)
    float* wo_f = nullptr;
    float* ffn2_f = nullptr;   // the FFN linear as A fragments in iteration order: conv_xres.hip's FFN fusion
    void* ffn1_f16[2] = {nullptr, nullptr};   // bf16 / fp16 fragment-order copies of the two FFN contractions (conv_mfma16.hip; the opt-in "text16")
    void* ffn2_f16[2] = {nullptr, nullptr};
    void* qkv_f16[2] = {nullptr, nullptr};    // ... and of the in- / out-projection of the self-attention
    void* wo_f16[2] = {nullptr, nullptr};
    float* wvT;  // [256 c][256 d]
};
struct Predictor {
    std::vector<PackedConv> convs;
    std::vector<float*> convs_f;     // 256 -> 256 convs as MFMA A fragments in iteration order (conv_xl_kernel), else null
    std::vector<void*> convs_f16[2]; // bf16 / fp16 fragment-order copies (conv_mfma16.hip; the opt-in "text16"), else null
    std::vector<float*> convs_q;     // k = 5 convs into 256 rows: F(4,3) transformed weights (conv_k5q.hip: to_wino43_iter_fragments), else null
    std::vector<float*> ln_g, ln_b;
    float *lin_w = nullptr, *lin_b = nullptr, *alpha = nullptr;
    int odim = 0;
};
struct ResLayer {
    PackedConv cond, conv3, outp;
    float *w3f = nullptr, *wof = nullptr;   // fragment-order copies for the fused kernel
    float* w3w = nullptr;                   // Winograd F(2,3) transformed conv weights as A fragments (persistent denoiser, 8-wave WINO instances)
    float* w3w43 = nullptr;                 // Winograd F(4,3) transformed conv weights (8-wave WINO == 2 instances: to_wino43_fragments)
    float* b3f = nullptr;                   // conv_layer bias in the fused kernel's row order
    void *w3f16[3] = {nullptr, nullptr, nullptr}, *wof16[3] = {nullptr, nullptr, nullptr};   // bf16 / fp16 / fp16x3 (hi | lo) fragment-order copies
};

struct cmtts_model {
    cmtts_config cfg;
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    int precision = 0;     // operand precision of the residual-block contractions: 0 fp32, 1 bf16, 2 fp16
    int text16 = 0;        // 16-bit models (precision 1 / 2): the FFN contractions of the FFT blocks with 16-bit operands too (opt-in: the text side feeds the integer stages — durations, pitch buckets, lengths — which then depend on the precision mode; cmtts_model_set_option)
    int winograd = 1;                       // fp32 persistent denoiser: Winograd k = 3 conv (cmtts_model_set_option "winograd"): 1 = F(4,3) (~8e-6 on the mel against the direct form),
                                            // 2 = F(2,3) (~4e-6), 0 = direct
    int batch_invariant = 0;                // fp32, winograd = 1: the per-layer residual blocks in the persistent stack's F(4,3) form (cmtts_model_set_option "batch_invariant")
    int ffn2_split = 1;    // FFT blocks: the FFN linear as 8 partial GEMMs over K segments + one reduction (another fp32 summation order than one launch: a property of the model handle, cmtts_model_set_option)
    cmtts_variance_controls vc = {1.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    cmtts_control_tables ct = {nullptr, nullptr, nullptr, 0};      // per-phoneme control tables [B][ld] (cmtts_set_control_tables); a table replaces the scalar of its control
    cmtts_duration_targets dt = {nullptr, nullptr, nullptr, 0, 0};      // duration targets [B][n_seg] (cmtts_set_duration_targets): the fit runs behind the durations kernel
    Allocs al;
    float *embed = nullptr, *omega_h = nullptr, *omega_cwt = nullptr, *omega_res = nullptr;
    float *pe_h = nullptr, *pe_cwt = nullptr;   // sinusoid tables [PE_ROWS][C]
    std::vector<EncLayer> enc;
    float *encln_g = nullptr, *encln_b = nullptr;
    // FastspeechDecoder (model/modules.py:154-165): optional, present when the state dict holds "decoder.*"
    std::vector<EncLayer> dec;
    float *decln_g = nullptr, *decln_b = nullptr, *dec_alpha = nullptr;
    float *spk_wt = nullptr, *spk_b = nullptr, *spk_table = nullptr;
    Predictor dur, energy, cwt;
    PackedConv cwt_in;
    float* cwt_in_f = nullptr;     // the same as MFMA A fragments in iteration order (conv_xres.hip)
    float *energy_bins = nullptr, *energy_emb = nullptr, *pitch_emb = nullptr;
    float *st0_wt = nullptr, *st0_b = nullptr, *st2_wt = nullptr, *st2_b = nullptr, *st4_wt = nullptr, *st4_b = nullptr;
    PackedConv in_proj, skip_proj, out_proj;
    float* in_proj_f = nullptr;   // input projection as MFMA A fragments (inproj.hip)
    float *skip_f = nullptr, *outp_f = nullptr;   // skip / output projection in fragment order (persistent kernel's tail)
    PackedConv cond_all;   // the 20 conditioner_projections stacked: [256][NL*256] (+ stacked bias)
    float* cond_all_f = nullptr;   // the same in MFMA A-fragment order (cond_gemm.hip)
    // factored conditioner projections (cond_factored below): P2[r][i] = sum_k Wc[r][k] * pitch_embed[i][k] + bias[r], [NL*C][pitch_bins],
    // computed once at cmtts_finalize with cond_gemm_kernel itself; a zero bias vector for the phoneme-level factor
    float* cond_p2 = nullptr;
    float* cond_p2t = nullptr;             // [NL][pitch_bins][C]: cond_p2 with the channels contiguous (PersistArgs.p2t)
    float* cond_zero_bias = nullptr;
    void* cond_all_f16[3] = {nullptr, nullptr, nullptr};   // bf16 / fp16 / fp16x3 (hi | lo) fragment-order copies (cond_gemm16.hip)
    float *mlp0_wt = nullptr, *mlp2_wt = nullptr, *dproj_wt = nullptr, *sproj_wt = nullptr;
    std::vector<ResLayer> res;
    // Step-embedding cache (round 2): the DiffusionEmbedding -> MLP -> 20 stacked diffusion projections of a timestep depend
    // on nothing but the timestep, and the consistency sampler evaluates every batch at the same few sigmas: the row
    // [NL * C] of each rescaled timestep seen by cmtts_sample is kept on the device (first use computes and copies it; an
    // entry is used once the event recorded behind that copy has completed, whatever stream asks).
    struct StepRow { float t; float* row; hipEvent_t ready; };
    std::vector<StepRow> step_rows;
};

struct cmtts_vocoder {
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    Allocs al;
    PackedConv conv_pre;
    PackedConv ups[4];
    float* ups_f[4] = {nullptr, nullptr, nullptr, nullptr};   // two-tap stacked-phase weights as iteration-order fragments (convT_xl_kernel)
    void* ups_f16[4][3] = {};                                  // the same as bf16 / fp16 / fp16x3 (hi | lo) fragments (convT_xl16_kernel)
    int up_rate[4] = {8, 8, 2, 2};
    int up_kernel[4] = {16, 16, 4, 4};
    int rb_kernel[3] = {3, 7, 11};
    int rb_dil[3] = {1, 3, 5};
    PackedConv c1[12][3], c2[12][3];
    void *c1f[12][3][3] = {}, *c2f[12][3][3] = {};   // bf16 / fp16 / fp16x3 (hi | lo) fragment-order copies of the ResBlock convs
    float *c1f32[12][3] = {}, *c2f32[12][3] = {};    // fp32 fragments in iteration order (resblock_pair.hip: pair kernels at C <= 64, conv_xl above)
    float *c1q32[12][3] = {}, *c2q32[12][3] = {};    // F(4,3) fragments of the dilation-1 convs (conv_xlq_kernel; c1q32 only for the first pair of a ResBlock), else null
    float *c1w32[12][3] = {}, *c2w32[12][3] = {};    // Winograd-transformed fragments of the C >= 128 stages (conv_xlw_kernel), else null
    int winograd = 1;                                 // fp32 generator: ResBlock convs of the C >= 128 stages in their Winograd form (cmtts_vocoder_set_option "winograd")
    int batch_invariant = 0;                          // fp32 generator: every launch-size gate takes its large-launch branch (cmtts_vocoder_set_option "batch_invariant")
    int precision = 0;                               // 0 fp32, 1 bf16, 2 fp16 operands in the ResBlock convs
    int ups16 = 1;                                    // 16-bit modes: upsampler operands in 16 bits as well (cmtts_vocoder_set_option "ups16"; 0 = fp32 upsamplers, different numerics)
    float *post_w = nullptr, *post_b = nullptr;
    int post_cin = 32, post_k = 7;
};

// import.hip
int pack_conv(Allocs& al, const HostTensor& W, const HostTensor* bias, const std::vector<int>* perm, PackedConv* out,
              std::vector<float>* host_copy = nullptr);
int set_tensor(std::map<std::string, HostTensor>& host, const char* name, const float* data, const int64_t* shape, int ndim);
int finalize_model(cmtts_model* m);         // re-pack + upload of every tensor set so far; the caller releases m->al on failure
int finalize_vocoder(cmtts_vocoder* v);     // ... v->al
