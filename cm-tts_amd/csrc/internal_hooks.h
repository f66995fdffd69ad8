// NOT part of the C ABI (include/cmtts_hip.h): A/B switches between a fused kernel and the path it replaces, for the bitwise
// cross-check tests (tests/test_gpu_parity.py) and the measurement tools (tools/).  Every pair produces identical bits EXCEPT:
// attn_fused for L > 192 (the key-chunked online softmax against the two-pass softmax of the three-launch path: ~1e-7),
// attn_fused for L <= 192 against the three-launch path (different fp32 summation order: <= 2e-5 on the encoder output),
// cond_gemm16 (16-bit against fp32 operands of the conditioner GEMM in bf16 / fp16 / fp16x3 models: a numerics switch — since
// round 3 the 16-bit form is the default for EVERY shape of a 16-bit model, which changed those models' default numerics against
// round 2), persist_wino (the fp32 persistent stack's k = 3 conv in a Winograd form — the process-wide A/B twin of the model option "winograd":
// 3 (default since round 5) F(4,3), <= 1.8e-5 per network evaluation against the direct form; 1 F(2,3) (round 4), <= 1e-5; 2 runs as 1 (round 5's
// one-wave-per-SIMD F(2,3) stack left the build in round 6: tools/attic/); 0 direct), ffn_wino (the FFT blocks' k = 9 FFN conv as Winograd tap groups in the fused launch: 1 (default
// since round 6) F(2,3) over output pairs, ~2.5e-6 on the encoder output against the direct form; 2 F(4,3) over quads (round 5), ~4.5e-6; 0 direct), pred_wino (round 6: the frame-level
// pitch predictor's k = 5 convs as F(4,3) tap groups, conv_k5q.hip, at every launch size: ~7e-6 on the cwt output; 0 = the direct kernels), voc_wino43 (round 5: the Winograd path's convs as F(4,3) tap groups over output quads, conv_xlq_kernel: 1 (default)
// dilation 1 and 3 everywhere + dilation 5 at C = 256 or k = 3, 2 only dilation 1, 3 every conv, 0 none), voc_wino (round 4: the fp32 generator's C >= 128 ResBlock
// convs in their Winograd form — 0 never, 1 (default) launches of >= 1024 column tiles, 2 always; <= 1.2e-6 on the waveform), voc_qpair (round 6: the k = 3 pairs of the
// C = 64 / 128 stages of that path as ONE fused F(4,3) launch, conv_xlq_pair.hip — 0 the forms it replaces (C = 128: two conv_xlq launches; C = 64: the direct pair kernel), 1 (default)
// with voc_wino's launch-size rule, 2 always; <= 1e-6 on the waveform between the arms).  The switches are process-wide and unsynchronised.  Exported from libcmtts_hip.so so that ctypes can reach it
// (cmtts_amd/_lib.py: internal_set).
// The kernel launchers of resblock_args.h, cond_gemm.h and inproj.h are exported too: tests/test_gpu_denoiser_kernels.py calls them directly (-2 = an
// argument the launcher's header excludes, nothing launched).
// The launch wrappers of kernels.h have one hook each, cmtts_internal_k_<name> (kernel_hooks.hip, declared at the end of this file):
// tests/test_gpu_frame_kernels.py calls the frame-side and small kernels alone through them (cases: tests/frame_kernel_cases.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
// Returns the previous value (a value outside the switch's range only queries) or CMTTS_E_INVALID for an unknown name.
// Names: cond_gemm, persist_tail, inproj_fused, ffn_xres, ffn_fused, text_xres, attn_fused, pred_xl, pred_head, voc_pair,
// voc_pair3, voc_pairw, voc_rb16, voc_xl, voc_xl16, voc_upsT, post_v4, cond_gemm16, cond_factored, cond_inkernel, xres_small, pred_xres, cwt_in_phoneme, voc_xl_split, text_xt16,
// persist_wino, ffn_wino, pred_wino, voc_wino, voc_wino43, voc_wino64, voc_wino64_k, voc_qpair, xres_nt, and (round 6, same bits on / off) attn_qb (attention with the queries split over workgroups),
// stats_mlp (cwt_stats_layers as one launch), energy_head (energy bucketize + embedding add inside the energy predictor's head launch)   (cmtts_api.hip: cmtts_internal_set; the denoiser's and conditioner's switches: denoiser_side.hip; the voc_* switches and post_v4: vocoder.hip; the FFT blocks', predictors' and frame side's switches: text_side.hip).
int cmtts_internal_set(const char* name, int value);
// Test hook: the stacked conditioner projections alone, with the model's current precision mode.  cond_ct [B][hidden][T] -> cp [B][NL * C][T]
// (device pointers).  Returns a cmtts_status.
struct cmtts_model;
int cmtts_internal_cond_projections(struct cmtts_model* m, const float* cond_ct, int B, int T, float* cp, void* stream);
// Test hook: the same tensor expanded from the factors cmtts_frame_forward_sub returns (cond_p1 [B][NL*C][p1_ld], mel2ph, p_idx [B][T])
int cmtts_internal_cond_factored(struct cmtts_model* m, const float* p1, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx, int B, int T,
                                 float* cp, void* stream);
// Test hook: the streaming rounds' mel window gather alone (stream_windows.hip: mel_window_gather_kernel).  mel_ct [B][80][T] ->
// out [N][80][Tw], windows: device [N][4] int32 (utterance, start, core_off, core_len) — NOT validated here (the caller's test does).
int cmtts_internal_mel_window_gather(const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, float* out, void* stream);
// Test hook: the raw Philox4x32-10 blocks of the seeded noise (noise_philox.hip), before Box-Muller: bits uint32
// [n_draws][B][T][ceil(M / 4)][4] for the arguments of cmtts_noise_fill (seeds: device int64 [B]).
int cmtts_internal_noise_bits(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, uint32_t* bits, void* stream);
// Test hook: one of the host-side weight packers (weight_pack.h) on HOST memory; never touches the GPU.  layout = the packer's name without "to_"
// (fragment_order, fragment_iter_order, fragment16, fragment16_iter, fragment16_split, wino_fragments, wino43_fragments, wino_iter_fragments,
// wino43_iter_fragments, wino43_xres_fragments, wino23_xres_fragments, conv2d_fragments, lstm_fragments (taps 1, M 1024)); kmajor [taps][K][M] floats; mode 1 = bf16 / 2 = fp16 for fragment16 and
// fragment16_iter, ignored elsewhere.  *need = the size of the packed stream in bytes, padding included; out == NULL only queries it.  An unknown
// layout, a (taps, K, M) the packer does not cover or out_bytes < *need returns CMTTS_E_INVALID.
int cmtts_internal_pack_weights(const char* layout, const float* kmajor, int taps, int K, int M, int mode, void* out, size_t out_bytes, size_t* need);
// Measurement hook (tools/duration_fit_bench.py): duration_fit_kernel alone on the caller's buffers, the launch cmtts_text_forward adds behind its
// durations kernel while targets are installed (cmtts_set_duration_targets: d_rounded fp32 [B][L] in place, cum int32 [B][L], mel_len int64 [B],
// seg int32 [B][L] or NULL, target int32 [B][n_seg], unmet int32 [B] or NULL).  L up to 4096.
int cmtts_internal_duration_fit(float* d_rounded, int* cum, int64_t* mel_len, const int64_t* src_lens, const int32_t* seg, const int32_t* target,
                                int32_t* unmet, int B, int L, int n_seg, void* stream);
// Test hook: retake_step_kernel alone (retake.hip; the one kernel between the evaluations of cmtts_retake) on the caller's device buffers.
// mode 0: out [N][Tw][M] = scale * z(seeds[n], draw, windows[n].start + t, m); 1: out [N][Tw][M] = (regen ? x0 : known) + (z * scale) * 0.85f;
// 2: out [B][T][M] (utterance windows[n].b, frame start + t) = x0 (+ (z * scale) * 0.85f when scale >= 0) where regen [N][Tw] is set, nothing
// else written.  windows: DEVICE int32 [N][4] — NOT validated here (the caller's test does).
int cmtts_internal_retake_step(const float* x0, const float* known, const uint8_t* regen, const int64_t* seeds, const int32_t* windows, int N, int Tw,
                               int M, int T, int draw, float scale, int mode, float* out, void* stream);
// Test hook: the utterance-evaluations (sum over evaluations of the utterances they ran on) launched by the last sampler call of the process:
// B * n_steps after a uniform call, sum(n_steps[b]) after cmtts_sample_mixed — finished utterances really left, seen without timing anything.
long cmtts_internal_sample_rows(void);
// Test hook: the sampler's fp32 scalings of one evaluation (denoiser_side.hip: scalings — get_scalings_for_boundary_condition and the rescaled
// timestep) on the HOST; never touches the GPU.  out4 = (c_in, c_out, c_skip, 250 log(sigma)).
void cmtts_internal_eval_scalings(float sigma, float sigma_min, float sigma_data, float* out4);
// Test hook: the speaker encoder's Conv2D packer with its BatchNorm fold (weight_pack.h: pack_conv2d_bn) on HOST memory.  kernel (taps, cin, cout) floats, bias [cout] or
// NULL, bn [4][cout] (gamma, beta, moving mean, moving variance) or NULL.  *need = floats of the fragment stream; frag == NULL only queries it.
int cmtts_internal_spkenc_pack(const float* kernel, int taps, int cin, int cout, const float* bias, const float* bn, float* frag, size_t frag_floats,
                               float* bias_out, size_t* need);
// Test hook: conv2d_mfma_kernel alone (speaker_encoder.hip) on the caller's device buffers: x [B][H][W][cin] -> y [B][ceil(H/stride)][ceil(W/stride)][cout] =
// clip(conv + bias) (+ res, clip again, when res is not NULL), TensorFlow 'same' padding; frag / bias from cmtts_internal_spkenc_pack.
int cmtts_internal_spkenc_conv(const float* x, const float* frag, const float* bias, const float* res, int B, int H, int W, int cin, int cout, int ks,
                               int stride, float* y, void* stream);
// Test hook: the fbank kernel alone on rows whose kept span the CALLER sets: info [rows][4] int32 with (first, last) filled in (device); otherwise as
// cmtts_spkenc_features behind its trim.  twiddles are made and released inside the call (it synchronises the stream).
int cmtts_internal_spkenc_fbank(const float* wav, int rows, int64_t ld, int fs, int win_length, int mode, const int32_t* offsets, int max_windows,
                                float* windows, int32_t* info, void* stream);
// Test hooks of the GE2E encoder (ge2e.h; tests/test_gpu_ge2e.py, tools/ge2e_bench.py).  _mel: the front end alone, as cmtts_ge2e_features without a
// handle (the tables are made and released inside the call, which synchronises the stream).  _layer (kernel_hooks.hip): one LSTM layer — the projection
// GEMM and the recurrence — on the caller's device buffers: x [N][T][K], wih / whh the lstm_fragments streams of cmtts_internal_pack_weights, bias
// [1024] in packed row order, lens int32 [N] or NULL, tile 16 (-2 otherwise), pre [N][T][1024] scratch, hseq [N][T][256], hlast [N][256].  _tail
// (kernel_hooks.hip): hlast [W][256], lin_t [256 k][256 o] -> emb_w [W][256] and, with row_map (DEVICE int32 [W]) not NULL, emb [rows][256].
// _mel_basis: mel_basis.cpp at
// the odd transform length, out [40][276] (host memory, no GPU).
int cmtts_internal_ge2e_mel(const float* wav, int rows, int64_t ld, const int32_t* n_valid, int mode, int max_windows, int T, float* windows,
                            int32_t* win_lens, int32_t* info, void* stream);
int cmtts_internal_ge2e_layer(const float* x, int N, int T, int K, const float* wih, const float* whh, const float* bias, const int32_t* lens, int tile,
                              float* pre, float* hseq, float* hlast, void* stream);
int cmtts_internal_ge2e_tail(const float* hlast, int W, const float* lin_t, const float* lin_b, float* emb_w, const int32_t* row_map, int rows,
                             float* emb, void* stream);
int cmtts_internal_ge2e_mel_basis(float* out);
// Test hooks (kernel_hooks.hip; tests/test_gpu_frame_kernels.py with the cases of tests/frame_kernel_cases.py): the k_* wrappers of kernels.h
// alone on the caller's device buffers, one hook per wrapper, cmtts_internal_k_<name>(<the wrapper's arguments in its order, defaulted ones
// included>, stream).  NOTHING is validated: the arguments reach the wrapper unchanged, so the launch is production's (k_dense_small's 16-slice
// rule, k_conv_post's 16-byte-load rule, k_durations wave against k_durations_serial).  Returns 0; -2 where a bool wrapper (k_ln_linear,
// k_stats_mlp) declined, nothing launched.  The generic conv needs no hook: cmtts_launch_conv (conv_args.h) is exported,
// as are its 16-bit forms cmtts_launch_conv16 (the ResBlock epilogue, or with text_epi the text side's) and cmtts_launch_conv_xt16 (what each refuses: conv_args.h).
// Bitwise contracts these tests hold: k_ln_linear_energy == k_ln_linear + k_energy_embed; k_stats_mlp == three k_dense_small launches;
// conv_post_v4_kernel == conv_post_kernel; durations wave == serial; a durations table of one value == the scalar form.
int cmtts_internal_k_embed_tokens(const int64_t* texts, const int64_t* lens, const float* E, const float* omega, const float* tab, int tab_rows,
                                  float* x, int B, int L, int ld, int C, float scale, void* stream);
int cmtts_internal_k_layernorm_ct(const float* in, float* out, const float* gamma, const float* beta, float eps, const int64_t* lens, int B, int T,
                                  int ld, void* stream);
int cmtts_internal_k_softmax_cols(float* st, const int64_t* lens, int nz, int H, int L, int ld, long zs, void* stream);
int cmtts_internal_k_pos_embed_add(const float* x, float* out, const float* alpha, const float* omega, const float* tab, int tab_rows, int B, int C,
                                   int T, int ld, const int64_t* lens, void* stream);
int cmtts_internal_k_pos_embed_add_lr(const float* src, int ldl, const int64_t* mel2ph, const float* padv, float* out, const float* alpha,
                                      const float* omega, const float* tab, int tab_rows, int B, int C, int T, void* stream);
int cmtts_internal_k_chan_linear(const float* x, const float* W, const float* bias, float* out, const int64_t* lens, int B, int C, int T, int ld,
                                 int O, void* stream);
int cmtts_internal_k_stats_mlp(const float* in, long in_bs, long in_ks, const float* W0, const float* b0, const float* W1, const float* b1,
                               const float* W2, const float* b2, float* out, int B, int K0, int N0, int N1, int N2, void* stream);
int cmtts_internal_k_dense_small(const float* in, long in_bs, long in_ks, const float* Wt, const float* bias, const float* add, float* out, int B,
                                 int K, int N, int act, void* stream);
int cmtts_internal_k_energy_embed(const float* x, const float* e_pred, float* e_scaled, const float* e_target, float e_control, const float* bins,
                                  int nbins, const float* E, float* out1, int64_t* e_idx, int B, int C, int L, int ld, const float* e_table,
                                  void* stream);
int cmtts_internal_k_durations(const float* logd, float d_control, float* d_rounded, int* cum, int64_t* mel_len, int B, int L, void* stream);
int cmtts_internal_k_durations_serial(const float* logd, float d_control, float* d_rounded, int* cum, int64_t* mel_len, int B, int L, void* stream);
int cmtts_internal_k_durations_table(const float* logd, const float* dtab, float* d_rounded, int* cum, int64_t* mel_len, int B, int L, void* stream);
int cmtts_internal_k_durations_table_serial(const float* logd, const float* dtab, float* d_rounded, int* cum, int64_t* mel_len, int B, int L,
                                            void* stream);
int cmtts_internal_k_pitch_table_scale(float* cwt, const int64_t* mel2ph, const int* cum, const float* ptab, int B, int O, int L, int T, void* stream);
int cmtts_internal_k_reduce_partials(const float* part, int nseg, const float* bias, const float* res, const int64_t* lens, float* out, int B, int C,
                                     int L, int ld, void* stream);
int cmtts_internal_k_ln_linear_energy(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* out,
                                      const int64_t* ln_lens, const int64_t* out_lens, int B, int T, int ld, const float* xin, const float* e_target,
                                      float e_control, const float* bins, int nbins, const float* E, float* out1, int64_t* e_idx, float* e_scaled,
                                      const float* e_table, void* stream);
int cmtts_internal_k_ln_linear(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* out,
                               const int64_t* ln_lens, const int64_t* out_lens, int B, int T, int ld, int O, void* stream);
int cmtts_internal_k_cumsum_durations(const float* dur, int* cum, int64_t* mel_len, int B, int L, void* stream);
int cmtts_internal_k_mel2ph(const int* cum, int64_t* mel2ph, int B, int L, int T, void* stream);
int cmtts_internal_k_length_regulate(const float* out1, const int64_t* mel2ph, float* xlr, int B, int C, int ldl, int T, const float* padv,
                                     void* stream);
int cmtts_internal_k_pitch_index(const float* cwt, int O, const float* mean_p, const float* std_p, int stat_ld, float std_scale,
                                 const float* uv_logit, int uv_ld, const uint8_t* uv_mask, float eps, float* r_ws, int64_t* p_idx, float* f0_denorm,
                                 int B, int T, void* stream);
int cmtts_internal_k_gather_add(const float* x, const int64_t* idx, const float* E, float* out, int B, int C, int T, void* stream);
int cmtts_internal_k_lr_gather_add(const float* out1, const int64_t* mel2ph, int ldl, const int64_t* idx, const float* E, float* out, int B, int C,
                                   int T, void* stream);
int cmtts_internal_k_mel_prep(const float* x, const float* scale_b, float scale, float* hin, int B, int T, int M, void* stream);
int cmtts_internal_k_mel_post(const float* F, const float* xold, const float* noise, float c_out, float c_skip, float nstd, float* out, int B, int T,
                              int M, unsigned* flag, void* stream);
// rows: device PostRow [B] (persist_args.h: c_out, c_skip, nstd floats, flags uint32)
int cmtts_internal_k_mel_post_rows(const float* F, const float* xold, const float* noise, const void* rows, float* out, float* out_final, int B,
                                   int T, int M, unsigned* flag, void* stream);
int cmtts_internal_k_diff_embed(const float* t, const float* omega, float* emb, int B, int C, void* stream);
int cmtts_internal_k_conv_post(const float* x, const float* w, const float* bias, float pre_div, float slope, float* wav, int B, int C, int T, int ld,
                               int KW, void* stream);
// Test hook (kernel_hooks.hip; host only, never touches the GPU): sizeof PostRow, PersistGroup, PersistArgs and offsetof thirteen fields of PersistArgs and
// five of PersistGroup (persist_args.h), in the order kernel_hooks.hip lists — what the ctypes mirrors of tests/persist_stack_cases.py are checked against
// before tests/test_gpu_persist_stack.py hands them to the launchers of the persistent stack (exported like those of resblock_args.h).  Writes
// min(n, 21) values, returns 21.
int cmtts_internal_persist_args_layout(size_t* out, int n);
#ifdef __cplusplus
}
#endif
