// Launch hooks of the frame-side and small kernels (kernels.h): one extern "C" function per k_* wrapper, for tests/test_gpu_frame_kernels.py.
// NOT part of the C ABI (internal_hooks.h).  Every hook hands its arguments to the wrapper unchanged — no validation, no logic: the launch
// under test is the one production makes, grid choice included — and returns 0 (-2 where a bool wrapper declined).  No product path calls one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ge2e.h"
#include "internal_hooks.h"
#include "kernels.h"
#include "persist_args.h"

#define ST (hipStream_t)stream

extern "C" {

int cmtts_internal_k_embed_tokens(const int64_t* texts, const int64_t* lens, const float* E, const float* omega, const float* tab, int tab_rows,
                                  float* x, int B, int L, int ld, int C, float scale, void* stream) {
    k_embed_tokens(texts, lens, E, omega, tab, tab_rows, x, B, L, ld, C, scale, ST);
    return 0;
}
int cmtts_internal_k_layernorm_ct(const float* in, float* out, const float* gamma, const float* beta, float eps, const int64_t* lens, int B, int T,
                                  int ld, void* stream) {
    k_layernorm_ct(in, out, gamma, beta, eps, lens, B, T, ld, ST);
    return 0;
}
int cmtts_internal_k_softmax_cols(float* st, const int64_t* lens, int nz, int H, int L, int ld, long zs, void* stream) {
    k_softmax_cols(st, lens, nz, H, L, ld, zs, ST);
    return 0;
}
int cmtts_internal_k_pos_embed_add(const float* x, float* out, const float* alpha, const float* omega, const float* tab, int tab_rows, int B, int C,
                                   int T, int ld, const int64_t* lens, void* stream) {
    k_pos_embed_add(x, out, alpha, omega, tab, tab_rows, B, C, T, ld, ST, lens);
    return 0;
}
int cmtts_internal_k_pos_embed_add_lr(const float* src, int ldl, const int64_t* mel2ph, const float* padv, float* out, const float* alpha,
                                      const float* omega, const float* tab, int tab_rows, int B, int C, int T, void* stream) {
    k_pos_embed_add_lr(src, ldl, mel2ph, padv, out, alpha, omega, tab, tab_rows, B, C, T, ST);
    return 0;
}
int cmtts_internal_k_chan_linear(const float* x, const float* W, const float* bias, float* out, const int64_t* lens, int B, int C, int T, int ld,
                                 int O, void* stream) {
    k_chan_linear(x, W, bias, out, lens, B, C, T, ld, O, ST);
    return 0;
}
int cmtts_internal_k_stats_mlp(const float* in, long in_bs, long in_ks, const float* W0, const float* b0, const float* W1, const float* b1,
                               const float* W2, const float* b2, float* out, int B, int K0, int N0, int N1, int N2, void* stream) {
    return k_stats_mlp(in, in_bs, in_ks, W0, b0, W1, b1, W2, b2, out, B, K0, N0, N1, N2, ST) ? 0 : -2;
}
int cmtts_internal_k_dense_small(const float* in, long in_bs, long in_ks, const float* Wt, const float* bias, const float* add, float* out, int B,
                                 int K, int N, int act, void* stream) {
    k_dense_small(in, in_bs, in_ks, Wt, bias, add, out, B, K, N, act, ST);
    return 0;
}
int cmtts_internal_k_energy_embed(const float* x, const float* e_pred, float* e_scaled, const float* e_target, float e_control, const float* bins,
                                  int nbins, const float* E, float* out1, int64_t* e_idx, int B, int C, int L, int ld, const float* e_table,
                                  void* stream) {
    k_energy_embed(x, e_pred, e_scaled, e_target, e_control, bins, nbins, E, out1, e_idx, B, C, L, ld, ST, e_table);
    return 0;
}
int cmtts_internal_k_durations(const float* logd, float d_control, float* d_rounded, int* cum, int64_t* mel_len, int B, int L, void* stream) {
    k_durations(logd, d_control, d_rounded, cum, mel_len, B, L, ST);
    return 0;
}
int cmtts_internal_k_durations_serial(const float* logd, float d_control, float* d_rounded, int* cum, int64_t* mel_len, int B, int L,
                                      void* stream) {
    k_durations_serial(logd, d_control, d_rounded, cum, mel_len, B, L, ST);
    return 0;
}
int cmtts_internal_k_durations_table(const float* logd, const float* dtab, float* d_rounded, int* cum, int64_t* mel_len, int B, int L,
                                     void* stream) {
    k_durations_table(logd, dtab, d_rounded, cum, mel_len, B, L, ST);
    return 0;
}
int cmtts_internal_k_durations_table_serial(const float* logd, const float* dtab, float* d_rounded, int* cum, int64_t* mel_len, int B, int L,
                                            void* stream) {
    k_durations_table_serial(logd, dtab, d_rounded, cum, mel_len, B, L, ST);
    return 0;
}
int cmtts_internal_k_pitch_table_scale(float* cwt, const int64_t* mel2ph, const int* cum, const float* ptab, int B, int O, int L, int T,
                                       void* stream) {
    k_pitch_table_scale(cwt, mel2ph, cum, ptab, B, O, L, T, ST);
    return 0;
}
int cmtts_internal_k_reduce_partials(const float* part, int nseg, const float* bias, const float* res, const int64_t* lens, float* out, int B, int C,
                                     int L, int ld, void* stream) {
    k_reduce_partials(part, nseg, bias, res, lens, out, B, C, L, ld, ST);
    return 0;
}
int cmtts_internal_k_ln_linear_energy(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* out,
                                      const int64_t* ln_lens, const int64_t* out_lens, int B, int T, int ld, const float* xin, const float* e_target,
                                      float e_control, const float* bins, int nbins, const float* E, float* out1, int64_t* e_idx, float* e_scaled,
                                      const float* e_table, void* stream) {
    k_ln_linear_energy(x, gamma, beta, eps, W, bias, out, ln_lens, out_lens, B, T, ld, xin, e_target, e_control, bins, nbins, E, out1, e_idx,
                       e_scaled, ST, e_table);
    return 0;
}
int cmtts_internal_k_ln_linear(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* out,
                               const int64_t* ln_lens, const int64_t* out_lens, int B, int T, int ld, int O, void* stream) {
    return k_ln_linear(x, gamma, beta, eps, W, bias, out, ln_lens, out_lens, B, T, ld, O, ST) ? 0 : -2;
}
int cmtts_internal_k_cumsum_durations(const float* dur, int* cum, int64_t* mel_len, int B, int L, void* stream) {
    k_cumsum_durations(dur, cum, mel_len, B, L, ST);
    return 0;
}
int cmtts_internal_k_mel2ph(const int* cum, int64_t* mel2ph, int B, int L, int T, void* stream) {
    k_mel2ph(cum, mel2ph, B, L, T, ST);
    return 0;
}
int cmtts_internal_k_length_regulate(const float* out1, const int64_t* mel2ph, float* xlr, int B, int C, int ldl, int T, const float* padv,
                                     void* stream) {
    k_length_regulate(out1, mel2ph, xlr, B, C, ldl, T, ST, padv);
    return 0;
}
int cmtts_internal_k_pitch_index(const float* cwt, int O, const float* mean_p, const float* std_p, int stat_ld, float std_scale,
                                 const float* uv_logit, int uv_ld, const uint8_t* uv_mask, float eps, float* r_ws, int64_t* p_idx, float* f0_denorm,
                                 int B, int T, void* stream) {
    k_pitch_index(cwt, O, mean_p, std_p, stat_ld, std_scale, uv_logit, uv_ld, uv_mask, eps, r_ws, p_idx, f0_denorm, B, T, ST);
    return 0;
}
int cmtts_internal_k_gather_add(const float* x, const int64_t* idx, const float* E, float* out, int B, int C, int T, void* stream) {
    k_gather_add(x, idx, E, out, B, C, T, ST);
    return 0;
}
int cmtts_internal_k_lr_gather_add(const float* out1, const int64_t* mel2ph, int ldl, const int64_t* idx, const float* E, float* out, int B, int C,
                                   int T, void* stream) {
    k_lr_gather_add(out1, mel2ph, ldl, idx, E, out, B, C, T, ST);
    return 0;
}
int cmtts_internal_k_mel_prep(const float* x, const float* scale_b, float scale, float* hin, int B, int T, int M, void* stream) {
    k_mel_prep(x, scale_b, scale, hin, B, T, M, ST);
    return 0;
}
int cmtts_internal_k_mel_post(const float* F, const float* xold, const float* noise, float c_out, float c_skip, float nstd, float* out, int B, int T,
                              int M, unsigned* flag, void* stream) {
    k_mel_post(F, xold, noise, c_out, c_skip, nstd, out, B, T, M, flag, ST);
    return 0;
}
int cmtts_internal_k_mel_post_rows(const float* F, const float* xold, const float* noise, const void* rows, float* out, float* out_final, int B,
                                   int T, int M, unsigned* flag, void* stream) {
    k_mel_post_rows(F, xold, noise, static_cast<const PostRow*>(rows), out, out_final, B, T, M, flag, ST);
    return 0;
}
int cmtts_internal_k_diff_embed(const float* t, const float* omega, float* emb, int B, int C, void* stream) {
    k_diff_embed(t, omega, emb, B, C, ST);
    return 0;
}
int cmtts_internal_k_conv_post(const float* x, const float* w, const float* bias, float pre_div, float slope, float* wav, int B, int C, int T, int ld,
                               int KW, void* stream) {
    k_conv_post(x, w, bias, pre_div, slope, wav, B, C, T, ld, KW, ST);
    return 0;
}
// the GE2E encoder's launches alone (ge2e.h; tests/test_gpu_ge2e.py): the launcher's status is the hook's (-2: an argument no instance covers)
int cmtts_internal_ge2e_layer(const float* x, int N, int T, int K, const float* wih, const float* whh, const float* bias, const int32_t* lens, int tile,
                              float* pre, float* hseq, float* hlast, void* stream) {
    return cmtts_launch_ge2e_layer(x, N, T, K, wih, whh, bias, lens, tile, pre, hseq, hlast, stream);
}
int cmtts_internal_ge2e_tail(const float* hlast, int W, const float* lin_t, const float* lin_b, float* emb_w, const int32_t* row_map, int rows,
                             float* emb, void* stream) {
    return cmtts_launch_ge2e_tail(hlast, W, lin_t, lin_b, emb_w, row_map, rows, emb, stream);
}
// persist_args.h as THIS compiler lays it out (host only, no logic): tests/persist_stack_cases.py mirrors the three structs in ctypes and the
// launchers of the persistent stack take PersistArgs from it.  out[0..2] = sizeof PostRow, PersistGroup, PersistArgs; then offsetof PersistArgs'
// W3f, halo, cp_bstride, tail, skip_div, post_rows, fact, p1t, wino, xst, n_groups, grp, desc; then PersistGroup's cp_bstride, B, p1, ldp, xst.
// Writes min(n, 21) values and returns how many there are.
int cmtts_internal_persist_args_layout(size_t* out, int n) {
    const size_t v[] = {sizeof(PostRow), sizeof(PersistGroup), sizeof(PersistArgs),
                        offsetof(PersistArgs, W3f), offsetof(PersistArgs, halo), offsetof(PersistArgs, cp_bstride), offsetof(PersistArgs, tail),
                        offsetof(PersistArgs, skip_div), offsetof(PersistArgs, post_rows), offsetof(PersistArgs, fact), offsetof(PersistArgs, p1t),
                        offsetof(PersistArgs, wino), offsetof(PersistArgs, xst), offsetof(PersistArgs, n_groups), offsetof(PersistArgs, grp),
                        offsetof(PersistArgs, desc),
                        offsetof(PersistGroup, cp_bstride), offsetof(PersistGroup, B), offsetof(PersistGroup, p1), offsetof(PersistGroup, ldp),
                        offsetof(PersistGroup, xst)};
    const int have = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < have; ++i) out[i] = v[i];
    return have;
}

}  // extern "C"
