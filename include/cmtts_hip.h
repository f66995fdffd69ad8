/* cmtts_hip.h — C ABI of the MI355X-native CM-TTS inference hot path (libcmtts_hip.so).
 *
 * The reference (XiangLi2022/CM-TTS) is pure Python/PyTorch and has no FFI; the path sits behind
 * Python callables.  Each entry point below replaces one of those callables and
 * cites it (paths relative to the reference root).  Conventions:
 *   - plain pointers and sizes only, no torch types; every tensor pointer is a DEVICE pointer unless
 *     the parameter is documented as host;
 *   - caller-allocated outputs, caller-provided workspaces (size queries below), no hidden
 *     allocation and no host synchronisation on the hot path;
 *   - `stream` is a hipStream_t passed as void*; the result is ordered on it.  Independent branches of a call may run
 *     on library-owned side streams that are forked from and joined back into `stream` with events before the call
 *     returns control of the data (cmtts_set_option("branch_streams", 0) keeps everything on `stream`);
 *   - like the reference (one Python thread, synthesize.py), the library is NOT thread-safe: process-wide options,
 *     the error string and the persistent-launch admission table are unsynchronised — one host thread per process
 *     (one process per GPU), any number of streams;
 *   - return 0 on success, negative on error (CMTTS_E_*), message via cmtts_last_error();
 *   - integer tensors are int64 (torch.long) like the reference's; activations fp32;
 *   - frame-level activations cross the boundary channel-major ("_ct": [B, C, T], T contiguous) —
 *     the layout the reference itself transposes to before Conv1d (tts_net.py:31-32);
 *     cmtts_transpose() converts to/from the reference's [B, T, C].
 */
#ifndef CMTTS_HIP_H
#define CMTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMTTS_OK 0
#define CMTTS_E_INVALID (-1)      /* bad argument / missing tensor */
#define CMTTS_E_UNSUPPORTED (-2)  /* shape outside what the kernels support */
#define CMTTS_E_HIP (-3)          /* HIP runtime error */
#define CMTTS_E_WORKSPACE (-4)    /* workspace too small */

/* Supported shapes: the kernels are specialised for what the reference's three configs use — hidden = res_channels = 256,
 * 2 attention heads of 128 channels, 80 mel bins (<= 96), <= 32 residual layers, HiFi-GAN V1 (hifigan/config.json).  Anything
 * else returns CMTTS_E_UNSUPPORTED from cmtts_create / cmtts_finalize / the forward calls — never a silent fallback. */
typedef struct cmtts_model cmtts_model;      /* CMTotalTTS weights, packed for the kernels */
typedef struct cmtts_vocoder cmtts_vocoder;  /* hifigan.Generator weights */

/* Hyper-parameters: config/<dataset>/{model,preprocess,train}.yaml of the reference. */
typedef struct cmtts_config {
    int32_t n_symbols, hidden, enc_layers, enc_heads, ffn_kernel;
    int32_t pred_filter, pred_layers, pred_kernel, dur_layers, dur_kernel, cwt_hidden;
    int32_t pitch_bins, energy_bins, use_uv, multi_speaker, external_speaker_dim;
    int32_t n_speaker;   /* > 0: preprocess.yaml speaker_embedder "none" — speaker_emb is nn.Embedding(n_speaker, hidden) indexed by
                            `speakers` (model/cmtts.py:26-38,77-78); 0: nn.Linear(external_speaker_dim, hidden) of spker_embeds */
    int32_t n_mels, res_layers, res_channels;
    float cwt_std_scale, pitch_norm_eps;
    float sigma_min, sigma_max, sigma_data, rho;
} cmtts_config;

const char* cmtts_last_error(void);
const char* cmtts_version(void);
/* Binary-interface revision of this header: bumped whenever a struct layout or an existing signature changes (round 2
 * inserted cmtts_config.n_speaker and the `speakers` parameter of cmtts_text_forward: revision 2; round 3 adds entry
 * points only but starts the counter: 3; round 4 appends the conditioner factors to cmtts_sample_group: 4;
 * round 6: 5 — no layout change, but the MEANING of an existing option value changed in round 5 without a bump: cmtts_model_set_option(m, "winograd", 1) selects
 * the F(4,3) form since then and 2 the F(2,3) form that 1 used to select, and cmtts_poll_error's codes 2 / 3 no longer fail the next launch);
 * 6 — entry points only: the text-state records (cmtts_text_state_*) and cmtts_exchange_records of a sharded synthesis;
 * 7 — entry points only: windowed vocoding for streamed PCM (cmtts_vocoder_halo_frames, cmtts_vocoder_windows_workspace_bytes,
 * cmtts_vocoder_forward_windows);
 * 8 — options only: cmtts_model_set_option / cmtts_vocoder_set_option "batch_invariant" (a host detects support here);
 * still 8 — cmtts_set_control_tables (per-phoneme control tables) is a new entry point and a new struct: no existing layout or
 * signature changes, so the number stays; a host detects it by looking the symbol up (dlsym).  Likewise the resampler
 * (cmtts_resampler_*, cmtts_resample_encode) and cmtts_vocoder_forward_windows_f32: entry points only, still 8; and the duration
 * targets (cmtts_set_duration_targets, a new struct) with cmtts_phoneme_marks: entry points only, still 8.
 * Likewise the loudness measurement (cmtts_loudness_*) and cmtts_resample_encode_gain: entry points only, still 8.
 * Likewise the speaker encoder (cmtts_spkenc_*, a new opaque handle): entry points only, still 8.
 * Likewise the GE2E speaker encoder (cmtts_ge2e_*, a new opaque handle): entry points only, still 8.
 * Likewise the recorded-speech analysis (cmtts_mel_basis, cmtts_analysis_*, cmtts_mel_analysis, cmtts_phoneme_energy, cmtts_pcm_crossfade): still 8.
 * Likewise the alignment of a recording to its phonemes (cmtts_align_*): entry points only, still 8.
 * Likewise the pitch of a recording (cmtts_pitch_*, a new opaque handle): entry points only, still 8.
 * Likewise the objective metrics of a rendering against its recording (cmtts_metric_*): entry points only, still 8.
 * A host compares cmtts_abi_version() with the CMTTS_ABI_VERSION it was built
 * against before it passes a struct (cmtts_amd/_lib.py does at load time). */
#define CMTTS_ABI_VERSION 8
int cmtts_abi_version(void);

/* ---- weight import: replaces torch.load + load_state_dict (synthesize.py:79-83).
 * cmtts_set_tensor takes one entry of CMTotalTTS.state_dict() under its original key and in its
 * original layout (HOST pointer); cmtts_finalize re-packs (k-major / transposed / gate-permuted)
 * and uploads.  Unknown keys (e.g. *_float_tensor buffers) are ignored. */
int cmtts_create(const cmtts_config* cfg, cmtts_model** out);
int cmtts_set_tensor(cmtts_model* m, const char* name, const float* host_data, const int64_t* shape, int ndim);
int cmtts_finalize(cmtts_model* m);
void cmtts_destroy(cmtts_model* m);

/* ---- DurationPitchSpeakerNet.forward, phoneme-level half (model/cmtts.py:44-122 up to the
 * duration rounding, model/modules.py:331-372): text encoder, speaker projection, duration and
 * energy predictors, durations, cumulative sums.  The phoneme-level state needed by
 * cmtts_frame_forward stays in `text_ws`.  Optional outputs may be NULL.
 *   texts int64 [B,L] (0 = pad), src_lens int64 [B], spker_embeds fp32 [B,external_speaker_dim]
 *   (multi-speaker with an external embedder, else NULL), speakers int64 [B] (multi-speaker with n_speaker > 0:
 *   rows of the speaker_emb table, else NULL / ignored).
 *   out: log_d fp32 [B,L], d_rounded fp32 [B,L], mel_len int64 [B], e_pred fp32 [B,L],
 *        e_idx int64 [B,L], enc_out_ct fp32 [B,hidden,L], speaker_emb fp32 [B,hidden]. */
size_t cmtts_text_workspace_bytes(const cmtts_model* m, int B, int L);
int cmtts_text_forward(cmtts_model* m, const int64_t* texts, const int64_t* src_lens, const float* spker_embeds,
                       const int64_t* speakers, int B, int L, float d_control,
                       float* log_d, float* d_rounded, int64_t* mel_len, float* e_pred, int64_t* e_idx,
                       float* enc_out_ct, float* speaker_emb,
                       void* text_ws, size_t text_ws_bytes, void* stream);
/* The same for a RAGGED batch (round 4; BASELINE.json configs[3]): utterances of several padded groups — the bucket groups of a shard —
 * in one call, padded to the longest group's L.  pad_lens int64 [B] (device): the padded phoneme count of each utterance's OWN group;
 * columns l >= pad_lens[b] do not exist for utterance b.  The padded length enters the reference's arithmetic in three places:
 * LayerNorm2 of an FFT block turns a masked (zero) column into its bias vector, which the k = 9 FFN conv reads up to four columns beyond
 * src_len (model/blocks.py:612-615, 539-546); the speaker vector is added to every column of the padded batch
 * (model/modules.py:349-352); the energy predictor runs unmasked over them (:520-554).  All three stop at pad_lens[b]; everything else
 * is column-local or masked by src_lens, so every utterance gets the bits of running its group alone through cmtts_text_forward.  Outputs are [B, L] with L the call's; a group's [Bg, Lg] block is the
 * sub-array rows b0.., columns < Lg (columns >= pad_lens[b] hold unspecified values).  pad_lens NULL = cmtts_text_forward. */
int cmtts_text_forward_ragged(cmtts_model* m, const int64_t* texts, const int64_t* src_lens, const int64_t* pad_lens,
                              const float* spker_embeds, const int64_t* speakers, int B, int L, float d_control,
                              float* log_d, float* d_rounded, int64_t* mel_len, float* e_pred, int64_t* e_idx,
                              float* enc_out_ct, float* speaker_emb,
                              void* text_ws, size_t text_ws_bytes, void* stream);

/* ---- VarianceAdaptor controls and teacher-forced targets (model/modules.py:331-343: p_control, e_control,
 * pitch_target, energy_target, duration_target; d_control is an argument of cmtts_text_forward).  The
 * settings stay on the model until replaced; NULL restores the inference defaults (controls 1, no
 * targets).  All pointers are DEVICE pointers that must stay valid while the forward calls run.
 *   d_target fp32 [B,L]: durations used instead of the predicted ones (:365-367)
 *   e_target fp32 [B,L]: energies bucketized instead of prediction * e_control (:318-328)
 *   cwt_spec fp32 [B,T,10] + f0_mean, f0_std fp32 [B] + uv u8 [B,T]: pitch target (:379-390; f0 from
 *   cwt2f0_norm utils/pitch_tools.py:268-273 with the target statistics; uv only read when use_uv)
 * The predictors still run and their outputs are returned, like the reference. */
typedef struct cmtts_variance_controls {
    float p_control, e_control;
    const float* d_target;
    const float* e_target;
    const float* cwt_spec;
    const float* f0_mean;
    const float* f0_std;
    const uint8_t* uv;
} cmtts_variance_controls;
int cmtts_set_variance_controls(cmtts_model* m, const cmtts_variance_controls* vc);

/* ---- Per-utterance and per-phoneme controls: the three multiplications of the reference (model/modules.py:270 pitch, :326 energy,
 * :369 duration) are elementwise, so a TABLE of factors in place of the scalar is the same model.  d, e, p: fp32 [B, ld] DEVICE
 * pointers, one factor per phoneme (a per-utterance control = one value repeated along its row), valid while the forward calls run;
 * each may be NULL on its own.  ld = the row pitch = the L (L_all) of the next text-side call; another L is CMTTS_E_INVALID there.
 *   d: d_rounded[b,l] = max(rint(exp(log_d[b,l]) - 1) * d[b,l], 0); its integer part feeds the cumulative sums and mel_len as before
 *   e: e_pred[b,l] = prediction * e[b,l], bucketized and returned (like e_control != 1)
 *   p: cwt_out[b,t,:] *= p[b, mel2ph[b,t] - 1] for the frames of the utterance (all columns, the uv logit included, like p_control).
 *      A padding frame (t >= mel_len[b]) takes the factor of the utterance's LAST frame: the f0 normalisation that follows takes its
 *      mean and deviation over all T padded frames (utils/pitch_tools.py cwt2f0_norm), so the scale of the padding rows reaches every
 *      valid frame, and the scalar p_control scales them too — with this rule a per-utterance factor gives, bit for bit, what the
 *      utterance gets from the scalar in a batch of the same shape.  cmtts_text_forward(_ragged) copies p into the text workspace, cmtts_frame_forward* reads it
 *      there: with p installed a text-state record carries the utterance's row as a fifth region (fp32 [L_all], layout word
 *      0x54530002; cmtts_text_state_record_bytes grows accordingly) and cmtts_text_state_unpack restores it, so every rank of a
 *      sharded synthesis must have the same "p installed" state — a frame-side rank needs p != NULL and ld, not the values.
 * A table REPLACES the scalar of its control: a table together with d_control / e_control / p_control != 1 is CMTTS_E_INVALID at the
 * forward call.  Teacher-forced targets keep their precedence (d_target over d, e_target over e; p scales the returned cwt_out
 * also when a pitch target supplies the index, like p_control).  The caller's contract, as for all device data: p > 0 (it scales
 * the uv logit), d >= 0, no NaN; entries at l >= src_lens[b] are ignored.  Without a table every path runs the scalar code.
 * The tables stay on the model until replaced; NULL clears them. */
typedef struct cmtts_control_tables {
    const float* d;
    const float* e;
    const float* p;
    int ld;
} cmtts_control_tables;
int cmtts_set_control_tables(cmtts_model* m, const cmtts_control_tables* t);

/* ---- Duration targets: an utterance, or segments of it (words, a subtitle cue), fitted to an exact number of frames.  The reference has
 * only the multiplier (model/modules.py:369-372), and sum(int(round(exp(log_d) - 1) * d)) is a step function of d that in general hits
 * no given length; the definition is this library's (cmtts_amd/timing.py is its executable form).  With targets
 * installed cmtts_text_forward(_ragged) runs one more kernel behind its durations kernel (the scalar or the table form, so relative
 * emphasis from d_control or a duration table survives).  Per utterance b and segment g with t = target[b, g] >= 0, over the phonemes
 * l < src_lens[b] with seg[b, l] = g in index order, n = max((int)d_rounded, 0) and S = sum n:
 *     q = n t,  a = q / S,  r = q % S,  R = t - sum a      (exact 64-bit integers)
 *     the R phonemes with the largest r get a + 1 frames, the others a; equal r: the lower index first.
 * So the segment has exactly t frames, a phoneme of 0 frames keeps 0, every phoneme is within one frame of n t / S, and t = S changes
 * nothing.  S = 0 leaves the segment as it is; with t > 0 it could not be met and is counted in unmet[b].  d_rounded then holds the
 * INTEGER frame counts (as fp32, every phoneme of the batch, also outside all segments), cum and mel_len their sums; log_d is not
 * touched.  Everything downstream — mel2ph, the length regulator, the pitch table, the text-state records — reads cum and mel_len
 * only, so a fitted length travels through the frame side, the sampler, streaming and a sharded synthesis unchanged.
 *   seg    int32 [B, ld] DEVICE: the segment of each phoneme, -1 = in none (left alone); NULL = one segment per utterance holding all
 *          its phonemes (n_seg must then be 1)
 *   target int32 [B, n_seg] DEVICE: frames per segment, -1 = leave alone
 *   unmet  int32 [B] DEVICE or NULL: written by every text-side call while installed
 *   ld     = the L of the next text-side call; another L is CMTTS_E_INVALID there (and L above 4096, the kernel's LDS)
 * Targets together with a teacher-forced d_target (cmtts_set_variance_controls) are CMTTS_E_INVALID at the forward call: absolute
 * durations leave nothing to fit.  The caller's contract, as for all device data: 0 <= target <= 1 << 24 (a frame count is returned
 * as fp32) or -1; seg in [-1, n_seg); entries at l >= src_lens[b] are ignored.  (A seg value outside the range is treated as -1.)
 * A frame is the model's unit: a length asked for in seconds is met to within half a frame, hop / (2 sampling_rate) s.
 * Without targets the text side's launch sequence is unchanged.  The targets stay on the model until replaced; NULL clears them;
 * the pointers must stay valid while the forward calls run. */
typedef struct cmtts_duration_targets {
    const int32_t* seg;
    const int32_t* target;
    int32_t* unmet;
    int ld, n_seg;
} cmtts_duration_targets;
int cmtts_set_duration_targets(cmtts_model* m, const cmtts_duration_targets* t);
/* Where each phoneme lies in the delivered audio: marks int32 [B, L, 4] DEVICE = start frame, end frame, start sample, end sample.
 * Frames are the cumulative sums of max((int)d_rounded[b, l], 0) over l < src_lens[b] (d_rounded fp32 [B, L] as cmtts_text_forward
 * returned it, src_lens int64 [B]: no text workspace is read), clipped to T when T > 0 (a mel cut at T frames; T = 0: no clipping);
 * samples are ceil(frame * hop * up / down): up / down = output rate / native rate in lowest terms (1, 1 = native), the mapping of
 * the streamed vocoder's chunk offsets (cmtts_resample_encode), so a mark and a chunk offset are on one scale.  Rows l >= src_lens[b]
 * repeat the utterance's end. */
int cmtts_phoneme_marks(const float* d_rounded, const int64_t* src_lens, int B, int L, int T, int hop, int up, int down,
                        int32_t* marks, void* stream);

/* ---- frame-level half (model/modules.py:373-412; LengthRegulator :415-448; dur_to_mel2ph
 * utils/tools.py:768-798; get_pitch_embedding cwt branch :259-317).  T = padded frame count chosen
 * by the host (max(mel_len) like the reference, or a static bucket).
 *   out: cond_ct fp32 [B,hidden,T], mel2ph int64 [B,T], cwt_out fp32 [B,T,10|11] (opt),
 *        f0_denorm fp32 [B,T] (opt), p_idx int64 [B,T] (opt), f0_stats fp32 [B,2] (opt). */
size_t cmtts_frame_workspace_bytes(const cmtts_model* m, int B, int T);
int cmtts_frame_forward(cmtts_model* m, const void* text_ws, int B, int L, int T,
                        float* cond_ct, int64_t* mel2ph, float* cwt_out, float* f0_denorm, int64_t* p_idx,
                        float* f0_stats, void* frame_ws, size_t frame_ws_bytes, void* stream);
/* The same for the sub-batch [b0, b0 + B) of a text workspace filled for B_all utterances padded to L_all phonemes (a bucket group of a
 * ragged shard with its own padded frame count T), and — optionally — with the phoneme-level factor of the conditioner projections:
 *   cond_p1 fp32 [B, res_layers * res_channels, L_all rounded up to 4] (or NULL) = conditioner_projection weights of all residual
 *   layers (model/blocks.py:663,676) applied to the phoneme-level conditioning, no bias.  Since
 *   cond[:, t] = out1[:, mel2ph[t] - 1] + pitch_embed[p_idx[t]] (model/modules.py:373-395), the projections of the frames are
 *   W out1 [:, mel2ph - 1] + (W pitch_embed^T + b)[:, p_idx]: cmtts_sample_factored / cmtts_sample_group expand them from cond_p1,
 *   mel2ph and p_idx instead of running the stacked GEMM over the frames (7 instead of 43 GFLOP per 32 x 512-frame batch; fp32 rounding
 *   differs from the dense product at the 1e-7 level). */
int cmtts_frame_forward_sub(cmtts_model* m, const void* text_ws, int B_all, int L_all, int b0, int B, int T,
                            float* cond_ct, int64_t* mel2ph, float* cwt_out, float* f0_denorm, int64_t* p_idx,
                            float* f0_stats, float* cond_p1, void* frame_ws, size_t frame_ws_bytes, void* stream);
/* cmtts_frame_forward_sub that also returns the phoneme-level factor with the CHANNELS contiguous (round 6):
 *   cond_p1t fp32 [B, res_layers, p1_ld = L_all rounded up to 4, res_channels] (or NULL; needs cond_p1) — the layout the persistent denoiser's
 *   factored instances gather from (16-byte loads of four consecutive channels).  Given here it is written on the library's branch
 *   stream beside the frame-level predictors (a bandwidth-bound copy under MFMA-bound convs); cmtts_sample_factored_t then takes it as it
 *   is, where cmtts_sample_factored transposes cond_p1 at the sampler's entry, in front of the first evaluation (38 us per call at
 *   B = 32 x 88 phonemes).  The same values either way: bit-identical mels. */
int cmtts_frame_forward_sub_t(cmtts_model* m, const void* text_ws, int B_all, int L_all, int b0, int B, int T,
                              float* cond_ct, int64_t* mel2ph, float* cwt_out, float* f0_denorm, int64_t* p_idx,
                              float* f0_stats, float* cond_p1, float* cond_p1t, void* frame_ws, size_t frame_ws_bytes, void* stream);

/* ---- text-side state of single utterances as fixed-size records (new work: the hand-off of a sharded synthesis that starts from
 * text — each rank runs the text side of its slice of the batch, the ranks agree on the frame buckets once the lengths are known, and
 * each utterance's state moves to the rank the plan gives it; the reference synthesizes one padded batch in one process,
 * synthesize.py:195-227).  A record holds, for one utterance of a text workspace filled for L_all phonemes, what
 * cmtts_frame_forward_sub reads: out1 fp32 [hidden][Lp], h128 fp32 [cwt_hidden][Lp], spk fp32 [hidden] (the speaker vector,
 * = the speaker_emb output of the text side for multi-speaker models), cum int32 [L_all] (cumulative rounded durations: d_rounded =
 * its differences) — and, only while a pitch control table is installed (cmtts_set_control_tables), its row fp32 [L_all] with layout
 * 0x54530002 —, behind a 64-byte header { int64 global index, int64 mel_len, int32 src_len, uint32 layout = 0x54530001,
 * int32 L_all, hidden, cwt_hidden, n_regions, 24 bytes zero }; every region starts 16-byte aligned.  The size depends on
 * (config, L_all) only.  Records are plain bytes: any transport may move them between ranks of the same build.
 *   pack: rows int32 [n] (device) = the workspace rows to gather, in record order; global_idx int64 [n] (device, NULL = the row) and
 *   src_lens int64 [B_all] (device, NULL = -1) only fill the header; records [n][record_bytes] (device, 16-byte aligned).  A row
 *   outside [0, B_all) leaves its record untouched.
 *   unpack: scatters n records into rows 0..n-1 of a text workspace of cmtts_text_workspace_bytes(m, n, L_all) bytes;
 *   cmtts_frame_forward_sub(_t)(m, text_ws, n, L_all, b0, B, T, ...) then runs on it unchanged and returns the bits it returns on the
 *   workspace the records came from.
 * Both are single bandwidth-bound launches (one 16 KB chunk of one region of one record per workgroup, 16-byte loads and stores). */
size_t cmtts_text_state_record_bytes(const cmtts_model* m, int L_all);
int cmtts_text_state_pack(cmtts_model* m, const void* text_ws, int B_all, int L_all, const int32_t* rows, int n, const int64_t* global_idx,
                          const int64_t* src_lens, void* records, void* stream);
int cmtts_text_state_unpack(cmtts_model* m, const void* records, int n, int L_all, void* text_ws, size_t text_ws_bytes, void* stream);

/* ---- length regulator alone (LengthRegulator.forward, model/modules.py:446-448): bit-exact
 * gather x_ct [B,C,L] -> out_ct [B,C,T] given fp32 durations [B,L]; also emits mel2ph and mel_len.
 * scratch_cum: int32 [B,L]. */
int cmtts_length_regulate(const float* x_ct, const float* durations, int B, int C, int L, int T,
                          float* out_ct, int64_t* mel2ph, int64_t* mel_len, int32_t* scratch_cum, void* stream);

/* ---- CMDenoiserTTS.forward(x, timesteps, conditioner, speaker_emb, mask) (tts_net.py:29-37;
 * Denoiser.forward model/modules.py:600-639).  x fp32 [B,1,T,80] (already scaled by c_in),
 * timesteps fp32 [B] (= 250 ln sigma), cond_ct fp32 [B,hidden,T], speaker_emb [B,hidden] or NULL,
 * out fp32 [B,1,T,80].  `mask` is ignored by the reference and is not a parameter. */
size_t cmtts_denoiser_workspace_bytes(const cmtts_model* m, int B, int T);
int cmtts_denoiser_forward(cmtts_model* m, const float* x, const float* timesteps, const float* cond_ct,
                           const float* speaker_emb, int B, int T, float* out,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- karras_sample_tts (karras_diffusion.py:480-577) with sampler onestep (:801-811) for
 * n_steps = 1 and stochastic_iterative_sampler (:830-854) as synthesize.py:111-147 calls it for
 * n_steps = 2, 4; KarrasDenoiser.denoise (:392-407) with boundary-condition scalings fused.
 * The noise is an input (random_util.py:17-25 draws it with th.randn on the reference device):
 *   noise fp32 [n_noise,B,1,T,80] N(0,1): noise[0] -> x_T, noise[1+i] -> re-noise after eval i
 *   (n_noise = 1 for n_steps = 1, else n_steps + 1).
 *   sigmas, renoise_std: HOST fp32 [n_steps] (cmtts_schedule fills them).
 *   out mel fp32 [B,T,80]. */
int cmtts_schedule(const cmtts_model* m, int n_steps, float* sigmas_host, float* renoise_std_host);
int cmtts_sample(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb,
                 int B, int T, int n_steps, const float* sigmas_host, const float* renoise_std_host,
                 float* mel, void* ws, size_t ws_bytes, void* stream);
/* cmtts_sample for conditioning that cmtts_frame_forward_sub produced together with its phoneme-level factor: cond_p1 / p1_ld / L /
 * mel2ph / p_idx as described there.  cond_ct stays required (16-bit models and the unfused path read it); cond_p1 NULL = cmtts_sample. */
int cmtts_sample_factored(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb,
                          int B, int T, int n_steps, const float* sigmas_host, const float* renoise_std_host,
                          float* mel, void* ws, size_t ws_bytes, void* stream,
                          const float* cond_p1, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx);
/* ... with cmtts_frame_forward_sub_t's channel-contiguous copy of the factor (cond_p1t NULL = cmtts_sample_factored). */
int cmtts_sample_factored_t(cmtts_model* m, const float* noise, const float* cond_ct, const float* speaker_emb,
                            int B, int T, int n_steps, const float* sigmas_host, const float* renoise_std_host,
                            float* mel, void* ws, size_t ws_bytes, void* stream,
                            const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx);

/* ---- seeded per-utterance sampler noise, generated on the device (noise_philox.hip; the reference's "determ-indiv" generator,
 * model/cm_tool/random_util.py:97-182, in its stronger form: one request — text, speaker, controls, seed — gives one result
 * whatever it is batched with).  The value at (utterance seed, draw, frame, mel bin) is a pure function of those four numbers;
 * B, the row, the padded T, the bucket, the rank and the launch shape do not enter.  The definition (cmtts_amd/noise.py states it in numpy):
 *   bits     Philox4x32-10 with the standard constants (multipliers 0xD2511F53, 0xCD9E8D57; Weyl key increments 0x9E3779B9,
 *            0xBB67AE85; ten rounds; per round c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key bump)
 *   key      the utterance's 64-bit seed: (seed mod 2^32, seed >> 32)
 *   counter  (j mod 2^32, j >> 32, draw, 0x434D5454), j = (t0 + t) * ceil(M / 4) + floor(m / 4): t the frame row of the tensor,
 *            t0 the tensor's first frame, m the mel bin, M = n_mels; element (t, m) is lane m mod 4 of its block
 *   normals  Box-Muller on 24-bit uniforms (every conversion exact in fp32): u1 = ((x_a >> 8) + 1) * 2^-24, u2 = (x_b >> 8) * 2^-24,
 *            r = sqrt(-2 ln u1); lanes 0, 1 = r cos(2 pi u2), r sin(2 pi u2) from (x0, x1), lanes 2, 3 the same from (x2, x3); |z| <= 5.77
 *   draws    the sampler's numbering: draw 0 is x_T, draw 1 + i the re-noise after evaluation i
 *   math     logf, sqrtf, sincospif(2 u2) — full-precision device functions, no fast intrinsics, no fast-math flag
 * How a request seed becomes utterance seeds is the host's business (cmtts_amd/noise.py: utterance_seeds, splitmix64).
 * seeds: DEVICE int64 [B].  out: fp32 [n_draws,B,1,T,M], draws first_draw .. first_draw + n_draws - 1, frames t0 .. t0 + T - 1.
 * One launch.  Null pointers, B / T / M / n_draws < 1, first_draw < 0, t0 < 0: CMTTS_E_INVALID before any launch. */
int cmtts_noise_fill(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, float* out, void* stream);
/* ... for every padded (B, T) group of a ragged shard in ONE launch (t0 = 0): `groups` is a HOST array, the table travels by
 * value in the kernel arguments, 32 groups per launch (more groups = more launches). */
typedef struct cmtts_noise_group {
    const int64_t* seeds;        /* device [B] */
    int32_t B, T;
    float* out;                  /* device [n_draws,B,1,T,M] */
} cmtts_noise_group;
int cmtts_noise_fill_groups(const cmtts_noise_group* groups, int n_groups, int M, int first_draw, int n_draws, void* stream);
/* cmtts_sample_factored_t without a noise argument: x_T = sigma_max * draw 0 is generated straight into the sampler's state and the
 * re-noise draws into the tail of the workspace (one launch, beside the conditioner branch).  The mel has the bits of
 * cmtts_sample_factored_t on the tensor cmtts_noise_fill(seeds, B, T, n_mels, 0, n_noise, 0, ...) writes.
 * ws: cmtts_sample_seeded_workspace_bytes(m, B, T, n_steps) bytes (the denoiser workspace + n_steps noise tensors). */
size_t cmtts_sample_seeded_workspace_bytes(const cmtts_model* m, int B, int T, int n_steps);
int cmtts_sample_seeded(cmtts_model* m, const int64_t* seeds, const float* cond_ct, const float* speaker_emb,
                        int B, int T, int n_steps, const float* sigmas_host, const float* renoise_std_host,
                        float* mel, void* ws, size_t ws_bytes, void* stream,
                        const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx);

/* ---- re-taking spans of an utterance: the masked consistency sampler on frame windows (retake.hip; the
 * definition in numpy: cmtts_amd/retake.py; the image form is the reference's iterative_inpainting, karras_diffusion.py:946-1003).
 * Frames marked in `regen` are sampled again, every other frame of mel_known is KEPT: with z = the seeded noise of the utterance
 * (cmtts_noise_fill's definition at the ABSOLUTE frame, so a window draws what the whole utterance would)
 *   x  = sigma_max * z(draw 0)                                                      every frame, kept ones too
 *   x0 = denoise(x, sigmas[i]); v = regen ? x0 : mel_known; x = v + (z(draw 1 + i) * renoise_std[i]) * 0.85f      i < n_steps - 1
 *   last evaluation: mel_out = x0 (+ the same term when renoise_std[i] >= 0) on regenerated frames; kept frames are mel_known's
 *   values verbatim — nothing is added to them (cmtts_schedule's last renoise_std is ~1e-10, not 0).
 * Each operation is rounded to fp32, nothing is contracted; there is no clamp.  Only the last renoise_std may be negative.
 * The denoiser's output at frame f depends on its input at frames f - res_layers .. f + res_layers only, and kept frames are reset
 * after every evaluation, so the reach does not grow with n_steps: a span is sampled on a WINDOW of the utterance that reaches
 * res_layers frames beyond it.  windows: HOST int32 [N][4] = (utterance b, window start, core_off, core_len), the table format of
 * cmtts_vocoder_forward_windows: window n is frames [start, start + Tw) of utterance b; only regenerated frames inside its core
 * [start + core_off, start + core_off + core_len) are sampled and written back, every other frame of the window is kept.  A core frame
 * closer than res_layers to a window edge that is not 0 or T is computed against zero padding where the whole utterance has frames:
 * keeping cores res_layers away from cut edges, and spans that interact in one core, is the planner's business
 * (cmtts_amd/retake.py: plan_retake_windows).  Tw = T with start 0 is the whole-utterance form.
 * The evaluations run the unchanged denoiser on the gathered [N, Tw] batch with the dense conditioner projections of the window's
 * cond_ct; the seeded noise is drawn inside the one kernel between evaluations (no noise tensor).
 * mel_known, mel_out fp32 [B,T,n_mels] (device): mel_out may BE mel_known (the known frames are gathered before anything is written);
 * otherwise it first receives a device copy of mel_known (partly overlapping buffers are not supported).  regen: DEVICE uint8 [B,T].
 * seeds: DEVICE int64 [B].  A pageable `windows` table is read before the call returns; a page-locked one is copied on `stream`.
 * Validated on the host before anything is launched (CMTTS_E_INVALID, mel_out untouched): null pointers, B / T / N / Tw / n_steps
 * < 1, Tw > T, b outside [0, B), a window outside [0, T], a core outside its window or empty, two cores of one utterance that overlap,
 * a negative renoise_std before the last evaluation, no speaker_emb for a multi-speaker model.  A short workspace: CMTTS_E_WORKSPACE.
 * ws: cmtts_retake_workspace_bytes(m, N, Tw) bytes (0 for N or Tw < 1). */
size_t cmtts_retake_workspace_bytes(const cmtts_model* m, int N, int Tw);
int cmtts_retake(cmtts_model* m, const float* mel_known, const uint8_t* regen, const float* cond_ct, const float* speaker_emb,
                 const int64_t* seeds, int B, int T, const int32_t* windows, int N, int Tw, int n_steps,
                 const float* sigmas_host, const float* renoise_std_host, float* mel_out, void* ws, size_t ws_bytes, void* stream);

/* ---- mixed step counts in one batch: a sampler schedule per utterance (the definition in numpy: cmtts_amd/steps.py).
 * Utterance b takes n_steps[b] >= 1 evaluations with its own sigmas / renoise_std; its result is, by definition, row b of
 * cmtts_sample_seeded / cmtts_sample_factored_t run on that schedule (the reference's loop, karras_diffusion.py:801-811, 830-854, on one
 * row): nothing is new mathematically and the draw numbering stays — draw 0 is x_T, draw 1 + i the re-noise after evaluation i.
 * ORDER: n_steps must be NON-INCREASING in b (cmtts_amd/steps.py: order gives the stable permutation).  Evaluation i then runs on the
 * prefix [0, B_i), B_i = #{b : n_steps[b] > i}, of the batch-major workspace: finished utterances leave — a T = 1 draft batched with T = 4
 * finals costs one evaluation, not four.  An utterance's last evaluation writes its rows straight into `mel`; every row of mel is written
 * exactly once.  The conditioner branch, the factors and the seeded noise (all max_steps draws of all rows) are set up once for the batch.
 * Exactly one of `seeds` (DEVICE int64 [B]: cmtts_sample_seeded's noise) and `noise` (device fp32 [n_noise,B,1,T,n_mels], tensor 0 = x_T's
 * draw, tensor 1 + i the re-noise of evaluation i: max_steps + 1 tensors when a last evaluation re-noises, as cmtts_schedule's do for
 * n > 1, max_steps otherwise) is given.  cond_p1 .. p_idx: the factors of cmtts_sample_factored_t, or NULL / 0.
 * The scalings of every (i, b) are computed on the host by cmtts_sample's fp32 expressions and uploaded once, in one table, before the
 * first launch; a pageable plan is read before the call returns.
 * Step embedding: while all utterances of an evaluation share the timestep (the reference's own schedules: every sigma is sigma_max) the
 * call takes cmtts_sample's path, cached row included; otherwise it computes the embedding per row.  Either way the embedding MLP runs on
 * all B rows of the CALL, never on the shrinking prefix, so its K-slicing (16 slices while 4 * ceil(B / 8) < 128, i.e. B <= 248, else 4)
 * is that of the uniform call on the same batch: the results are the bits of the uniform entry points on the same full batch at every B, and
 * do not depend on the batch size among batches of B <= 248.
 * A plan whose n_steps are all equal and whose columns are all the same IS cmtts_sample_seeded / cmtts_sample_factored_t: same launches,
 * same bits.  With model option "batch_invariant" an utterance's bits do not depend on which evaluations took the persistent stack.
 * Validated on the host before anything is launched (CMTTS_E_INVALID, mel untouched): null pointers, both or neither of seeds and noise,
 * B / T / max_steps < 1, n_steps increasing or outside [1, max_steps], n_steps[0] != max_steps, a negative renoise_std before an
 * utterance's last evaluation, a non-finite or non-positive sigma where one is read, no speaker_emb for a multi-speaker model.  A short
 * workspace: CMTTS_E_WORKSPACE.  "batch_invariant" with the F(2,3) stack: CMTTS_E_UNSUPPORTED, as everywhere.
 * ws: cmtts_sample_mixed_workspace_bytes(m, B, T, max_steps) bytes (0 for a null model or B / T / max_steps < 1): the seeded sampler's
 * workspace + 24 bytes per (evaluation, utterance). */
typedef struct cmtts_step_plan {
    int32_t max_steps;          /* evaluations of the call = n_steps[0] */
    const int32_t* n_steps;     /* HOST [B], 1 <= n_steps[b] <= max_steps, NON-INCREASING in b */
    const float* sigmas;        /* HOST [max_steps][B]; (i, b) read only where i < n_steps[b] */
    const float* renoise_std;   /* HOST [max_steps][B]; < 0 = no re-noise, allowed only at i = n_steps[b] - 1 */
} cmtts_step_plan;
size_t cmtts_sample_mixed_workspace_bytes(const cmtts_model* m, int B, int T, int max_steps);
int cmtts_sample_mixed(cmtts_model* m, const int64_t* seeds, const float* noise, const float* cond_ct, const float* speaker_emb,
                       int B, int T, const cmtts_step_plan* plan, float* mel, void* ws, size_t ws_bytes, void* stream,
                       const float* cond_p1, const float* cond_p1t, int p1_ld, int L, const int64_t* mel2ph, const int64_t* p_idx);

/* ---- the same sampler for a RAGGED shard (BASELINE.json configs[3]: variable-length utterances dealt into static frame buckets;
 * new work — the reference synthesizes one padded batch at a time, synthesize.py:195-227).  Every group is one padded (B, T) batch
 * with its own noise / conditioning / output / workspace (cmtts_denoiser_workspace_bytes(m, B, T)) exactly as cmtts_sample takes
 * them, and its results are those of cmtts_sample on that batch (outputs are defined per padded bucket: model/modules.py:429-430
 * via model/cmtts.py:61-62); but the residual layers of ALL groups run in ONE persistent launch per evaluation, so that
 * buckets too small to fill 256 CUs fill them together.
 *   active_frames: optional HOST int64 [B] (NULL = every frame of the padded batch): the frames of each utterance the caller
 *   will use (its mel_len).  With it the utterance is only computed on its first
 *   ceil((active_frames + tail_frames + res_layers * (n_steps - i)) / 64) 64-frame tiles in evaluation i — an output frame
 *   depends on res_layers frames of input to either side, so every frame below active_frames + tail_frames comes out
 *   BIT-IDENTICAL to the untrimmed result in the direct and F(2,3) forms of the stack, and within fp32 rounding of it (<= 1.5e-5) in the
 *   default F(4,3) form (model option "winograd" below: a quad of frames is rounded from all six inputs of the quad); frames beyond the computed range are unspecified padding — zeros in the one-launch
 *   form, the untrimmed values when the call falls back to cmtts_sample per group (the reference fills them with denoised
 *   padding that every caller slices off: utils/tools.py:575-576, utils/model.py:199-203).
 *   tail_frames: frames beyond active_frames that must still be exact (the receptive field of whatever consumes the padded
 *   mel: 16 covers hifigan.Generator; 0 for mel-only use).
 * Falls back to one cmtts_sample per group when the one-launch form does not apply (16-bit precision modes, tiny shards). */
typedef struct cmtts_sample_group {
    const float* noise;          /* [n_noise,B,1,T,80] */
    const float* cond_ct;        /* [B,hidden,T] */
    const float* speaker_emb;    /* [B,hidden] or NULL */
    int32_t B, T;
    const int64_t* active_frames;/* HOST [B] or NULL */
    float* mel;                  /* out [B,T,80] */
    void* ws;
    size_t ws_bytes;
    /* round 4 (ABI 4), all optional (NULL / 0 = the dense conditioner GEMM on cond_ct): the factors cmtts_frame_forward_sub returned */
    const float* cond_p1;        /* [B, res_layers * res_channels, p1_ld] */
    int32_t p1_ld, L;            /* row stride of cond_p1 (L_all rounded up to 4) and the phoneme count mel2ph indexes into */
    const int64_t* mel2ph;       /* [B,T] */
    const int64_t* p_idx;        /* [B,T] */
} cmtts_sample_group;
int cmtts_sample_ragged(cmtts_model* m, const cmtts_sample_group* groups, int n_groups, int n_steps,
                        const float* sigmas_host, const float* renoise_std_host, int tail_frames, void* stream);

/* ---- hifigan.Generator (hifigan/models.py:112-174) + get_vocoder weight handling
 * (utils/model.py:155-184; weights with weight-norm already folded). */
int cmtts_vocoder_create(cmtts_vocoder** out);
int cmtts_vocoder_set_tensor(cmtts_vocoder* v, const char* name, const float* host_data, const int64_t* shape, int ndim);
int cmtts_vocoder_finalize(cmtts_vocoder* v);
void cmtts_vocoder_destroy(cmtts_vocoder* v);
size_t cmtts_vocoder_workspace_bytes(const cmtts_vocoder* v, int B, int T);
/* Generator.forward: mel_ct fp32 [B,80,T] -> wav fp32 [B,1,256*T] */
int cmtts_vocoder_forward(cmtts_vocoder* v, const float* mel_ct, int B, int T, float* wav,
                          void* ws, size_t ws_bytes, void* stream);
/* vocoder_infer's cast (utils/model.py:195-198): pcm = (wav * max_wav_value).astype(int16) */
int cmtts_wav_to_int16(const float* wav, int16_t* pcm, int64_t n, float max_wav_value, void* stream);

/* ---- streamed PCM: windowed vocoding (DESIGN.md §3 "Streaming").  The generator is purely convolutional: output
 * frame f (samples [256 f, 256 f + 256)) depends on mel frames [f - H, f + H] only, H = cmtts_vocoder_halo_frames(v) (13 for V1).
 * So a mel can be vocoded in windows whose CORES tile each utterance, every window reaching at least H frames beyond its core
 * unless it is clamped at 0 or T (the only places where the whole-mel run sees zero padding): the core samples are those of
 * cmtts_vocoder_forward + cmtts_wav_to_int16 on the whole mel — bitwise in the direct fp32 form ("winograd" 0), within the
 * forms' rounding otherwise (the window batch may take another conv form than the whole batch).
 * cmtts_vocoder_forward_windows: mel_ct fp32 [B,80,T] (device); windows int32 [N][4] = (utterance b, window start, core_off, core_len):
 * window n is mel frames [start, start + Tw) of utterance b (0 <= start, start + Tw <= T), its core frames
 * [start + core_off, start + core_off + core_len) with 1 <= core_len <= core and core_off + core_len <= Tw.  pcm int16 [N, core * 256]
 * (device): row n holds the core's int16 samples, (int16)(int)(tanh(.) * max_wav_value) exactly as cmtts_wav_to_int16, then zeros
 * after a short core.  Only the generator's last layer (conv_post + tanh + the cast) is restricted to the core columns.
 * The table may be device memory or page-locked host memory; it is VALIDATED on the host before anything is launched (a bad
 * argument or window returns CMTTS_E_INVALID and launches nothing; a short workspace CMTTS_E_WORKSPACE).  A device table is
 * read back first, which synchronises `stream`; a page-locked host table is read in place and copied on `stream`, so the
 * caller keeps it unchanged until the call's work has completed.  ws: cmtts_vocoder_windows_workspace_bytes(v, N, Tw) bytes. */
int cmtts_vocoder_halo_frames(const cmtts_vocoder* v);
size_t cmtts_vocoder_windows_workspace_bytes(const cmtts_vocoder* v, int N, int Tw);
int cmtts_vocoder_forward_windows(cmtts_vocoder* v, const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, int core,
                                  int16_t* pcm, float max_wav_value, void* ws, size_t ws_bytes, void* stream);

/* ---- output sample rates and encodings (the definition in executable form: cmtts_amd/resample.py).
 * A resampler is a rational L / M polyphase FIR (output rate = input rate * L / M, L and M coprime) whose taps come from the HOST, so the
 * filter has exactly one definition: taps_host fp32 [2 half + 1], symmetric about index half, on the x L grid.  Output m of an utterance
 * x[0 .. n) is y[m] = sum_j x[j] * taps[m M - j L + half] over the j with a tap, j ascending, fp32 fmaf from 0, x zero outside [0, n);
 * there are ceil(n L / M) outputs.  R = ceil(half / L) = cmtts_resampler_half_width(r) is the filter's half-width in source samples.
 * cmtts_resampler_create builds the phase-major tap table [L][2 R + 1] on the current device (synchronises the null stream once);
 * CMTTS_E_UNSUPPORTED when the table holds more than 65536 floats or 256 outputs span more than 8192 source samples.
 * cmtts_resample_encode: wav fp32 [rows][ld] (device); segments int32 [N][5] = (source row, absolute sample index of that row's element
 * 0, m0, m1, the utterance's valid sample count n): output row i holds the encoded outputs [m0, m1) of its utterance — which need
 * source samples [ceil((m0 M - half) / L), floor(((m1 - 1) M + half) / L)] clipped to [0, n), all of which the row must hold
 * (origin <= first, last < origin + ld) — then zeros up to out_ld.  The phase comes from the absolute m and the summation order does not
 * depend on the segment, so a wave resampled in pieces is BITWISE the wave resampled whole.  out [N][out_ld]: float (CMTTS_ENC_F32),
 * int16 (CMTTS_ENC_S16: (int)(y * max_wav_value) truncated toward zero as cmtts_wav_to_int16 does, but SATURATED to [-32768, 32767] where
 * that cast wraps) or uint8 (CMTTS_ENC_MULAW / CMTTS_ENC_ALAW: ITU-T G.711 of that int16 value).
 * The table may be device memory or page-locked host memory and is VALIDATED on the host before anything is launched, with the contract
 * of cmtts_vocoder_forward_windows (CMTTS_E_INVALID and nothing launched; a device table is read back first, which synchronises `stream`;
 * a page-locked host table is read in place and copied on `stream`, so the caller keeps it unchanged until the call's work has completed).
 * The copy lands in a buffer the resampler owns: calls on one resampler are issued on one stream (or ordered by the caller).
 * cmtts_vocoder_forward_windows_f32: cmtts_vocoder_forward_windows with a float last layer that carries margins — wav_rows fp32
 * [N][(core + 2 margin_frames) * 256]: row n holds tanh(conv_post(.)) for the window-local frames [max(core_off - margin_frames, 0),
 * min(core_off + core_len + margin_frames, Tw)), bitwise the columns of cmtts_vocoder_forward's wav under the conditions above, then
 * zeros.  0 <= margin_frames, and core + 2 margin_frames <= Tw unless Tw == T (a whole-tensor window).  Same table contract, same
 * workspace (cmtts_vocoder_windows_workspace_bytes(v, N, Tw)).  With windows that reach H + 1 frames beyond their cores and margin_frames
 * = 1 the rows hold what cmtts_resample_encode needs for the cores, since R <= 256. */
#define CMTTS_ENC_F32 0
#define CMTTS_ENC_S16 1
#define CMTTS_ENC_MULAW 2
#define CMTTS_ENC_ALAW 3
typedef struct cmtts_resampler cmtts_resampler;
int cmtts_resampler_create(int L, int M, const float* taps_host, int half, cmtts_resampler** out);
void cmtts_resampler_destroy(cmtts_resampler* r);
int cmtts_resampler_half_width(const cmtts_resampler* r);
int cmtts_resample_encode(cmtts_resampler* r, const float* wav, int rows, int64_t ld, const int32_t* segments, int N, int encoding,
                          float max_wav_value, void* out, int64_t out_ld, void* stream);
int cmtts_vocoder_forward_windows_f32(cmtts_vocoder* v, const float* mel_ct, int B, int T, const int32_t* windows, int N, int Tw, int core,
                                      int margin_frames, float* wav_rows, void* ws, size_t ws_bytes, void* stream);

/* ---- loudness measurement and output gain (the definition in executable form: cmtts_amd/loudness.py).
 * Integrated loudness by ITU-R BS.1770 of mono fp32 rows: K-weighting (two biquads derived for `fs` by the bilinear transform; the
 * BS.1770-4 table at 48 kHz), 0.4 s blocks with a 0.1 s hop that lie wholly inside [0, n), the absolute gate at -70 LKFS and the relative
 * gate 10 LU under the absolutely gated mean.  A row shorter than one block is one block [0, n) under the absolute gate alone; an empty
 * row, or one no block of which passes, has L = -inf.  The peak is the SAMPLE peak max |x[0 .. n)|: no true-peak oversampling.
 * fs % 10 == 0 and 8000 <= fs <= 48000, else CMTTS_E_INVALID.
 * cmtts_loudness_coefficients: host only, never touches the GPU: out10 = b0 b1 b2 a1 a2 of the shelf, then of the high-pass, in double.
 * cmtts_loudness_measure: wav fp32 [rows][ld] (device); n_valid int32 [rows] (device or page-locked host memory, read by the kernels on
 * `stream`: keep it unchanged until the call's work has completed; values are clamped to [0, ld]); whatever the rows hold at or beyond
 * n_valid is never used, and a row's result does not depend on the other rows.  target_lufs fp32 [rows] (device) or NULL; ceiling_db: the
 * sample-peak ceiling in dBFS (not NaN).  stats fp32 [rows][4] (device) = (L in LKFS, sample peak, linear gain, number of gated blocks):
 * gain = 10^((target - L) / 20), lowered to 10^(ceiling_db / 20) / peak where peak * gain would exceed the ceiling, and exactly 1 when
 * target_lufs is NULL, the row's target is NaN, L = -inf or the peak is 0 (measure only).  Two launches on `stream`, no allocation, no host
 * synchronisation.  ws: cmtts_loudness_workspace_bytes(rows, ld, fs) bytes (0 for arguments the measurement rejects).  Null pointers, rows
 * or ld < 1, rows > 65535, a bad fs, a NaN ceiling or a workspace that is too small: CMTTS_E_INVALID, checked before any launch.
 * cmtts_resample_encode_gain: cmtts_resample_encode with gains fp32 [rows] (device), indexed by a segment's SOURCE row: every source
 * sample x is replaced by fl32(gains[row] * x) as it is staged — one multiplication per source sample, so pieces stay BITWISE the whole.
 * gains == NULL is cmtts_resample_encode itself.  A ceiling bounds the source samples; the resampled wave can still overshoot between
 * them, which the saturating encoders absorb. */
int cmtts_loudness_coefficients(int fs, double* out10);
int64_t cmtts_loudness_workspace_bytes(int rows, int64_t ld, int fs);
int cmtts_loudness_measure(const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, const float* target_lufs, float ceiling_db,
                           float* stats, void* ws, size_t ws_bytes, void* stream);
int cmtts_resample_encode_gain(cmtts_resampler* r, const float* wav, int rows, int64_t ld, const int32_t* segments, int N, int encoding,
                               float max_wav_value, void* out, int64_t out_ld, const float* gains, void* stream);

/* ---- speaker embeddings from reference audio (the definition in executable form: cmtts_amd/speaker.py).
 * The zero-shot path's first step: the 512-d DeepSpeaker vector of a reference clip, on the device.  Entry points only: CMTTS_ABI_VERSION stays 8.
 * cmtts_spkenc_create / _set_tensor / _finalize / _destroy replace deepspeaker/embedding.py: build_model (DeepSpeakerModel + load_weights,
 *   deepspeaker/conv_models.py:50-135): tensors under their Keras names ("conv64-s/kernel" (5,5,1,64), "conv64-s_bn/moving_variance",
 *   "res3_1_branch_2b/kernel" (3,3,256,256), "affine/kernel" (2048,512), "affine/bias"; a ":0" suffix is accepted), kernels (kh, kw, cin, cout).
 *   finalize folds every BatchNorm (epsilon 1e-3) into its conv in double, packs the MFMA fragment streams and uploads them.
 * cmtts_spkenc_features replaces deepspeaker/audio_ds.py: read_mfcc (34-44) + mfcc_fbank / normalize_frames (126-137) and batcher.py:
 *   sample_from_mfcc (23-29): wav fp32 [rows][ld] (device) at sample rate fs, n_valid int32 [rows] (device; clamped to [0, ld]) ->
 *   info int32 [rows][4] (device) = (first, last, frames, windows) — x[first:last] is what the 95th-percentile trim keeps, (-1, -1, 0, 0) where
 *   it keeps nothing (silence, constant magnitude, one sample above the threshold: the reference raises there) — and the normalised 64-filter
 *   fbank windows fp32 [sum of windows][160][64] (device; room for rows * max_windows), rows in order, zero rows behind an utterance's end.
 *   mode 0: one centred window per row; 1: every window at hop 80 plus one aligned to the end, the first max_windows (<= 64) of them;
 *   2: one window per row at frame offsets int32 [rows] (device; clamped into the utterance).  max_windows must be 1 for modes 0 and 2.
 *   8000 <= fs <= 40000 and 512 < win_length <= 1024 (a 1024-point FFT).  Two launches, no allocation, no host synchronisation.
 * cmtts_spkenc_forward replaces deepspeaker/embedding.py: predict_embedding's model.predict: windows fp32 [W][160][64] (device), row_map int32
 *   [W] (device): the row each window belongs to (an entry outside [0, rows) leaves its window out) -> emb fp32 [rows][512] (device): per row the
 *   L2-normalised mean of its windows' unit-norm embeddings, zeros for a row without windows.  A window's embedding does not depend on the
 *   other windows of the call.  ws: cmtts_spkenc_workspace_bytes(rows, ld, max_windows) bytes cover W <= rows * max_windows (0 for rejected
 *   arguments).  30 launches on `stream`, no allocation, no host synchronisation.
 * Null pointers, rows or ld < 1, an unsupported fs / win_length / mode / max_windows, a workspace that is too small, a handle that is not
 * finalized: CMTTS_E_INVALID, checked before any launch. */
typedef struct cmtts_spkenc cmtts_spkenc;
int cmtts_spkenc_create(cmtts_spkenc** out);
int cmtts_spkenc_set_tensor(cmtts_spkenc* e, const char* name, const float* data, const int64_t* shape, int ndim);
int cmtts_spkenc_finalize(cmtts_spkenc* e);
void cmtts_spkenc_destroy(cmtts_spkenc* e);
size_t cmtts_spkenc_workspace_bytes(int rows, int64_t ld, int max_windows);
int cmtts_spkenc_features(cmtts_spkenc* e, const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, int win_length, int mode,
                          const int32_t* offsets, int max_windows, float* windows, int32_t* info, void* stream);
int cmtts_spkenc_forward(cmtts_spkenc* e, const float* windows, int W, const int32_t* row_map, int rows, float* emb, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- GE2E speaker embeddings from reference audio (the definition in executable form: cmtts_amd/ge2e.py).
 * The zero-shot path's other embedder (preprocess.yaml speaker_embedder: "GE2E"): the 256-d vector of a reference clip, on the device, fp32.
 * Entry points only: CMTTS_ABI_VERSION stays 8.  The reference hands the raw 22 050 Hz waveform over: preprocess_wav (volume normalisation, the
 * webrtcvad silence trim) is not applied on this path and is not part of these calls.
 * cmtts_ge2e_create / _set_tensor / _finalize / _destroy replace ge2e_encoder/inference.py: load_model (SpeakerEncoder + load_state_dict of
 *   checkpoint["model_state"], ge2e_encoder/model.py:12-24): tensors under torch's names — "lstm.weight_ih_l0" (1024, 40), "lstm.weight_hh_l1"
 *   (1024, 256), "lstm.bias_ih_l2" (1024), "linear.weight" (256, 256), "linear.bias"; gate rows in torch's order i, f, g, o.  finalize packs the MFMA
 *   fragment streams, sums the two biases, makes the windowed 551-point DFT table in double and uploads them.
 * cmtts_ge2e_features replaces ge2e_encoder/audio.py: wav_to_mel_spectrogram and, for mode 1, inference.py: compute_partial_slices (58-107) with
 *   the padding rule of embed_utterance (138-141): wav fp32 [rows][ld] (device) at fs = 22050 (anything else: CMTTS_E_INVALID), n_valid int32 [rows]
 *   (device; clamped to [0, ld]) -> info int32 [rows][4] (device) = (n, the zero-padded length, its frames 1 + (n - 1) / 220, windows) and the
 *   40-channel POWER mels (n_fft 551, hop 220, centred, reflect padding, periodic Hann, Slaney triangles on linspace(0, fs / 2, 276); no logarithm).
 *   mode 1: windows fp32 [sum of windows][160][40], rows in order, a row's partials every 80 frames (the last one dropped below 75 % coverage unless
 *   it is the only one), at most max_windows of them; win_lens int32 [windows] = 160.  mode 0: each row's whole spectrogram as one window
 *   [rows][T][40], zero rows at and beyond its frames, win_lens = min(frames, T); max_windows must be 1.  A row with n = 0 has no window.
 *   One launch, no allocation, no host synchronisation.
 * cmtts_ge2e_forward replaces ge2e_encoder/model.py: SpeakerEncoder.forward (41-61) and the mean / norm of embed_utterance (147-149): windows fp32
 *   [W][T][40] (device), lengths int32 [W] (device) or NULL (every window has T frames): a window's state stays as it is from its length on, what
 *   the window holds there is not read into it.  row_map int32 [W] in HOST memory: the row each window belongs to, every entry in [0, rows) ->
 *   emb fp32 [rows][256] (device) = the mean of a row's window embeddings relu(linear(h)) / (norm + 1e-5), divided by its L2 norm (no epsilon, as the
 *   reference; zeros for a row without windows).  row_map NULL (rows == W): the window embeddings themselves, what embed_utterance returns with
 *   using_partials = False.  A window's embedding does not depend on the other windows of the call.  ws: cmtts_ge2e_workspace_bytes(W, T) bytes (0
 *   for rejected arguments; W T 5 KB: the gate pre-activations of one layer).  Seven or eight launches on `stream`, no allocation, no host
 *   synchronisation.  No workgroup of the recurrence waits on another: a tile of windows is one workgroup from its first frame to its last.
 * Null pointers, rows / ld / T < 1, W < 0, a row_map entry out of range, another sample rate or mode, a workspace that is too small, a handle that is
 * not finalized: CMTTS_E_INVALID, checked before any launch. */
typedef struct cmtts_ge2e cmtts_ge2e;
int cmtts_ge2e_create(cmtts_ge2e** out);
int cmtts_ge2e_set_tensor(cmtts_ge2e* e, const char* name, const float* data, const int64_t* shape, int ndim);
int cmtts_ge2e_finalize(cmtts_ge2e* e);
void cmtts_ge2e_destroy(cmtts_ge2e* e);
size_t cmtts_ge2e_workspace_bytes(int W, int T);
int cmtts_ge2e_features(cmtts_ge2e* e, const float* wav, int rows, int64_t ld, const int32_t* n_valid, int fs, int mode, int max_windows, int T,
                        float* windows, int32_t* win_lens, int32_t* info, void* stream);
int cmtts_ge2e_forward(cmtts_ge2e* e, const float* windows, int W, int T, const int32_t* lengths, const int32_t* row_map, int rows, float* emb, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- recorded speech in (the definition in executable form: cmtts_amd/analysis.py).
 * The features the model was trained on, from a waveform, per request and on the device.  Entry points only: CMTTS_ABI_VERSION stays 8.
 * cmtts_mel_basis replaces the librosa filterbank TacotronSTFT builds (preprocessor/preprocessor.py:44-52: Audio.stft.TacotronSTFT): pure
 *   host, never touches the GPU: out fp32 [n_mels][n_fft / 2 + 1], the Slaney filterbank (linear below 1000 Hz at 200 / 3 Hz per mel, logarithmic
 *   above with step ln(6.4) / 27; n_mels + 2 corners equally spaced in mel between fmin and fmax; triangles on linspace(0, fs / 2, bins), each
 *   scaled by 2 / (f[i+2] - f[i])), computed in double, stored as float.
 * cmtts_analysis_create / _destroy: an opaque handle that holds the sparse filterbank, the periodic Hann window and the FFT twiddles on the current
 *   device.  The one STFT geometry every reference config uses — filter_length = win_length = 1024, hop_length = 256, 80 mel channels — with
 *   8000 <= fs <= 48000 and 0 <= fmin < fmax <= fs / 2 (they shape the filterbank only); anything else is CMTTS_E_INVALID, refused before the GPU
 *   is touched.
 * cmtts_mel_analysis replaces preprocessor/preprocessor.py:292, Audio.tools.get_mel_from_wav: wav [rows][ld] (device), fp32 in [-1, 1] (clipped to
 *   that range) or, with is_int16 != 0, int16 taken as x / 32768; n_valid int32 [rows] (device; clamped to [0, ld]).  pad_mode
 *   CMTTS_PAD_REFERENCE: 512 reflected samples on either side, 1 + n / 256 frames for n > 512 — what the acoustic model's mels were made with;
 *   CMTTS_PAD_VOCODER: 384 reflected samples on either side and no centring, n / 256 frames for n > 384, frame f covering samples [256 f, 256 f +
 *   256), the cell the generator emits for it.  A row at or below the minimum has no frames.  Periodic Hann window, 1024-point real DFT,
 *   magnitude sqrt(re^2 + im^2) (no + 1e-9 under the root, in either mode) -> energy fp32 [rows][T] = sqrt(sum of mag^2) per frame, mel =
 *   log(max(basis mag, 1e-5)) as fp32 [rows][T][80] (CMTTS_MEL_TC: what cmtts_retake takes) or [rows][80][T] (CMTTS_MEL_CT: what
 *   cmtts_vocoder_forward takes; the two hold the same bits), frames int32 [rows] = min(the row's frames, T).  At and beyond a row's frames mel
 *   and energy are zero (utils/tools.py: pad_2D / pad_1D).  A frame's bits depend on its samples alone: not on the row, the batch or T.  One
 *   launch on `stream`, no allocation, no host synchronisation.  ws: cmtts_analysis_workspace_bytes(rows, T) bytes (0 for rejected arguments).
 * cmtts_phoneme_energy replaces preprocessor/preprocessor.py:296-305 (phoneme-level average) and 426-437 (normalize): energy fp32 [B][T],
 *   durations int32 [B][L] (device; a negative entry counts as 0) -> out fp32 [B][L] (device): (m - mean) / std with m the mean of the phoneme's
 *   frames [sum d[:l], sum d[:l] + d[l]) — frames ascending, accumulated in double; frames at or beyond T count as zero — and m = 0 for d[l] = 0;
 *   mean, std: stats.json "energy"[2:4], std > 0.  One launch.
 * cmtts_pcm_crossfade (no reference counterpart) joins vocoded windows into a recording: wav_rows fp32 [N][(core + 2 xfade_frames) * hop] as
 *   cmtts_vocoder_forward_windows_f32 wrote them with margin_frames = xfade_frames, rec_rows int16 of the same shape: the recording's samples at
 *   the same positions; table int32 [N][4] (device) = (lead: margin frames the row holds before the core, core frames, trail: margin frames after
 *   it, fades: bit 0 the lead, bit 1 the trail) -> out_rows int16 [N][same].  Core samples: wav * 32768 rounded to nearest, saturated.  A faded
 *   margin (its bit set and all xfade_frames present): rec + w (wav * 32768 - rec), w = (i + 0.5) / (xfade_frames * hop) for the i-th sample from
 *   the fade's outer end, rounded and saturated alike.  Every other sample: rec's bits.  One launch.
 * Null pointers, counts < 1 or rows, B, N > 65535, ld >= 2^30, T > 2^22, an unknown pad_mode or layout: CMTTS_E_INVALID, checked before any
 * launch; a workspace that is too small: CMTTS_E_WORKSPACE. */
#define CMTTS_PAD_REFERENCE 0
#define CMTTS_PAD_VOCODER 1
#define CMTTS_MEL_TC 0
#define CMTTS_MEL_CT 1
typedef struct cmtts_analysis cmtts_analysis;
int cmtts_mel_basis(int fs, int n_fft, int n_mels, double fmin, double fmax, float* out);
int cmtts_analysis_create(int fs, int filter_length, int hop_length, int win_length, int n_mels, double fmin, double fmax, cmtts_analysis** out);
void cmtts_analysis_destroy(cmtts_analysis* a);
size_t cmtts_analysis_workspace_bytes(int rows, int T);
int cmtts_mel_analysis(cmtts_analysis* a, const void* wav, int is_int16, int rows, int64_t ld, const int32_t* n_valid, int pad_mode, int T, int layout,
                       float* mel, float* energy, int32_t* frames, void* ws, size_t ws_bytes, void* stream);
int cmtts_phoneme_energy(const float* energy, int B, int T, const int32_t* durations, int L, double mean, double std, float* out, void* stream);
int cmtts_pcm_crossfade(const float* wav_rows, const int16_t* rec_rows, const int32_t* table, int N, int core, int xfade_frames, int hop,
                        int16_t* out_rows, void* stream);

/* ---- alignment of a recording to its phonemes by dynamic time warping (the definition in executable
 * form: cmtts_amd/align.py; no reference counterpart: the reference takes its durations from Montreal Forced Aligner TextGrids, preprocessor/
 * preprocessor.py:268-282, and compares utterances by DTW only in its evaluation code).  Entry points only: CMTTS_ABI_VERSION stays 8.
 * x fp32 [B][Ts][80] is the model's own rendering of the phonemes (cmtts_sample*), y fp32 [B][Tr][80] the recording's log-mel
 * (cmtts_mel_analysis, CMTTS_MEL_TC), both on the device.  x_len, y_len: int32 [B] in HOST memory, 1 <= x_len[b] <= Ts, 1 <= y_len[b] <= Tr; each
 * call checks them and copies them into its workspace on `stream` (a page-locked array stays valid until the stream has passed the call).
 * cmtts_align_cost: cost fp32 [B][Ts][Tr] (device), c[i][j] = sum_k (x[i][k] - y[j][k])^2 in the difference form; with normalise != 0 each side's
 *   per-channel mean over its valid frames (in double, fixed order) is removed first.  Cells with i >= x_len[b] or j >= y_len[b] are neither read
 *   nor written, in x, y and cost alike.  Two launches (one without normalise).
 * cmtts_align_dtw: ANY fp32 cost [B][Ts][Tr] (device) -> D[0][0] = c[0][0], D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]), every
 *   operation one fp32 add or compare, both ends fixed, no band, no slope constraint; ties go to the diagonal, then (i-1, j), then (i, j-1): a
 *   later candidate wins only if strictly smaller (a NaN never wins).  total fp32 [B] = D[x_len-1][y_len-1], path_len int32 [B] = points of the
 *   path walked back from there (on row 0 it goes left, on column 0 up: at most x_len + y_len - 1 points whatever the matrix holds), row int32
 *   [B][Tr]: for j < y_len[b] the path's point in column j with the smallest c[i][j], ties to the smallest i; entries at or beyond y_len[b] are
 *   not written.  The result has the bits of the definition for every matrix.  Two launches: the cost into the DP's order, then one workgroup per pair.
 * cmtts_align_durations: row as cmtts_align_dtw wrote it (non-decreasing per row; entries are clamped to [0, x_len)), the cost it was made from,
 *   d_syn int32 [B][L] (device): the rendering's frames per phoneme, a negative entry counts as 0 -> d_rec int32 [B][L]: the recording's frames j
 *   whose row[j] lies in the phoneme's frames (sum = y_len[b] when sum d_syn = x_len[b]; 0 for a phoneme of 0 frames), phoneme_cost fp32 [B][L]:
 *   the fp32 sum of c[row[j]][j] over those frames, j ascending, divided by their number; 0 for none.  d_syn_host: the same table in host memory,
 *   or NULL; when given, a negative entry or sum d_syn[b] != x_len[b] is refused.  One launch.
 * ws: cmtts_align_workspace_bytes(B, Ts, Tr) bytes, the same for the three calls (0 for B < 1, B > 65535, a side < 1 or > 4096); it holds the
 *   lengths, the means, the cost in the DP's order and one byte per cell and anti-diagonal step for the walk back (about 5 bytes per cell).
 * Refused before the GPU is touched (CMTTS_E_INVALID, message in cmtts_last_error): a null pointer, a length outside its side, n_mels != 80,
 * L outside [1, 65536], d_syn_host that does not sum to x_len; a workspace that is too small: CMTTS_E_WORKSPACE. */
size_t cmtts_align_workspace_bytes(int B, int Ts, int Tr);
int cmtts_align_cost(const float* x, const int32_t* x_len, int Ts, const float* y, const int32_t* y_len, int Tr, int B, int n_mels, int normalise,
                     float* cost, void* ws, size_t ws_bytes, void* stream);
int cmtts_align_dtw(const float* cost, const int32_t* x_len, const int32_t* y_len, int B, int Ts, int Tr, int32_t* row, float* total,
                    int32_t* path_len, void* ws, size_t ws_bytes, void* stream);
int cmtts_align_durations(const int32_t* row, const float* cost, const int32_t* d_syn, const int32_t* d_syn_host, const int32_t* x_len,
                          const int32_t* y_len, int B, int Ts, int Tr, int L, int32_t* d_rec, float* phoneme_cost, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- pitch of a recording: F0 tracking and the CWT pitch targets (the definition in executable form:
 * cmtts_amd/pitch.py).  Entry points only: CMTTS_ABI_VERSION stays 8.  What comes out is what cmtts_set_variance_controls takes as cwt_spec,
 * f0_mean, f0_std and uv.  The recipes are the public ones (Boersma 1993; Torrence & Compo as pycwt implements them), restated: NOT Praat bit
 * for bit — frame f is centred on sample hop_length * f, the centre of mel frame f of CMTTS_PAD_REFERENCE (the reference shifts Praat's frames
 * by a fixed lpad instead), and the peak is refined by a parabola through three lags (no sinc interpolation).
 * cmtts_pitch_tables: pure host, never touches the GPU: the tables a handle holds, for the CPU tests.  geometry int32 [3] = (W: the window, 3
 *   periods of the floor rounded up to even; LMIN = ceil(fs / ceiling); LMAX = floor(fs / floor)); the others may be NULL: window fp32 [W] =
 *   0.5 - 0.5 cos(2 pi (i + 0.5) / W), r_w double [LMAX + 2]: its autocorrelation over r_w[0], lg fp32 [LMAX + 2] = log2(lag) (lg[0] = 0),
 *   lg_floor = log2(fs / floor), cwt fp32 [10][cwt_n]: the periodised DOG-2 wavelets of transform length cwt_n (a power of two in [4, 4096]).
 *   All made in double, rounded once.
 * cmtts_pitch_create / _destroy: an opaque handle that holds these tables, the CWT's for every length 4 .. 4096, on the current device.
 *   Refused (CMTTS_E_INVALID) before the GPU is touched: fs < 1, hop_length outside [1, 1024], not 0 < floor < ceiling <= fs / 2, W > 2048,
 *   LMAX + 2 > 512.
 * cmtts_pitch_nacf replaces the framing and autocorrelation of parselmouth's Sound.to_pitch_ac (utils/pitch_tools.py:102-104): wav [rows][ld]
 *   (device), fp32 clipped to [-1, 1] or, with is_int16 != 0, int16 taken as x / 32768; n_valid int32 [rows] (device; clamped to [0, ld];
 *   samples at or beyond it are not read).  Frame f < 1 + n / hop_length covers samples [hop f - W / 2, hop f + W / 2), zeros outside the clip:
 *   mean removed, pk fp32 [rows][T] = max |x|, Hann window, a[tau] = sum_i x[i] x[i + tau], r fp32 [rows][T][LMAX + 2] = a[tau] / a[0] / r_w[tau]
 *   (all 0 when a[0] is not positive), frames int32 [rows] = min(the row's frames, T); zeros at and beyond a row's frames.  Fixed summation
 *   order, no atomics: a frame's bits depend on its samples alone.  One launch.
 * cmtts_pitch_track replaces the path finder of to_pitch_ac (voicing threshold 0.6, silence threshold 0.03, octave cost 0.01, octave-jump cost
 *   0.35, voiced / unvoiced cost 0.14, 8 candidates): ANY fp32 r, pk (device), frames int32 [B] (device; clamped to [0, T]) -> lag int32 [B][T]
 *   (0 = unvoiced), f0 fp32 [B][T] = fs / (lag + the vertex of the parabola through r[lag-1 .. lag+1]), 0 where unvoiced; zeros at and beyond a
 *   row's frames.  Candidates, strengths, transitions and tie rules as cmtts_amd/pitch.py states them, every operation one rounded fp32
 *   operation: lag has the bits of the definition for every input, NaN and infinities included.  Two launches.
 * cmtts_pitch_targets replaces preprocessor/preprocessor.py:408-414 (get_cont_lf0, mean / std, get_lf0_cwt): f0 fp32 [B][T] (device; 0 =
 *   unvoiced), frames -> uv uint8 [B][T] = (f0 == 0), the continuous contour (ends filled, interior runs interpolated linearly), its log, f0_mean
 *   and f0_std fp32 [B] (population; in double, fixed order), cwt_spec fp32 [B][T][10] = the real part of the DOG-2 CWT of (lf0 - mean) / std at
 *   scales 0.01 2^j, dt = 0.005, zero-padded to the next power of two >= the row's frames (4 at the least).  status int32 [B]: 0 fine, 1 no
 *   voiced frame, 2 a constant contour (std == 0), 3 fewer than 3 frames; for 1-3 cwt_spec is zeros, f0_std 1 and f0_mean the single log value
 *   (0 for 1 and 3).  A row's result depends on the row alone; zeros at and beyond a row's frames.  One launch.
 * ws: cmtts_pitch_workspace_bytes(B, T) bytes, the same for the three calls (0 for B < 1, B > 65535, T < 1, T > 4096).  No allocation, no
 * host synchronisation.  Null pointers, rows or B outside [1, 65535], T outside [1, 4096] ([3, 4096] for the targets), ld >= 2^30:
 * CMTTS_E_INVALID, checked before any launch; a workspace that is too small: CMTTS_E_WORKSPACE. */
typedef struct cmtts_pitch cmtts_pitch;
int cmtts_pitch_tables(int fs, int hop_length, double floor_hz, double ceiling_hz, int32_t* geometry, float* window, double* r_w, float* lg,
                       float* lg_floor, int cwt_n, float* cwt);
int cmtts_pitch_create(int fs, int hop_length, double floor_hz, double ceiling_hz, cmtts_pitch** out);
void cmtts_pitch_destroy(cmtts_pitch* p);
size_t cmtts_pitch_workspace_bytes(int B, int T);
int cmtts_pitch_nacf(cmtts_pitch* p, const void* wav, int is_int16, int rows, int64_t ld, const int32_t* n_valid, int T, float* r, float* pk,
                     int32_t* frames, void* ws, size_t ws_bytes, void* stream);
int cmtts_pitch_track(cmtts_pitch* p, const float* r, const float* pk, const int32_t* frames, int B, int T, int32_t* lag, float* f0, void* ws,
                      size_t ws_bytes, void* stream);
int cmtts_pitch_targets(cmtts_pitch* p, const float* f0, const int32_t* frames, int B, int T, float* cwt_spec, float* f0_mean, float* f0_std,
                        uint8_t* uv, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- objective metrics of a rendering against the recording it was made from (the definition in
 * executable form: cmtts_amd/metrics.py).  Entry points only: CMTTS_ABI_VERSION stays 8.  They stand in for the reference's evaluation,
 * all_metrics.py: Cal.get_all (SSIM, FFE, MCD), which needs librosa, pyworld, pysptk, fastdtw, pymcd and torchmetrics; the public recipes are
 * restated on the features this library already makes on the device.  The cepstra are the orthonormal DCT-II of the 80-channel natural-log
 * mel of cmtts_mel_analysis, NOT WORLD / SPTK mel-cepstra (all_metrics.py:401-408): an MCD from here is comparable within this project only.
 * Every pointer is device memory unless it says host; x_len, y_len, lens: int32 [B] on the DEVICE (clamped to [1, side]; cmtts_metric_cepstra:
 * [0, T]).  Frames, cells and rows at or beyond a pair's lengths are neither read nor written.  No atomics; a pair's result does not depend
 * on what it is batched with.  No allocation, no host synchronisation.
 * cmtts_metric_dct_table: pure host, never touches the GPU: table fp32 [80][n_cep] (HOST), D[n][0] = sqrt(1/80), D[n][k] = sqrt(2/80)
 *   cos(pi (n + 1/2) k / 80), made in double and rounded once; the caller copies it to the device once.
 * cmtts_metric_cepstra: mel fp32 [B][T][80] -> cepstra fp32 [B][T][n_cep], c[t][k] = sum_n mel[t][n] table[n][k], one fused fp32 chain of 80
 *   terms (within 82 * 2^-24 * sum_n |mel| |D| of the exact sum).  One launch.
 * cmtts_metric_cost replaces log_spec_dB_dist without its constant (all_metrics.py:396-399): cx fp32 [B][Ts][n_cep], cy fp32 [B][Tr][n_cep] ->
 *   cost fp32 [B][Ts][Tr], the layout cmtts_align_dtw takes: c[i][j] = sqrt(sum_{k_lo <= k <= k_hi} (cx[i][k] - cy[j][k])^2) in the difference
 *   form, one fused chain and a correctly rounded square root: relative error <= (K / 2 + 2) * 2^-24, K = k_hi - k_lo + 1; exactly 0 where
 *   both frames are equal.  One launch.  cmtts_align_dtw on this matrix gives row, total and path_len of pymcd's "dtw" mode
 *   (all_metrics.py:447-452); the MCD is (10 sqrt 2 / ln 10) total / path_len.
 * cmtts_metric_diagonal: the frame-by-frame mode (no DTW): total fp32 [B] = the fp32 sum of c[j][j], j ascending, over path_len int32 [B] =
 *   min(x_len, y_len) frames.  One launch.
 * cmtts_metric_f0 replaces metrics/f0_frame_error.py:37-57 and compute_f0_corr / compute_f0_rmse (all_metrics.py:306-333): f0_syn fp32 [B][Ts],
 *   f0_rec fp32 [B][Tr] in Hz with 0 = unvoiced (cmtts_pitch_track), row int32 [B][Tr] as cmtts_align_dtw wrote it (entries clamped to
 *   [0, x_len)) or NULL: row[j] = min(j, x_len - 1).  Over the recording's frames j < y_len with i = row[j]: counts int32 [B][4] = (n = y_len,
 *   n_vv: voiced on both sides, n_gpe: both voiced and |f_syn - f_rec| > 0.2f * f_rec in fp32 — one multiply, one subtract, one compare; the
 *   reference divides: |est / (true + 1e-8) - 1| > 0.2 —, n_vde: exactly one side voiced), bit for bit the definition; vals fp32 [B][3] =
 *   (rmse_cents, mae_cents, corr) over the both-voiced frames with e = 1200 log2(f_syn / f_rec), in double and in the definition's order,
 *   rounded once; NaN for n_vv = 0 and, for corr, a zero variance.  FFE = (n_gpe + n_vde) / n, GPE = n_gpe / n_vv, VDE = n_vde / n.  One launch.
 * cmtts_metric_ssim_prepare replaces all_metrics.py:365-371 on the recording's time axis: a[j] = cx[row[j]][0 .. C), b[j] = cy[j][0 .. C)
 *   (row may be NULL as above), every column divided by its L2 norm over the y_len frames (norm in double: four interleaved partial sums
 *   joined (0 + 1) + (2 + 3); the quotient in double, rounded once; a zero column stays zero) -> u, v fp32 [B][Tr][C], minmax fp32 [B][2] = the
 *   min and max over the pair's u and v.  One launch.
 * cmtts_metric_ssim replaces torchmetrics' StructuralSimilarityIndexMeasure as all_metrics.py:379-387 uses it (Wang et al. 2004: 11 x 11
 *   Gaussian window, sigma 1.5, C1 = (0.01 L)^2, C2 = (0.03 L)^2, only the (y_len - 10) x (C - 10) windows inside the image): range points to
 *   ONE fp32 on the device, the data range L (the reference: max - min over the corpus), so no host synchronisation lies between the two
 *   calls -> ssim fp32 [B]: the five moments, the index and its mean in double, rounded once; NaN for y_len < 11 or C < 11.  Two launches.
 *   ws: cmtts_metric_workspace_bytes(B, Tr, C) bytes (0 for B outside [1, 65535], Tr outside [1, 4096], C outside [1, 80]): one partial sum
 *   per pair and 8 window rows.
 * Refused before the GPU is touched (CMTTS_E_INVALID, message in cmtts_last_error): a null pointer (row excepted), B outside [1, 65535], a
 * side outside [1, 4096], n_mels != 80, n_cep or C outside [1, 80], C > n_cep, not 0 <= k_lo <= k_hi < n_cep; a workspace that is too
 * small: CMTTS_E_WORKSPACE. */
int cmtts_metric_dct_table(int n_mels, int n_cep, float* table);
size_t cmtts_metric_workspace_bytes(int B, int Tr, int C);
int cmtts_metric_cepstra(const float* mel, const int32_t* lens, const float* table, int B, int T, int n_mels, int n_cep, float* cepstra,
                         void* stream);
int cmtts_metric_cost(const float* cx, const int32_t* x_len, int Ts, const float* cy, const int32_t* y_len, int Tr, int B, int n_cep, int k_lo,
                      int k_hi, float* cost, void* stream);
int cmtts_metric_diagonal(const float* cost, const int32_t* x_len, const int32_t* y_len, int B, int Ts, int Tr, float* total, int32_t* path_len,
                          void* stream);
int cmtts_metric_f0(const float* f0_syn, const int32_t* x_len, int Ts, const float* f0_rec, const int32_t* y_len, int Tr, const int32_t* row, int B,
                    int32_t* counts, float* vals, void* stream);
int cmtts_metric_ssim_prepare(const float* cx, const int32_t* x_len, int Ts, const float* cy, const int32_t* y_len, int Tr, const int32_t* row, int B,
                              int n_cep, int C, float* u, float* v, float* minmax, void* stream);
int cmtts_metric_ssim(const float* u, const float* v, const int32_t* y_len, int B, int Tr, int C, const float* range, float* ssim, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- measurement hook (no reference counterpart; the reference's only perf tooling is the
 * wall-clock Timer of p_rtf_cm.py:64-108): HIP events recorded on the launch stream around every
 * stride-th launch of the dominant kernel (the fused residual block of the denoiser) between begin and
 * end, at most max_launches of them.  end() synchronises on the events and returns the summed duration
 * and the number of launches measured.  (Two event records per launch cost ~4 % of a cfg2 step when every
 * launch is bracketed; bench.py samples one launch in seven, which visits every layer.) */
int cmtts_profile_begin(int max_launches, int stride);
/* Selects the fused one-kernel-per-layer residual block (default, 1) or the three-launch form (0) of
 * the denoiser; both are bitwise identical (tests) — the switch exists for A/B measurement.
 * Returns the previous setting. */
int cmtts_set_fused_resblock(int on);
/* Residual layers of the denoiser as ONE persistent launch per utterance chunk (denoiser_persist.hip: the tile's
 * residual stream and skip sum stay in registers for all layers, neighbouring tiles exchange their edge columns
 * in-kernel) instead of one launch per layer.  mode 0 = never, 1 = when it pays (default: more 64-frame
 * tiles than half the CUs, i.e. the per-layer kernels would need a second round of 32-frame tiles), 2 = whenever the shape is supported (an utterance has at most as many 64-frame tiles as the
 * GPU has CUs).  Bitwise identical to the per-layer kernels (tests); fp32 operands only.  Any other value only
 * queries.  Returns the previous mode. */
int cmtts_set_persistent_denoiser(int mode);
/* Asynchronous failures: one pinned host word that kernels set, read and cleared (one atomic exchange) by cmtts_poll_error(): 0, or
 * CMTTS_E_HIP with the message in cmtts_last_error().  Codes:
 *   1  the persistent launch bounds every wait for a neighbouring tile (~2 s); one expired: the kernel poisoned the affected utterance
 *      (its mel comes out NaN, never plausible-but-wrong).  The chip did not hold the whole grid: the NEXT denoiser call checks for
 *      this code before it launches and fails instead.
 *   2  a denoiser evaluation produced a non-finite mel value (any precision mode: the sampler's post-scaling sees every output element).
 *   3  a conv input of the fp16 / fp16x3 residual blocks left the fp16 range (|u| > 65504): that mel is finite and wrong.
 * Codes 2 / 3 describe ONE earlier request's numerics; the word is process-wide (not per model or stream), so they are reported by
 * cmtts_poll_error() only and never fail an unrelated later call (round 6; round 5 refused the next launch for them as well).
 * The word reflects launches that have COMPLETED, so call cmtts_poll_error() after synchronising the stream the mel was produced on
 * (host.py does, at every point where it hands host-visible data back: vocoder_infer, synthesize(sync=True), host.synchronize()).
 * There is no counterpart in the reference (its errors are Python exceptions). */
int cmtts_poll_error(void);
/* Process-wide scheduling options.  None of them changes a result bit (tested); they are per process, not per model or
 * stream.  Returns the previous value (a value outside the option's range only queries) or CMTTS_E_INVALID for an
 * unknown name.
 *   "branch_streams"      1 (default) / 0: independent branches of a call on library-owned side streams / all on `stream`
 *   "resblock_split"      fp32 residual block as two launches over 4x the CUs: 0 never, 1 (default) small batches, 2 always
 *   "step_cache"          1 (default) / 0: cmtts_sample keeps the timestep-only rows of the step embedding on the device
 *   "cooperative_launch"  persistent denoiser through hipLaunchCooperativeKernel: 0 never, 1 every launch, 2 (default)
 *                         automatic — once "process_group" is set the first launch of every (variant, grid) is cooperative
 *                         (the runtime validates that the grid is co-resident and fails the launch otherwise), later launches
 *                         of a validated shape are plain (every cooperative launch drains all queues of the device: +24 % per
 *                         step next to RCCL, profiles/r03_cooperative.md)
 *   "process_group"       1: a communicator / process group exists in this process (set by cmtts_comm_init_rank and by the
 *                         Python host once torch.distributed is initialised)
 * (The switches between a fused kernel and the path it replaces that the bitwise tests flip are not part of the ABI:
 * csrc/internal_hooks.h.) */
int cmtts_set_option(const char* name, int value);
/* Per-handle numerics options: choices that change low-order bits belong to a model, not to the process.
 *   cmtts_model_set_option(m, "ffn2_split", 1 (default) | 0): the FFN linear of the FFT blocks (model/blocks.py:547-551) as
 *       eight K-segment partial GEMMs added in ascending order, or as one launch — two fp32 summation orders.
 *   cmtts_model_set_option(m, "text16", 0 (default) | 1): bf16 / fp16 models only — the four weight contractions of every FFT block (encoder,
 *       decoder: in- / out-projection, FFN conv, FFN linear) and the conv layers of the variance predictors with 16-bit MFMA operands too (LayerNorm, attention scores / softmax / P V, bias,
 *       scale, GELU, residual, mask and accumulation stay fp32).  Off by default because
 *       the text side feeds the integer stages: with it, durations / pitch buckets / lengths may differ from the fp32 model's by one unit.
 *   cmtts_model_set_option(m, "winograd", 1 (default) | 2 | 0): fp32 models, large batches (the persistent denoiser stack, csrc/denoiser_persist.hip):
 *       the gated k = 3 convolution of every residual layer (model/blocks.py:672-679) as a Winograd convolution along the frame axis —
 *       1: F(4,3), 6 products per quad of output frames instead of 12 (round 5); 2: F(2,3), 4 per pair instead of 6 (round 4); transformed
 *       weights formed in double and rounded once, every product and sum in fp32 — or (0) as the direct 3-tap contraction, which is bit for
 *       bit what the per-layer kernels of small batches compute.  The forms differ by fp32 rounding only: F(4,3) <= 1.8e-5 / F(2,3) <= 1e-5 on
 *       one network evaluation, ~8e-6 / ~4e-6 on a T = 4 mel, all equally far from a float64 evaluation at ordinary activation scales
 *       (tests/test_gpu_precision.py; F(4,3) loses a decimal digit on conv inputs of ~6e4); with 1 or 2 an utterance's low-order bits depend on
 *       whether its batch takes the persistent stack.
 *   cmtts_model_set_option(m, "batch_invariant", 0 (default) | 1): fp32 models with "winograd" = 1: the residual layers of batches too small
 *       for the persistent stack (every per-layer route: fused, split, three-launch, the set-aside groups of cmtts_sample_ragged,
 *       cmtts_set_persistent_denoiser(0)) run the stack's F(4,3) form as well (csrc/resblock_split_w43.hip), bit for bit the stack's arithmetic:
 *       an utterance's mel no longer depends on what it was batched with, at the per-layer kernels' latency.  No effect with "winograd" = 0
 *       (every batch already takes the direct form) or on 16-bit models (one form at every shape).  With "winograd" = 2 (F(2,3), which has no
 *       per-layer form) every denoiser call (cmtts_denoiser_forward, cmtts_sample*, cmtts_sample_ragged) returns CMTTS_E_UNSUPPORTED
 *       before it launches anything.
 *   cmtts_vocoder_set_option(v, "batch_invariant", 0 (default) | 1): fp32 generator: every form choice that depends on the launch size takes
 *       its large-launch branch at every size (the Winograd ResBlock convs of "winograd" = 1 included), so that a row's waveform and int16 PCM
 *       do not depend on the batch; large launches are unchanged.  No effect on the 16-bit modes.
 *   cmtts_vocoder_set_option(v, "winograd", 1 (default) | 0): fp32 generator, launches of >= 1024 column tiles (large batches): the k = 3 / 7 / 11
 *       ResBlock convs of the C = 256 and C = 128 stages and the k = 7 / 11 ResBlock convs of the C = 64 stage (hifigan/models.py:96-103) as Winograd convolutions — since round 5
 *       over QUADS of outputs one dilation apart, groups of three taps as F(4,3): 6 / 16 / 24 fp32 products per quad instead of 12 / 28 / 44 (csrc/conv_xlq.hip; dilation 1 and 3, dilation 5 at
 *       C = 256 or k = 3); the remaining dilation-5 convs over PAIRS of outputs, groups of three taps as F(2,3), a remainder of two taps as F(2,2): 4 / 10 / 15 products per pair instead of
 *       6 / 14 / 22 (round 4) — or (0) in the direct form, which small batches always take.  fp32 rounding differences only: <= 1.4e-6 on the waveform, both forms
 *       1.0e-6 from a float64 evaluation (tests/test_gpu_precision.py); with 1 an utterance's int16 samples may differ by one LSB between a
 *       large and a small batch.
 *   cmtts_vocoder_set_option(v, "ups16", 1 (default) | 0): in the 16-bit precision modes the ConvTranspose1d upsamplers take
 *       16-bit operands as well, or stay fp32.
 * Same return convention as cmtts_set_option. */
int cmtts_model_set_option(cmtts_model* m, const char* name, int value);
int cmtts_vocoder_set_option(cmtts_vocoder* v, const char* name, int value);
/* Operand precision of the denoiser's residual-block contractions (93 % of its FLOPs): 0 = fp32 (default,
 * the reference's only inference precision), 1 = bf16, 2 = fp16 MFMA operands with fp32 accumulation;
 * activations in HBM, biases, gate and residual arithmetic stay fp32.  BASELINE.json configs[2]/[4].  In modes 1 / 2 the blocks'
 * conditioner projections take 16-bit operands as well (since round 3, every batch shape; mode 3: (hi, lo) pairs).
 * 3 = "fp16x3": every operand carried as hi = fp16(v), lo = fp16(v - hi) and every product as three fp16 MFMAs
 * (a_lo b_hi + a_hi b_lo + a_hi b_hi, fp32 accumulate): fp32-class accuracy (error vs float64 within 2x of the fp32
 * kernels', tests/test_gpu_precision.py) at 3/16 of the fp32 matrix cost; used by the persistent stack (large
 * batches), other shapes run the exact fp32 kernels. */
int cmtts_set_precision(cmtts_model* m, int mode);
/* Same switch for the HiFi-GAN generator.  Modes 1 / 2 (bf16 / fp16 operands, fp32 accumulate): the 72 ResBlock convs (94 %
 * of the generator's FLOPs) AND, by default, the four ConvTranspose1d upsamplers take 16-bit operands
 * (cmtts_vocoder_set_option(v, "ups16", 0) keeps the upsamplers fp32); inside a ResBlock pair the intermediate xt crosses HBM
 * (or stays in LDS) as convert(leaky_relu(xt)) in 16 bits; the stage tensors (residual stream, MRF sum), conv_pre and conv_post
 * stay fp32.  Mode 3 = fp16x3 as above (fp32-class): ResBlock convs and ("ups16", default) upsamplers with (hi, lo) operand pairs,
 * every HBM tensor fp32. */
int cmtts_vocoder_set_precision(cmtts_vocoder* v, int mode);

/* Tuning knob of the fused residual block: frames per workgroup (0 = automatic: 64 when that still
 * yields >= 512 workgroups, else 32).  Affects speed only, never results. */
int cmtts_set_resblock_tile(int frames);
/* Debug/tuning: when non-NULL, every workgroup of the fused residual block writes 8 int64 s_memtime
 * stamps (phase boundaries) to dev_buf[workgroup*8 ...]; NULL switches it off. */
int cmtts_set_debug_stamps(void* dev_buf);
int cmtts_profile_end(double* total_ms, int* n_launches);

/* ---- FastspeechDecoder.forward (model/modules.py:154-165 = FFTBlocks.forward :80-105 with use_pos_embed=True,
 * learnable pos_embed_alpha): available when the state dict held "decoder.layers.N.op.*", "decoder.layer_norm.*" and
 * "decoder.pos_embed_alpha" (what `self.decoder = FastspeechDecoder(model_config)` registers; CM-TTS defines the class
 * but never instantiates it).  x_ct, out_ct fp32 [B,hidden,T] channel-major; the padding mask is `t >= lens[b]`. */
size_t cmtts_decoder_workspace_bytes(const cmtts_model* m, int B, int T);
int cmtts_decoder_forward(cmtts_model* m, const float* x_ct, const int64_t* lens, int B, int T, float* out_ct,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- the path's one collective (new work: the reference's inference is single-process, synthesize.py:32,43):
 * every rank contributes its padded mel block [Bl,T,M] and mel_len [Bl] and receives all ranks' blocks in rank order.
 * RCCL (librccl.so, the library torch.distributed's "nccl" backend uses on ROCm) is opened at run time with dlopen — the
 * library does not link against it and every other entry point works without it.  A host that is not Python builds its
 * communicator here: rank 0 calls cmtts_comm_unique_id and ships the 128 bytes to the other ranks by any means, every rank
 * calls cmtts_comm_init_rank (one process per GPU, device already selected with hipSetDevice).
 *   cmtts_allgather_mels: mel fp32 [Bl,T,M], mel_len int64 [Bl] (device) -> out_mel fp32 [world*Bl,T,M], out_len int64
 *   [world*Bl] (device); ws = device scratch of cmtts_allgather_workspace_bytes(world, Bl, T, M) bytes (the packed send /
 *   receive buffers: mel_len rides in the same buffer as a trailing column, so it is ONE ncclAllGather); everything is
 *   enqueued on `stream`.  The persistent denoiser needs every CU: issue it after the gather has completed on the stream
 *   (same stream: automatic). */
int cmtts_comm_unique_id(void* id128_host);
int cmtts_comm_init_rank(void** comm, int world, int rank, const void* id128_host);
int cmtts_comm_destroy(void* comm);
size_t cmtts_allgather_workspace_bytes(int world, int Bl, int T, int M);
int cmtts_allgather_mels(void* comm, int world, const float* mel, const int64_t* mel_len, int Bl, int T, int M,
                         float* out_mel, int64_t* out_len, void* ws, size_t ws_bytes, void* stream);
/* The same exchange for end-to-end wav jobs (BASELINE.json configs[4]; SURVEY.md §8e: "cfg5 gathers int16 wav [16, 1024*256]"):
 * what it collates is vocoder_infer's output (utils/model.py:187-205) — pcm int16 [Bl,N] (N = padded frames * hop) and the
 * valid sample count wav_len int64 [Bl] = mel_len * hop (device) -> out_pcm int16 [world*Bl,N], out_len int64 [world*Bl] in
 * rank order.  The count rides in the same buffer (four int16 slots after each row), so it is ONE ncclAllGather of bytes.
 * ws = device scratch of cmtts_allgather_pcm_workspace_bytes(world, Bl, N) bytes. */
size_t cmtts_allgather_pcm_workspace_bytes(int world, int Bl, int64_t N);
int cmtts_allgather_pcm(void* comm, int world, const int16_t* pcm, const int64_t* wav_len, int Bl, int64_t N,
                        int16_t* out_pcm, int64_t* out_len, void* ws, size_t ws_bytes, void* stream);

/* Text-state records to the ranks a length plan gives them (cmtts_text_state_pack above): this rank sends send_counts[p] records
 * to rank p and receives recv_counts[p] records from rank p, both laid out consecutively in rank order — ONE grouped round of
 * ncclSend / ncclRecv with uneven splits, only what each rank needs (no all-gather of every record).  send_counts / recv_counts: HOST
 * int64 [world]; record_bytes = cmtts_text_state_record_bytes.  comm NULL (world 1): the records are copied.  Enqueued on `stream`. */
int cmtts_exchange_records(void* comm, int world, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts,
                           size_t record_bytes, void* stream);

/* ---- get_mask_from_lengths (utils/tools.py:275-283): mask[b][t] = (t >= lens[b]) as one byte per element
 * (True = padding), lens int64 [B], mask [B,W]. */
int cmtts_length_mask(const int64_t* lens, uint8_t* mask, int B, int W, void* stream);

/* ---- layout helper: in [B,R,C] -> out [B,C,R] */
int cmtts_transpose(const float* in, float* out, int B, int R, int C, void* stream);

/* ---- generic Conv1d on the MFMA kernel, exposed for kernel-level parity tests and roofline
 * measurement: y[B,Cout,T] = act(conv1d(x[B,Cin,T], w, bias, padding, dilation)).
 * `packed_w` comes from cmtts_pack_conv_weight (HOST in [Cout,Cin,K] -> DEVICE packed). */
int cmtts_pack_conv_weight(const float* host_w, int Cout, int Cin, int K, float** dev_packed, int* ld);
void cmtts_free_device(void* p);
int cmtts_conv1d(const float* x, const float* packed_w, int ld, const float* bias, int B, int Cin, int Cout,
                 int T, int K, int dilation, int padding, int act, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMTTS_HIP_H */
