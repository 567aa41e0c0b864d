/*
 * ttship — MI355X-native Tacotron2-DDC + MultiBand-MelGAN inference path, C ABI.
 *
 * Drop-in boundary. The reference has no FFI/plugin registry: its boundary is
 * nn.Module duck typing. Each entry point below replaces one reference call, cited as
 * path:line relative to the reference checkout:
 *
 *   tts_taco_set_tensor/finalize  <- Tacotron2.load_state_dict(cp['model'])
 *                                    (TTS/server/synthesizer.py:68-79, TTS/tts/utils/io.py:9-24)
 *   tts_taco_infer                <- Tacotron2.inference(text)  (TTS/tts/models/tacotron2.py:142-163)
 *   tts_taco_infer_spk            <- Tacotron2.inference(text, speaker_ids | speaker_embeddings)
 *                                    with decoder.set_r / max_decoder_steps (layers/tacotron2.py:209,156)
 *   tts_taco_forward              <- Tacotron2.forward(text, text_lengths, mel_specs, mel_lengths) in eval():
 *                                    the teacher-forced decode (models/tacotron2.py:95-140,
 *                                    layers/tacotron2.py:300-333)
 *   tts_taco_style_mel / _tokens  <- gst_layer(style_mel, speaker_embedding) / compute_gst with a token dict
 *                                    (TTS/tts/layers/gst_layers.py, tacotron_abstract.py:184-203)
 *   tts_taco_infer_style / tts_taco_forward_style <- the two calls above on a model with gst=True
 *   tts_taco_encoder              <- embedding + Encoder.inference (models/tacotron2.py:144-145,
 *                                    layers/tacotron2.py:112-119)
 *   tts_taco_postnet              <- Postnet + residual (models/tacotron2.py:159-160)
 *   tts_taco_decoder_state        <- the decoder state the reference leaves on `self` after inference
 *                                    (query, attention_rnn_cell_state, decoder_hidden, decoder_cell,
 *                                    context, attention_weights(_cum): layers/tacotron2.py:217-233,
 *                                    259-298; common_layers.py:251-260): per-stage decoder parity
 *   tts_melgan_set_tensor/finalize<- MultibandMelganGenerator.load_state_dict + remove_weight_norm
 *                                    (TTS/server/synthesizer.py:81-91, melgan_generator.py:91-97)
 *   tts_melgan_infer              <- MultibandMelganGenerator.inference (multiband_melgan_generator.py:32-39)
 *   tts_melgan_infer_strided      <- the same on a (B, M, C) tensor viewed as (B, C, M) (no transposed copy)
 *   tts_melgan_generator          <- MelganGenerator.layers(c) (melgan_generator.py:28-81)
 *   tts_pqmf_synthesis            <- PQMF.synthesis (TTS/vocoder/layers/pqmf.py:51-56)
 *   tts_taco_mbmelgan_infer       <- Tacotron2.inference then MultibandMelganGenerator.inference on its
 *                                    postnet output (TTS/server/synthesizer.py:150-159), one call
 *   tts_taco_mbmelgan_submit/finish <- the same, returning once the decode's results are on the host
 *                                    (the vocoder still running), completed by finish
 *   tts_mel_to_linear / tts_griffin_lim <- AudioProcessor.inv_melspectrogram on a batch
 *                                    (TTS/utils/audio.py:213-214, 241-248, 259-279)
 *   tts_stft_mag / tts_mag_to_feature <- AudioProcessor.spectrogram / melspectrogram on a batch of
 *                                    waveforms (TTS/utils/audio.py:108-124, 198-230, 259-267)
 *   tts_pqmf_analysis             <- PQMF.analysis (TTS/vocoder/layers/pqmf.py:48-49)
 *   tts_stft_pair_sums / tts_torch_stft_mag <- STFTLoss / TorchSTFT, evaluation only
 *                                    (TTS/vocoder/layers/losses.py:7-52)
 *
 * Conventions: every function returns 0 on success and nonzero on failure; the message is
 * available from tts_last_error() (thread-local). Pointers prefixed d_ are device (HIP) memory
 * owned by the caller; h_ are host memory. `stream` is a hipStream_t (NULL = default stream);
 * work is ordered after prior work on `stream` and later work on `stream` is ordered after it.
 * Tensors are fp32, C-contiguous, in the layouts documented per function.
 *
 * Threads: a context may be shared by host threads. Every entry point that takes a context holds
 * that context's (recursive) mutex for the whole call, so calls on one context run one at a time;
 * sequences that must not interleave (load a model then infer with it, glow_encode then
 * glow_decode) need a caller-side lock around them (the Python layer's Engine.lock). Different
 * contexts (one per device) run concurrently. The reference model is not re-entrant at all
 * (per-call state on self: TTS/tts/layers/tacotron2.py:221-233).
 *
 * Host synchronisation: tts_taco_infer(_spk) returns per-utterance step counts and so waits for
 * its work. In the default split-f16 GEMM mode every other compute entry (postnet, melgan,
 * pwgan, glow) also ends with one hipStreamSynchronize on its stream, to read the range flag and
 * re-run the call on the fp32 kernels if an operand left the f16 range (a NaN input counts as out
 * of range and runs the call twice). With tts_set_gemm_mode(ctx, 0) those entries stay
 * stream-asynchronous. INTEGRATION.md §3.
 *
 * Device use: the persistent kernels need every one of their workgroups resident at once (one per
 * CU); another process or stream keeping kernels on the same GPU during a call can delay them
 * past the barrier wait limit below, and the call then fails (retryable).
 *
 * Grid barriers: the persistent decoder / BiLSTM / GE2E kernels give up a barrier wait after
 * TTS_BARRIER_TIMEOUT_MS (environment, default 2000) and the call returns an error; nothing is
 * left half-written that a retry depends on, so retrying the call is safe.
 */
#ifndef TTSHIP_H
#define TTSHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tts_ctx tts_ctx;

int tts_version(void);
const char* tts_last_error(void);

/* One context per (process, device). Owns packed weights, workspace and captured graphs. */
int tts_ctx_create(int device, tts_ctx** out);
int tts_ctx_destroy(tts_ctx* ctx);

/* ---- Tacotron2 (DDC LJSpeech architecture; coarse_decoder.* accepted and ignored) ---- */
/* Register one state_dict tensor by its reference key, fp32 host data. */
int tts_taco_set_tensor(tts_ctx* ctx, const char* name, const float* h_data, const int64_t* shape, int ndim);
/* Fold BatchNorm, permute/swizzle and upload. attn_norm: 0 = sigmoid, 1 = softmax.
   r_init = reduction factor the model was constructed with (projection width 80*r_init). */
int tts_taco_finalize(tts_ctx* ctx, int num_chars, int r_init, int attn_norm);

/* Batched Tacotron2.inference. Output i equals the reference B=1 call on utterance i.
   d_ids      (B, T_max) int64 token ids; row b valid for t < h_lens[b] (1 <= h_lens[b] <= T_max)
   r          reduction factor in use (1 <= r <= r_init)
   h_max_steps per-utterance max_decoder_steps (>= 1); S_cap >= max(h_max_steps)
   d_dec, d_post (B, S_cap*r, 80): frames [0, steps_b*r) valid, rest zero
   d_align    (B, S_cap, T_max);  d_stop (B, S_cap) sigmoid(stop logit)
   h_steps    out: decoder steps taken per utterance; h_status out: 1 stopnet, 2 max steps */
int tts_taco_infer(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                   const int32_t* h_max_steps, int S_cap, float stop_threshold, float* d_dec, float* d_post,
                   float* d_align, float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream);

/* Multi-speaker Tacotron2.inference(text, speaker_ids=..., speaker_embeddings=...)
   (TTS/tts/models/tacotron2.py:142-156; speaker vector concatenated to the encoder outputs,
   tacotron_abstract.py:213-217). Exactly one of d_spk_ids (int64 (B), rows of the learned
   speaker_embedding table) or d_spk_emb (float (B, spk_dim), external per-sample embeddings) is
   non-null. At most 64 utterances per call, conditioning vectors of at most 1024 dims. Other arguments
   as tts_taco_infer. */
int tts_taco_infer_spk(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                       const int32_t* h_max_steps, int S_cap, float stop_threshold, const int64_t* d_spk_ids,
                       const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                       int32_t* h_steps, int32_t* h_status, void* stream);

/* Teacher-forced Tacotron2.forward(text, text_lengths, mel_specs, mel_lengths, speaker_ids,
   speaker_embeddings) of a model in eval() (TTS/tts/models/tacotron2.py:95-140,
   layers/tacotron2.py:300-333; notebooks/ExtractTTSpectrogram.ipynb): the decode driven by the
   ground-truth mel. Output i equals the reference B=1 call on row i alone, on its own
   S_i r frames, S_i = ceil(h_mel_lens[i] / r).
   d_mel      (B, M_max, 80) float, 16-byte aligned; M_max a multiple of r. Step t >= 1 of row b reads
              frame d_mel[b][t r - 1] (t < S_b, so never a frame at or past h_mel_lens[b])
   h_mel_lens per-row mel lengths, 1 <= h_mel_lens[b] <= M_max; rows take exactly S_b steps (no stop rule)
   d_spk_ids / d_spk_emb as tts_taco_infer_spk (both NULL: single-speaker model)
   d_dec, d_post (B, M_max, 80): frames [0, h_mel_lens[b]) valid, rest zero (the output mask; the
              postnet runs over the row's S_b r masked frames)
   d_align    (B, M_max / r, T_max), d_stop (B, M_max / r) RAW stopnet logits; zero for steps >= S_b
   Plain location attention only (windowing, forward and Graves attention: an error), on the
   persistent decoder only (an error where it is not in use), at most 64 rows per call. */
int tts_taco_forward(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                     const float* d_mel, const int32_t* h_mel_lens, int M_max, const int64_t* d_spk_ids,
                     const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                     void* stream);

/* ---- Global Style Tokens (TTS/tts/layers/gst_layers.py; tacotron_abstract.py:184-203) ----
   A multi-speaker Tacotron2 loaded with gst_layer.* tensors concatenates a style vector of
   gst_dim to every encoder output, in front of the speaker vector (models/tacotron2.py:147-155).
   tts_taco_speaker_dim then reports gst_dim + the speaker vector's width (the conditioning
   width); gst_dim is reported here. query_uses_speaker: the style attention's W_query has speaker
   columns (gst_use_speaker_embedding with external embeddings). gst_dim 0: no gst_layer. */
int tts_taco_gst_info(tts_ctx* ctx, int* gst_dim, int* num_tokens, int* query_uses_speaker);

/* gst_layer(mel, speaker_embedding): reference encoder + style-token attention.
   d_mel      (B, N_max, 80) float; row b holds h_lens[b] frames (1 <= h_lens[b] <= N_max <= 65536),
              nothing past them is read; B <= 64
   d_spk_emb  (B, Es) when query_uses_speaker, else NULL (ignored)
   d_style    out (B, gst_dim). Row b equals the reference B=1 call on d_mel[b, :h_lens[b]], bit for
              bit whatever batch it sits in. Stream-asynchronous. */
int tts_taco_style_mel(tts_ctx* ctx, const float* d_mel, const int32_t* h_lens, int B, int N_max,
                       const float* d_spk_emb, float* d_style, void* stream);

/* compute_gst with a {token: weight} dict: d_style (gst_dim) = sum_i h_weights[i] W_value tanh(token
   h_token_ids[i]), added in the order given (n <= 64; n = 0: zeros). An index outside
   [0, num_tokens) is an error. */
int tts_taco_style_tokens(tts_ctx* ctx, const int32_t* h_token_ids, const float* h_weights, int n, float* d_style,
                          void* stream);

/* tts_taco_infer_spk / tts_taco_forward with the rows' style vectors d_style (B, gst_dim), caller
   row order; NULL = zeros (style_mel=None). A non-NULL d_style on a model without gst_layer is an
   error. The older entries are these with NULL. */
int tts_taco_infer_style(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                         const int32_t* h_max_steps, int S_cap, float stop_threshold, const int64_t* d_spk_ids,
                         const float* d_spk_emb, const float* d_style, float* d_dec, float* d_post, float* d_align,
                         float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream);
int tts_taco_forward_style(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                           const float* d_mel, const int32_t* h_mel_lens, int M_max, const int64_t* d_spk_ids,
                           const float* d_spk_emb, const float* d_style, float* d_dec, float* d_post, float* d_align,
                           float* d_stop, void* stream);

/* Decoder options that no tensor reveals (layers/tacotron2.py:147-200 -> common_layers.py:196-372):
   attention windowing at inference (attn_win) and forward attention (forward_attn; the transition
   agent is on when decoder.attention.ta.* tensors are loaded). BN prenet is detected from the
   decoder.prenet.linear_layers.N.batch_normalization.* tensors. Variants decode on the persistent
   decoder only. forward_attn_mask keeps the forward alignment to [n-1, n+2] around the shifted
   previous argmax n (common_layers.py:309-318). Set before tts_taco_infer; kept across finalize. */
int tts_taco_set_options(tts_ctx* ctx, int windowing, int forward_attn, int forward_attn_mask);

/* speaker dimension of the finalized model (0 = single speaker) and its learned table size */
int tts_taco_speaker_dim(tts_ctx* ctx, int* spk_dim, int* num_speakers);

/* encoder outputs (B, T_max, 512), zero for t >= h_lens[b] */
int tts_taco_encoder(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max,
                     float* d_out, void* stream);

/* postnet(dec) + dec on time-major (B, M_max, 80) frames, valid for t < h_lens[b] */
int tts_taco_postnet(tts_ctx* ctx, const float* d_dec, const int32_t* h_lens, int B, int M_max, float* d_out,
                     void* stream);

/* Decoder state after the last decoder step of the previous tts_taco_infer* call on this context
   (persistent decoder path), rows in the caller's order: attention_rnn h and c (B, 1024),
   decoder_rnn h and c (B, 1024), context (B, 512), attention weights and cumulative weights
   (B, T_max). Rows that stopped before the call's last step hold the state the batched decode left
   in them, not their own final state: compare rows that ran the call's full step count. Any output
   pointer may be NULL (skipped). B and T_max size the caller's buffers and must equal the last
   decode's batch and encoder length (an error otherwise, nothing written). In split-f16 mode
   (tts_set_gemm_mode 1) the persistent decoder publishes attention_rnn h, decoder_rnn h and the
   context pre-split as f16 hi / lo halves; those three outputs are rebuilt as hi + 2^-11 lo, the
   value the next step's GEMMs consume (about 22 significant bits, within ~2^-22 relative of the
   fp32 value), not the unrounded fp32 state. The cell states and attention weights are fp32. */
int tts_taco_decoder_state(tts_ctx* ctx, int B, int T_max, float* d_att_h, float* d_att_c, float* d_dec_h,
                           float* d_dec_c, float* d_context, float* d_alpha, float* d_alpha_cum, void* stream);

/* ---- Tacotron (v1): CBHG encoder, GRU decoder, CBHG postnet (TTS/tts/models/tacotron.py) ----
   Single speaker, no GST, original location-sensitive attention, original prenet.
   tts_tacotron1_set_tensor/finalize <- Tacotron(...).load_state_dict: tensors by their reference keys
                       (coarse_decoder.* / decoder_backward.* are not needed); BatchNorm is folded at
                       finalize. r_init = the constructor's r (proj_to_mel has 80 * r_init rows),
                       memory_size as given to the constructor (<= 0: the prenet reads the last frame;
                       at most 32), attn_norm 0 = sigmoid / 1 = softmax, postnet_output_dim = rows of
                       last_linear.
   tts_tacotron1_infer <- Tacotron.inference, batched: output i equals the reference B = 1 call on
                       utterance i. Arguments as tts_taco_infer except: no stop threshold (the
                       reference's literals: after step t, stop if t > T/4 and (sigmoid(stop) > 0.6 or
                       alignment[T-1] > 0.6); else stop with status 2 if t > max_decoder_steps, so a
                       row that never stops takes h_max_steps[b] + 1 steps and S_cap must be at least
                       max(h_max_steps) + 1); d_post is (B, S_cap*r, postnet_output_dim). At most 64
                       rows and 1024 input positions per call. h_status: 1 stop rule, 2 max steps.
   tts_tacotron1_encoder <- Encoder(embedding(ids)): d_out (B, T_max, 256), zero for t >= h_lens[b]
   tts_tacotron1_postnet <- last_linear(PostCBHG(dec)) on d_dec (B, M_max, 80), rows valid for
                       m < h_lens[b]: d_out (B, M_max, postnet_output_dim), zero past the rows */
int tts_tacotron1_set_tensor(tts_ctx* ctx, const char* name, const float* h_data, const int64_t* shape, int ndim);
int tts_tacotron1_finalize(tts_ctx* ctx, int num_chars, int r_init, int memory_size, int attn_norm,
                           int postnet_output_dim);
int tts_tacotron1_infer(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                        const int32_t* h_max_steps, int S_cap, float* d_dec, float* d_post, float* d_align,
                        float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream);
int tts_tacotron1_encoder(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max,
                          float* d_out, void* stream);
int tts_tacotron1_postnet(tts_ctx* ctx, const float* d_dec, const int32_t* h_lens, int B, int M_max, float* d_out,
                          void* stream);

/* ---- MultiBand-MelGAN generator ---- */
int tts_melgan_set_tensor(tts_ctx* ctx, const char* name, const float* h_data, const int64_t* shape, int ndim);
/* upsample_factors: n_up entries (even), base_channels, num_res_blocks, out_channels (4 with PQMF) */
int tts_melgan_finalize(tts_ctx* ctx, int in_channels, int out_channels, int base_channels,
                        const int32_t* upsample_factors, int n_up, int num_res_blocks, int use_pqmf);

/* d_mel (B, in_channels, M_max) channel-major, utterance b valid for m < h_lens[b];
   pad = inference_padding (replicate). Requires h_lens[b] + 2*pad >= 4 (ReflectionPad1d(3)).
   d_wav (B, 1, hop*(M_max + 2*pad)), hop = prod(upsample_factors) * (out_channels if PQMF else 1);
   samples past hop*(h_lens[b] + 2*pad) are zero. */
int tts_melgan_infer(tts_ctx* ctx, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                     float* d_wav, void* stream);
/* the same with d_mel given by element strides (batch, channel, frame), e.g. a Tacotron2 postnet
   output (B, M, in_channels) read in place as (B, in_channels, M): strides (M*in_channels, 1,
   in_channels), no transposed copy. Channel stride 1 needs a frame stride divisible by 4 and a
   16-byte aligned d_mel. */
int tts_melgan_infer_strided(tts_ctx* ctx, const float* d_mel, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                             const int32_t* h_lens, int B, int M_max, int pad, float* d_wav, void* stream);

/* generator layers only: d_out (B, out_channels, up*(M_max + 2*pad)), up = prod(upsample_factors) */
int tts_melgan_generator(tts_ctx* ctx, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                         float* d_out, void* stream);

/* PQMF synthesis on (B, N, L) subbands with filter d_G (N, taps+1) -> d_y (B, 1, N*L) */
int tts_pqmf_synthesis(tts_ctx* ctx, const float* d_x, int B, int N, int L, const float* d_G, int taps,
                       float* d_y, void* stream);

/* ---- ParallelWaveGAN generator (TTS/vocoder/models/parallel_wavegan_generator.py) ----
   tts_pwgan_set_tensor/finalize <- ParallelWaveganGenerator(...) as setup_generator builds it
                       (vocoder/utils/generic_utils.py:79-92: 64 res / 128 gate / 64 skip / 80 aux
                       channels, kernel 3) + load_state_dict (weight_g / weight_v or folded weight)
   tts_pwgan_infer  <- ParallelWaveganGenerator.inference (:120-125): replicate pad `pad`, ConvUpsample,
                       first_conv on d_noise (B, 1, hop*(M_max + 2*pad)) standard normal, residual
                       blocks, output convs -> d_out (B, 1, hop*(M_max + 2*pad)); row b is zero past
                       hop*(h_lens[b] + 2*pad) */
int tts_pwgan_set_tensor(tts_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int tts_pwgan_finalize(tts_ctx* ctx, int num_res_blocks, int stacks, const int32_t* upsample_factors, int n_up);
int tts_pwgan_infer(tts_ctx* ctx, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                    const float* d_noise, float* d_out, void* stream);

/* ---- Glow-TTS (TTS/tts/models/glow_tts.py, reference configs: gated-conv encoder) ----
   tts_glow_set_tensor/finalize <- GlowTts(...).load_state_dict (enc_layers = 3 + num_layers_enc)
   tts_glow_encode  <- GlowTts.inference up to the durations (glow_tts.py:166-176): encoder,
                       duration predictor, w_ceil; h_ylens out: y_lengths per utterance
   tts_glow_decode  <- the rest (:177-193) for Ty = max(h_ylens): generate_path, expanded means,
                       z = y_mean + d_noise * noise_scale (d_noise (B, 80, Ty) standard normal),
                       reverse flows; d_y (B, 80, 2*floor(Ty/2)), d_ymean (B, 80, Ty),
                       d_attn (B, Ty, T_max), d_logw (B, T_max) = o_dur_log */
int tts_glow_set_tensor(tts_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int tts_glow_finalize(tts_ctx* ctx, int num_chars, int enc_layers, int num_flow_blocks, int num_block_layers);
int tts_glow_encode(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max,
                    float length_scale, int32_t* h_ylens, void* stream);
/* tts_glow_encode_spk <- GlowTts.inference(x, x_lengths, g) (glow_tts.py:159-176) for a
   multi-speaker model (num_speakers > 1, c_in_channels > 0): h_speaker_ids (B) index emb_g;
   g = F.normalize(emb_g(ids)) joins the duration predictor input (encoder.py:131-135) and, through
   each coupling block's cond_layer, the WN gates of the following tts_glow_decode (glow.py:119-130).
   h_speaker_ids = NULL is tts_glow_encode. Errors as the reference fails: ids given to a model
   without emb_g or cond_layer, no ids for a model with c_in_channels > 0, an id out of range. */
int tts_glow_encode_spk(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, const int32_t* h_speaker_ids,
                        int B, int T_max, float length_scale, int32_t* h_ylens, void* stream);
int tts_glow_decode(tts_ctx* ctx, const float* d_noise, float noise_scale, int Ty, float* d_y, float* d_ymean,
                    float* d_attn, float* d_logw, void* stream);
/* tts_glow_align <- GlowTts.forward in eval (glow_tts.py:114-156), the analysis direction, for the
   batch of the preceding tts_glow_encode / _encode_spk (it reuses that call's o_mean, o_dur_log,
   lengths and speaker conditioning). d_y (B, 80, Ty) is the mel, h_ylens its frames per row; each is
   rounded down to even and Te = 2 * floor(Ty / 2) (preprocess, :187-194). Out: d_z (B, 80, Te) the
   latent of the forward flows, d_logdet (B) their log-determinant, d_logp (B, T_max, Te) the
   likelihood matrix (:141-150; zero outside a row's lengths; NULL: kept internal), d_attn
   (B, Te, T_max) the monotonic alignment, d_ymean (B, 80, Te) the encoder means along it,
   d_oattn_dur (B, T_max) = log(1 + frames per token), d_logw (B, T_max) = o_dur_log. The alignment
   search runs on the device (no host round trip) and repeats maximum_path_c's arithmetic, so the
   path is a function of logp's bits. Fails if a row has fewer even-rounded frames than tokens, or
   fewer than 2: the reference's search reads outside its band there. */
int tts_glow_align(tts_ctx* ctx, const float* d_y, const int32_t* h_ylens, int Ty, float* d_z, float* d_logdet,
                   float* d_logp, float* d_attn, float* d_ymean, float* d_oattn_dur, float* d_logw, void* stream);
/* tts_glow_mas <- maximum_path (layers/glow_tts/monotonic_align) alone: d_logp (B, Tx, Ty), per-row
   h_xlens <= h_ylens; d_path (B, Tx, Ty) holds 1 on the path and 0 elsewhere. B <= 64, Tx <= 4096. */
int tts_glow_mas(tts_ctx* ctx, const float* d_logp, const int32_t* h_xlens, const int32_t* h_ylens, int B, int Tx,
                 int Ty, float* d_path, void* stream);

/* ---- GE2E speaker encoder (TTS/speaker_encoder/model.py) ----
   tts_ge2e_set_tensor/finalize <- SpeakerEncoder(input_dim, proj_dim, lstm_dim, num_lstm_layers,
                                   use_lstm_with_projection).load_state_dict  (model.py:31-47)
   tts_ge2e_infer               <- SpeakerEncoder.inference(x) (model.py:62-68) on B sequences of
                                   per-sequence length h_lens[b]: d_x (B, T_max, input_dim) fp32,
                                   d_out (B, proj_dim) L2-normalised embeddings. lstm_dim must be 768. */
int tts_ge2e_set_tensor(tts_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int tts_ge2e_finalize(tts_ctx* ctx, int input_dim, int proj_dim, int lstm_dim, int num_lstm_layers,
                      int use_lstm_with_projection);
int tts_ge2e_infer(tts_ctx* ctx, const float* d_x, const int32_t* h_lens, int B, int T_max, float* d_out,
                   void* stream);

/* ---- Griffin-Lim waveform stage (TTS/utils/audio.py, the path of a Synthesizer without a vocoder) ----
   Both entries only enqueue kernels: no host synchronisation in either GEMM mode, no graph capture.

   tts_mel_to_linear <- AudioProcessor._denormalize + _db_to_amp + _mel_to_linear and the power of
                       inv_melspectrogram (audio.py:213-214, 241-248, 126-163):
                       S = max(1e-10, inv_basis @ 10^((clip(mel) * scale + offset) / spec_gain)) ^ power
   d_mel       (B, M_max, n_mels) normalised mel, frame-major (a Tacotron2 postnet output); row b is
               read for t < h_lens[b] only (0 <= h_lens[b] <= M_max)
   d_inv_basis (n_freq, n_mels) pseudo-inverse of the mel filterbank
   d_scale, d_offset (n_mels) the denormalisation as dB = x * scale + offset per channel: covers the
               mean-var scaler (std, mean) and the range normalisations (one value repeated);
               use_clip != 0 clips x to [clip_lo, clip_hi] first (clip_norm)
   d_S         (B, M_max, n_freq); frames t >= h_lens[b] are written as zero
   1 <= B <= 64, 1 <= n_mels <= 512. */
int tts_mel_to_linear(tts_ctx* ctx, const float* d_mel, const int32_t* h_lens, int B, int M_max, int n_mels,
                      int n_freq, const float* d_inv_basis, const float* d_scale, const float* d_offset,
                      float clip_lo, float clip_hi, int use_clip, float spec_gain, float power, float* d_S,
                      void* stream);

/* tts_griffin_lim <- AudioProcessor._griffin_lim (audio.py:259-279) on a batch: librosa.istft of
                       S e^{2 pi i u}, then `iters` rounds of librosa.stft -> unit phase (a bin that is
                       exactly 0 counts as phase 0) -> librosa.istft. Periodic Hann window of win_length
                       points centred in n_fft, centred frames with reflect padding, window-square
                       envelope division where the envelope exceeds 1e-11; fp32.
   d_S         (B, M_max, n_fft / 2 + 1) target magnitudes, frame-major (tts_mel_to_linear's output)
   d_phase0    (B, M_max, n_fft / 2 + 1) uniform [0, 1) numbers u, the initial phase / (2 pi)
   d_wav       (B, hop_length * (M_max - 1)); row b holds hop_length * (h_lens[b] - 1) samples, the rest
               of the row is written as zero. Frames t >= h_lens[b] of d_S / d_phase0 are never read.
   Supported: n_fft == 1024, 1 <= win_length <= 1024, 64 <= hop_length <= 512, iters >= 0, 1 <= B <= 64,
   and every row hop_length * (h_lens[b] - 1) > n_fft / 2 (the reflect padding's own requirement,
   as torch.stft). Anything else is an error and launches nothing. Row b equals its own B = 1
   call bit for bit. The frame buffers live in the context's workspace; the window and twiddle
   tables are computed in double on the host once per win_length (a change of win_length waits for
   the context's queued work before the upload). */
int tts_griffin_lim(tts_ctx* ctx, const float* d_S, const int32_t* h_lens, int B, int M_max, int n_fft,
                    int win_length, int hop_length, int iters, const float* d_phase0, float* d_wav, void* stream);

/* ---- Audio analysis (TTS/utils/audio.py: waveform -> spectrogram / melspectrogram) ----
   Both entries only enqueue kernels, as the Griffin-Lim entries above.

   tts_stft_mag <- abs(AudioProcessor._stft(apply_preemphasis(y))) (audio.py:198-202, 259-267) on a
                       batch: librosa.stft conventions (periodic Hann window of win_length points
                       centred in n_fft, centred frames, reflect padding), pre-emphasis
                       y[q] - preemphasis * y[q-1] (y[-1] = 0) applied before the padding; fp32.
   d_wav       (B, L_max) waveform rows; row b is read for q < h_nsamples[b] only
   d_mag       (B, M_max, n_fft / 2 + 1) magnitudes, frame-major; row b holds
               1 + h_nsamples[b] / hop_length frames, the rest of the row is written as zero
   algo        0: the 1024-point FFT kernel when n_fft == 1024, else a direct DFT over an n_fft-entry
               twiddle table; 1: the FFT kernel (n_fft == 1024 only); 2: the direct DFT
   Supported: n_fft even in [64, 2048], 1 <= win_length <= n_fft, 16 <= hop_length <= n_fft,
   1 <= B <= 64, and every row n_fft / 2 < h_nsamples[b] <= L_max (the reflect padding's own
   requirement, as torch.stft) with 1 + h_nsamples[b] / hop_length <= M_max. Anything else is an
   error and launches nothing. Row b equals its own B = 1 call bit for bit. The twiddle and window
   tables are computed in double on the host, the twiddles once per n_fft (a change of n_fft or
   win_length waits for the context's queued work before the upload). */
int tts_stft_mag(tts_ctx* ctx, const float* d_wav, const int32_t* h_nsamples, int B, int L_max, int n_fft,
                 int win_length, int hop_length, float preemphasis, int algo, float* d_mag, int M_max,
                 void* stream);

/* tts_mag_to_feature <- AudioProcessor._normalize(_amp_to_db(basis @ mag)) (audio.py:108-124, 205-207):
                       out = clip(spec_gain * log10(max(1e-5, X)) * scale + offset), X = basis @ mag,
                       or X = mag when d_basis is NULL (the linear spectrogram; n_out == n_freq)
   d_mag       (B, M_max, n_freq) magnitudes, frame-major (tts_stft_mag's output); row b is read for
               t < h_lens[b] only (0 <= h_lens[b] <= M_max)
   d_basis     (n_out, n_freq) mel filterbank, or NULL
   d_scale, d_offset (n_out) the normalisation per channel: covers both range normalisations (one
               value repeated), the mean-var scaler (1 / std, -mean / std) and none (1, 0);
               use_clip != 0 clips the result to [clip_lo, clip_hi] (clip_norm)
   d_out       (B, M_max, n_out); frames t >= h_lens[b] are written as zero
   1 <= B <= 64, 1 <= n_freq, n_out <= 1025. */
int tts_mag_to_feature(tts_ctx* ctx, const float* d_mag, const int32_t* h_lens, int B, int M_max, int n_freq,
                       int n_out, const float* d_basis, float spec_gain, const float* d_scale,
                       const float* d_offset, float clip_lo, float clip_hi, int use_clip, float* d_out,
                       void* stream);

/* The waveform tail (wav_tail.hip): what lies between a model's output tensor and the bytes
   Synthesizer.tts returns. The three entries only enqueue kernels on `stream`: ordinary launches,
   every loop bounded by a length checked here on the host, plain vector stores, one fixed order of
   operations per output, so row b of a batched call equals its own B = 1 call bit for bit.
   1 <= B <= 64. An unsupported argument is an error that launches nothing.

   tts_spec_to_mag <- AudioProcessor.inv_spectrogram's magnitudes (audio.py:232-236), the linear
                      counterpart of tts_mel_to_linear without the basis:
                      S = (10 ^ ((clip(x) * scale + offset) / spec_gain)) ^ power
   d_spec      (B, M_max, n_freq) normalised linear spectrograms, frame-major (a Tacotron (v1)
               postnet output); row b is read for t < h_lens[b] only (0 <= h_lens[b] <= M_max)
   d_scale, d_offset (n_freq), clip_lo / clip_hi / use_clip: as tts_mel_to_linear
   d_S         (B, M_max, n_freq); frames t >= h_lens[b] are written as zero
   1 <= n_freq <= 1025. */
int tts_spec_to_mag(tts_ctx* ctx, const float* d_spec, const int32_t* h_lens, int B, int M_max, int n_freq,
                    const float* d_scale, const float* d_offset, float clip_lo, float clip_hi, int use_clip,
                    float spec_gain, float power, float* d_S, void* stream);

/* tts_deemphasis <- scipy.signal.lfilter([1], [1, -a], x) per row (audio.py:204-207):
                     y[n] = x[n] + a * y[n-1], y[-1] = 0, for n < h_nsamples[b]
   d_in, d_out (B, L_max); the rest of every output row is written as zero (0 <= h_nsamples[b] <=
               L_max); d_out may be d_in
   a           0 < a < 1
   One workgroup per row scans the affine maps of 16-sample chunks, 512 chunks to a tile, the tiles
   in sequence: the partition depends on the row's own length only. The powers of a that the scan
   multiplies by are computed in double here and rounded once. */
int tts_deemphasis(tts_ctx* ctx, const float* d_in, const int32_t* h_nsamples, int B, int L_max, double a,
                   float* d_out, void* stream);

/* tts_wav_finish <- the tail of Synthesizer.tts (server/synthesizer.py:179-193): per row
                     AudioProcessor.find_endpoint (audio.py:302-309), the rows cut there and joined in
                     order, `gap` zeros after each (the last included), then save_wav (audio.py:335-337)
   d_wav       (B, L_max) waveforms, row b valid for h_nsamples[b] samples (0 <= h_nsamples[b] <= L_max)
   window_length, hop_length, threshold: the endpoint of row b is x + hop_length for the first x in
               range(hop_length, n - window_length, hop_length) whose window [x, x + window_length)
               has a maximum of the signed samples m with (double) m < threshold, else n. Needs
               1 <= hop_length <= window_length, window_length / hop_length <= 64.
   d_pcm       int16, capacity sum(h_nsamples) + B * gap; the first *d_total entries are written:
               trunc(x * f) in float32, f = (float) (32767 / (double) peak) when the float32 peak
               of |x| over the joined signal is above 0.01, else 3276700: numpy 2's arithmetic in
               save_wav on a float32 array, bit for bit
   d_ends      (B) the endpoints; d_total: the joined length, sum(d_ends) + B * gap
   0 <= gap < 2^24; the capacity must stay below 2^31. */
int tts_wav_finish(tts_ctx* ctx, const float* d_wav, const int32_t* h_nsamples, int B, int L_max,
                   int window_length, int hop_length, double threshold, int gap, int16_t* d_pcm, int32_t* d_ends,
                   int32_t* d_total, void* stream);

/* Vocoder scoring (TTS/vocoder/layers/pqmf.py:48-49, TTS/vocoder/layers/losses.py:7-52). All three
   only enqueue work on `stream`; rows are read for their own lengths only.

   tts_pqmf_analysis <- PQMF.analysis: F.conv1d(x, H, padding = taps / 2, stride = N)
   d_x         (B, L_max) waveforms, row b valid for h_lens[b] samples (0 <= h_lens[b] <= L_max); the
               zero padding sits at the row's own ends
   d_H         (N, taps + 1) analysis filters, N <= 8, taps even and <= 254
   d_y         (B, N, Lout_max) bands; row b holds (h_lens[b] - 1) / N + 1 positions and zeros after
               them. Plain fp32 FMA over the taps in ascending order. */
int tts_pqmf_analysis(tts_ctx* ctx, const float* d_x, const int32_t* h_lens, int B, int L_max, int N,
                      const float* d_H, int taps, float* d_y, int Lout_max, void* stream);

/* tts_stft_pair_sums <- the sums behind STFTLoss.forward(y_hat, y) for one resolution, per row:
     d_sums[b] = { sum |log y_M - log y_hat_M|, sum (y_M - y_hat_M)^2, sum y_M^2 }   (B, 3) float64
   over the row's n_fft / 2 + 1 bins and 1 + (h_nsamples[b] + 2 (n_fft / 2) - n_fft) / hop_length frames,
   M = sqrt(max(re^2 + im^2, 1e-8)) of torch.stft(x, n_fft, hop_length, win_length,
   hann_window(win_length), center = True, pad_mode = "reflect", onesided = True).
   d_yhat, d_y (B, L_max), row b valid for h_nsamples[b] samples, n_fft / 2 < h_nsamples[b] <= L_max
               (a shorter row fails as in torch: "Padding size should be less than ...")
   16 <= win_length <= n_fft <= 2048 (either parity), hop_length >= 1, B <= 64.
   A windowed DFT as a GEMM on the fp32 MFMA, the spectra stay on chip; per-tile fp32 partial sums
   are added per row in tile order in float64. A row's tiles depend on its own length only: its
   sums are the same bits alone and in any batch. The first call with a new (n_fft, win_length)
   builds and uploads its DFT basis (a blocking copy); the context keeps it. */
int tts_stft_pair_sums(tts_ctx* ctx, const float* d_yhat, const float* d_y, const int32_t* h_nsamples, int B,
                       int L_max, int n_fft, int win_length, int hop_length, double* d_sums, void* stream);

/* tts_torch_stft_mag <- TorchSTFT.__call__: the magnitudes M above of one signal
   d_mag       (B, n_fft / 2 + 1, frames_max), row b zero past its own frames; frames_max >= every
               row's frame count. Other arguments and limits as tts_stft_pair_sums. */
int tts_torch_stft_mag(tts_ctx* ctx, const float* d_wav, const int32_t* h_nsamples, int B, int L_max, int n_fft,
                       int win_length, int hop_length, float* d_mag, int frames_max, void* stream);

/* Measurement hook for bench.py: average device time (ms) of `iters` launches of one kernel of the
   last tts_taco_infer configuration, timed with hipEvents on the context's stream.
   which: 0 = decoder LSTM GEMM step kernel (K4), 1 = full decoder step (all 7 kernels). */
int tts_time_decoder_kernel(tts_ctx* ctx, int which, int iters, float* ms_out);

/* Decoder launches of the last tts_taco_infer: path 1 = persistent kernel (one launch per
   batch-tile count, 64 / 48 / 32 / 16 rows, nlaunch <= 4: ms and steps must hold 4 entries;
   ms[i] = hipEvent time of launch i, steps[i] = decoder steps it completed), path 0 = step
   graphs (nlaunch = 0). */
int tts_decoder_stats(tts_ctx* ctx, int* path, int* nlaunch, float* ms, int* steps);

/* GEMM arithmetic of the context's kernels. mode 1 (default) = split-f16 MFMA where a kernel has
   it: every fp32 operand as hi + 2^-11 lo f16 halves, three f16 MFMAs per product accumulated in
   fp32, error equal to the fp32 MFMA GEMM's; a call whose operands leave the f16
   range (|v| >= 65504) is re-run on the fp32 kernels. mode 0 = fp32 MFMA everywhere. The
   environment variable TTS_GEMM=f32 starts contexts in mode 0. tts_gemm_mode reports the mode and
   how many calls fell back to fp32. */
int tts_set_gemm_mode(tts_ctx* ctx, int mode);
int tts_gemm_mode(tts_ctx* ctx, int* mode, int64_t* fallbacks);

/* Tacotron2.inference then MultibandMelganGenerator.inference on its postnet output in ONE call
   (TTS/server/synthesizer.py:150-159 runs the two back to back, the mel lengths passing through
   Python): the decoded lengths h_steps[b] * r go from the decode's status words straight to the
   vocoder launches, which read d_post in place (frame-major). Arguments as tts_taco_infer_spk
   (d_spk_ids / d_spk_emb may both be NULL: single-speaker model) plus the vocoder's inference
   padding `pad` and d_wav, which must hold B * hop * (S_cap * r + 2 pad) floats (hop = 4 x the
   product of the upsample factors). On return its first B * hop * (M + 2 pad) floats, M = r *
   max(h_steps), are the (B, 1, hop * (M + 2 pad)) waveform batch: bit-identical to
   tts_melgan_infer_strided on d_post viewed as (B, 80, M) with strides (S_cap r 80, 1, 80) and
   lengths h_steps * r. The vocoder is launched on the decoded lengths as the decode leaves them on
   the device (rows shorter than the vocoder's reflection pads fail the call), before the host
   reads the decode's status words. Split-f16 range scopes as the two calls: a decode overflow
   re-runs decode and vocoder in fp32, a vocoder overflow the vocoder alone. Returns with the
   call's work done. */
int tts_taco_mbmelgan_infer(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                            const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                            const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                            int pad, float* d_wav, int32_t* h_steps, int32_t* h_status, void* stream);

/* tts_taco_mbmelgan_infer in two halves, so that a caller can queue the next batch while this
   one's vocoder runs. submit returns when h_steps / h_status are filled and hands out *h_ticket:
   the decode's outputs are done and later work on `stream` is ordered after them, while the
   vocoder may still be running on the library's stream. finish(ticket, stream) waits for that
   vocoder and, if its split-f16 operands left the f16 range, runs it again on the fp32 kernels;
   then d_wav is final and later work on `stream` is ordered after it. Until finish, the caller
   must leave d_post and d_wav untouched and must not read d_wav. At most 4 submissions are outstanding per context: a fifth submit finishes the oldest
   first. finish on a ticket that is already complete returns 0. */
int tts_taco_mbmelgan_submit(tts_ctx* ctx, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                             const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                             const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                             int pad, float* d_wav, int32_t* h_steps, int32_t* h_status, int64_t* h_ticket,
                             void* stream);
int tts_taco_mbmelgan_finish(tts_ctx* ctx, int64_t ticket, void* stream);

/* Test hook (process-wide, off by default): recurrence >= 0 makes one workgroup of that persistent
   BiLSTM recurrence leave before its second grid barrier, so the others time out and the next
   Tacotron2 call reports the encoder barrier error; -1 turns it off. Only tests call it. */
int tts_test_stall_lstm(int recurrence);

/* Test hook: one launch of the generic conv (conv.hip / conv_x3.hip) through the production path.
   The layer is packed from the host weight and bias with the loaders' own functions (pack_conv,
   or pack_convT for a ConvTranspose1d), one run_conv is issued on the context's stream, the stream
   is synchronised and the layer is freed. The context's GEMM mode (tts_set_gemm_mode) decides
   whether the split-f16 kernel is offered; the range flag is reported, no fp32 re-run is made.
   Strides are {batch, channel, time} in elements. Only tests and tools call it.
     transposed = 0: Conv1d, h_weight (Cout, Cin, K), `nphase` phase blocks of it when nphase > 1
                     (each with its pad_left[phase]; output position q * out_mul + phase);
     transposed = 1: ConvTranspose1d(k = 2u, stride u, padding u / 2), u = nphase, h_weight
                     (Cin, Cout, 2u); K, dil and pad_left are ignored. merged_u = 0 runs the u
                     polyphase convs (set out_mul = u), merged_u = u the phase-merged split-f16 form
                     (set out_mul = 1 and max_q = the longest row + 1).
   Every other field has the meaning of the same-named ConvCall / ConvArgs field (csrc/common.h).
   Out: ran_x3 (1 split-f16 kernel, 0 fp32 kernel), tq (tile width in output positions of the kernel
   launched), range_flag (the split-f16 range flag after the call; 0 on the fp32 kernel). */
typedef struct tts_conv_test {
  const float* h_weight;
  const float* h_bias; /* [Cout] */
  int32_t transposed, Cin, Cout, K, dil, nphase;
  int32_t pad_left[8];
  int32_t merged_u;
  int32_t nsrc; /* 1 or 2 */
  const float* d_src[2];
  int64_t src_strides[2][3];
  int32_t src_C[2];   /* channels of each source (nsrc = 2; one source has Cin) */
  int32_t src_act[2]; /* 1: leaky-relu(0.2) on load */
  float* d_out;
  int64_t out_strides[3];
  const float* d_resid; /* or NULL */
  int64_t resid_strides[3];
  int32_t resid_rows;
  const float* d_aux; /* or NULL */
  int64_t auxb;
  const int32_t* h_lens; /* [B], host */
  int32_t B, max_q, len_add, in_mul, q_mul, out_mul, rep_pad, pad_mode, epi;
  int32_t ran_x3, tq; /* out */
  uint32_t range_flag; /* out */
} tts_conv_test;
int tts_test_conv(tts_ctx* ctx, tts_conv_test* d, void* stream);

/* Test hook: one launch of one vocoder kernel (resblock.hip, resblock_x3.hip, resstack_x3.hip,
   melgan_out.hip) through the production packing. The weights are packed from the host arrays with
   the functions tts_melgan_finalize uses ([W_1x1 | W_sc] and b_1x1 + b_sc through pack_conv,
   pack_resblock_x3 / pack_resblock_x3p, pack_convT, the output conv's transposition), the launcher
   `kind` names is called once on the context's stream, without the switches that choose between the
   kernels in a generator run, the stream is synchronised and what was packed is freed. A shape the
   launcher does not cover is the library's normal error with the launcher's message; no fp32 re-run
   is made. Only tests and tools call it.
     kind 0: launch_resblock (fp32)            1: launch_resblock_x3 (split-f16)
          2: launch_resstack_x3, blocks 0-2    3: the same with the fused LeakyReLU + ConvTranspose1d(u = 2)
          4: launch_out_pqmf                   5: launch_out_conv1
   Weights, all host: per block k (one block for kinds 0-1, three for kinds 2-3) wd (C, C, 3), bd,
   w1 (C, C, 1), b1, ws (C, C, 1), bs and dil[k]; kind 3 ct_w (2C, C, 4), ct_b; kinds 4-5 wo (N, C, 7),
   bo (N), N = 1 for kind 5; kind 4 G (N, taps + 1).
   d_x / d_y: device tensors, x_strides / y_strides = {batch, channel} in elements (kinds 0-2: equal for
   both; kind 3: d_x is the ConvTranspose's input, 2C channels at half the length; kinds 4-5: y has N rows
   resp. one row per utterance and only its batch stride is read). Row b has (h_lens[b] + len_add) * mul
   positions; h_lens is uploaded as the device lengths, h_bounds (or NULL: h_lens) is what the launcher
   gets as its host lengths: per-row upper bounds, as a fused Tacotron2 -> vocoder call passes them.
   max_q: the launcher's max_q / maxL.
   Out: tq (output positions per tile of the kernel launched), range_flag (the split-f16 range flag
   after the call, zeroed before it; 0 for kinds 0, 4, 5). */
typedef struct tts_voc_test {
  int32_t kind, C, N, taps;
  const float* wd[3];
  const float* bd[3];
  const float* w1[3];
  const float* b1[3];
  const float* ws[3];
  const float* bs[3];
  int32_t dil[3];
  const float* ct_w;
  const float* ct_b;
  const float* wo;
  const float* bo;
  const float* G;
  const float* d_x;
  float* d_y;
  int64_t x_strides[2], y_strides[2];
  const int32_t* h_lens;   /* [B], host */
  const int32_t* h_bounds; /* [B], host, or NULL */
  int32_t B, len_add, mul, max_q;
  int32_t tq;          /* out */
  uint32_t range_flag; /* out */
} tts_voc_test;
int tts_test_voc(tts_ctx* ctx, tts_voc_test* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
