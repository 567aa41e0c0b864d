// Launchers and host packers of the kernel files that have no header of their own (encoder.hip,
// glow.hip, glow_forward.hip, pwgan.hip). Each is declared here only; the file that defines it includes this header,
// so the compiler checks the signature against the definition.
#pragma once
#include "common.h"  // RowInts
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

// encoder.hip
void launch_embed_gather(const int64_t* ids, int T_max, const float* table, int num_rows, int D,
                         const int* lens, int B, float* out, hipStream_t s, const int* rowmap = nullptr);
int launch_bilstm_persist(const float* Gin, const float* Whh, const uint16_t* Whh16, const int* lens, int T_max,
                          int B, float* hbuf, unsigned* bar, float* out, hipStream_t s);
bool launch_ge2e_pipe(const uint16_t* const* w16, const float* const* bias, int nl, const float* gin0, const int* lens,
                      int T_max, int B, float* hbuf, unsigned* bar, float* out, hipStream_t s);
bool launch_lstm768_persist(const float* Gin, const float* Whh, const uint16_t* Whh16, const int* lens, int T_max,
                            int B, float* hbuf, unsigned* bar, float* out, hipStream_t s);
void launch_bilstm(const float* Gin, const float* Whh, const int* lens, int T_max, int B, float* hbuf, float* cbuf,
                   float* out, hipStream_t s);

// glow.hip
void launch_glu_ln_res(const float* x, long xb, int C2, const float* gamma, const float* beta, const float* res,
                       long rb, float* out, long ob, const int* lens, int B, int T, hipStream_t s);
void launch_ln(float* x, long xb, int C, const float* gamma, const float* beta, const int* lens, int B, int T,
               hipStream_t s, bool relu = false);
void launch_glow_mha(const float* qkv, int H, int heads, int T, const int* lens, float* out, int B, hipStream_t s);
void launch_tds_depthwise(const float* x, int C, int T, const float* w, const float* bias, const int* lens, float* y,
                          int B, hipStream_t s);
void launch_glow_durations(const float* logw, int T, const int* lens, float length_scale, float* cum, int* ylen,
                           float* wceil, int B, hipStream_t s);
void launch_glow_expand(const float* o_mean, int C, int Tx, const int* xlens, const float* cum, const int* ylens,
                        int Ty, const float* noise, float noise_scale, float* y_mean, float* z, float* attn, int B,
                        hipStream_t s);
void launch_glow_squeeze(const float* x, int C, int T, const int* ylens, float* y, int K, int B, hipStream_t s);
void launch_glow_unsqueeze(const float* x, int C2, int K, const int* ylens, float* y, int T, int B, hipStream_t s);
void launch_glow_speaker(const int* spk, const float* table, int c_in, int c_pad, float* g, int B, hipStream_t s);
void launch_glow_embed(const int64_t* ids, int T, const float* table, int rows, int D, const int* lens, float* out,
                       int B, hipStream_t s);

// glow_forward.hip (GlowTts.forward: forward flows, likelihood matrix, monotonic alignment search)
void launch_glow_fwd_glue(const float* x, const float* eo, const float* tab, float* out, int C, int K,
                          const int* klens, double* part, int B, hipStream_t s);
void launch_glow_logdet(const double* part, int nblk, int tiles, int B, const int* klens, double wconst, float* logdet,
                        hipStream_t s);
void launch_glow_logp(const float* om, int C, int Tx, const int* xlens, const float* z, int Ty, const int* ylens,
                      float* logp, int B, hipStream_t s);
long glow_mas_bits_words(int Tx, int Ty);  // 64-bit decision words per utterance
void launch_glow_mas(const float* logp, int Tx, int Ty, const int* xlens, const int* ylens, int max_xlen,
                     unsigned long long* bits, int* xof, int B, hipStream_t s);
void launch_glow_path(const int* xof, int Tx, int Ty, float* path, int B, hipStream_t s);
void launch_glow_align_out(const float* om, int C, int Tx, const int* xlens, const int* xof, int Ty, const int* ylens,
                           float* y_mean, float* attn, float* dur, int B, hipStream_t s);

// pwgan.hip
void launch_pw_upsample(const float* in, long ib, int Lin_max, const int* lens, int len_add, int in_mul, int s,
                        const float* h, float* out, long ob, int Lout_max, int C, int B, hipStream_t st);
void launch_pw_first(const float* noise, long nb, const float* w, const float* bias, const int* lens, int len_add,
                     int hop, float* x, int Tmax, int B, hipStream_t st);
void launch_pw_layer(const float* x, const float* c, float* xn, float* skip, const float* W1, const float* b1,
                     const float* W2, const float* b2, const int* lens, const float* zeros, int len_add, int hop,
                     int Tmax, int dil, int first, int B, int variant, hipStream_t st);
void launch_pw_layer_x3(const float* x, const float* c, float* xn, float* skip, const void* W1x, const float* b1,
                        const void* W2x, const float* b2, const int* lens, const int* h_lens, int len_add, int hop,
                        int Tmax, int dil, int first, int B, unsigned* oflow, hipStream_t st);
void pack_pw_layer_x3(const std::vector<float>& m1, const std::vector<float>& m2, std::vector<uint16_t>& w1x,
                      std::vector<uint16_t>& w2x);
void launch_pw_out(const float* skip, float scale, const float* W3, const float* b3, const float* w4,
                   const float* b4, const int* lens, int len_add, int hop, int Tmax, float* out, int B,
                   hipStream_t st);

// tacotron1.hip. Activations are channel-last (B, T, C) fp32; every kernel masks by the rows' own
// lengths (device ints) and writes zeros past them inside [0, T_max).
constexpr int T1_MEM_MAX = 32;   // memory_size (frames of the decoder's memory queue)
constexpr int T1_R_MAX = 10;     // r_init
constexpr int T1_T_MAX = 1024;   // encoder positions the decoder's attention state holds
// out[b][t][oc0 + co] = act(bias[co] + sum_{k, ci} W[k][ci][co] x[b][t + k - padl][ci]) (+ resid);
// W is [K][Cin][Cout], act 1 = ReLU, bias / resid may be null; K <= 16
struct T1Conv {
  const float* x;
  long xb;  // batch stride (elements)
  int ldx, Cin;
  const float* W;
  const float* bias;
  int K, padl, Cout, act;
  const float* resid;
  long rb;
  int ldr;
  float* out;
  long ob;
  int ldo, oc0;
};
void launch_t1_conv(const T1Conv& c, const int* lens, int B, int T_max, hipStream_t s);
// 4 highway layers in place on (B, T_max, 128); Wt [layer][H | T][in][out], bias [layer][H | T][128]
void launch_t1_highway(float* x, long xb, const float* Wt, const float* bias, const int* lens, int B, int T_max,
                       hipStream_t s);
// gin (B, T_max, 768) = [dir][r | z | n] input projections with b_ih; Whh [dir][384][128]; out (B, T_max, 256)
void launch_t1_bigru(const float* gin, long gb, const float* Whh, const float* bhh, const int* lens, int B, int T_max,
                     float* out, long ob, hipStream_t s);
// the whole decode, one workgroup per row. Matrices are transposed ([in][out]); wcomb = location_dense
// . location_conv folded, [2 channels][31 taps][128]. mem_frames = memory_size (<= 0: last frame only).
struct T1DecArgs {
  const float *enc, *pin;  // (B, T_max, 256) encoder outputs, (B, T_max, 128) inputs_layer(enc)
  const int *lens, *max_steps;
  int T_max, S_cap, r, r_init, mem_frames, softmax;
  const float *pre1, *pre1_b, *pre2, *pre2_b, *att_ih, *att_hh, *att_bih, *att_bhh, *wq, *wcomb, *v;
  float bv;
  const float *pdi, *pdi_b, *rnn_ih[2], *rnn_hh[2], *rnn_bih[2], *rnn_bhh[2], *mel, *mel_b, *stop_w;
  float stop_b;
  float *dec, *align, *stop;   // (B, S_cap * r, 80), (B, S_cap, T_max), (B, S_cap); zeroed by the caller
  int *steps, *status, *mlens;  // per row: steps taken, 1 = stop rule / 2 = max steps, steps * r
};
void launch_t1_decoder(const T1DecArgs& a, int B, hipStream_t s);

// gst.hip (Global Style Tokens). Row lengths (mel frames) travel as a kernel argument (RowInts).
constexpr int GST_HG_MAX = 256, GST_G_MAX = 512, GST_ES_MAX = 1024, GST_HEADS_MAX = 8, GST_TOK_MAX = 32,
              GST_DICT_MAX = 64;
// the six reference-encoder layers: mel (B, N_max, 80) -> bufB (B, W6, 2, 128), W_l = ceil(W_{l-1} / 2)
// of N_max; W[l] is [3][3][Cin][Cout] with BatchNorm folded, bias[l] the folded bias. bufA holds
// layer 1's output (B, W1, 40, 32), bufB layer 2's (B, W2, 20, 32); later layers alternate.
void launch_gst_convs(const float* mel, const RowInts& lens, int B, int N_max, const float* const* W,
                      const float* const* bias, float* bufA, float* bufB, hipStream_t s);
// GRU over x (B, W6, 256) ([mel bin][channel] features), then the style-token attention -> out (B, G).
// wihT [256][3 Hg], whhT [Hg][3 Hg] (gates r | z | n), wqT [Hg + Es][G], Kt / Vt [ntok][G];
// spk (B, Es) when the query takes the speaker embedding (Es > 0); scale = sqrt(G / heads)
struct GstHeadArgs {
  const float* x;
  long xb;
  RowInts lens;
  const float *wihT, *whhT, *bih, *bhh, *wqT, *Kt, *Vt, *spk;
  int Hg, G, heads, ntok, Es;
  float scale;
  float* out;
};
void launch_gst_head(const GstHeadArgs& a, int B, hipStream_t s);
// out (G) = sum_i w[i] Vt[id[i]] in the order given
struct GstTokenArgs {
  int n;
  int id[GST_DICT_MAX];
  float w[GST_DICT_MAX];
};
void launch_gst_tokens(const GstTokenArgs& a, const float* Vt, int G, int ntok, float* out, hipStream_t s);

// griffin_lim.hip. Row lengths travel as a kernel argument (RowInts: at most 64 rows), so a call
// needs no host-to-device copy. W = e^{-2 pi i m / 1024} (1024 complex), win = the window zero-padded to
// 1024, nonzero inside [wlo, whi); env (B, env_stride) the rows' window-square envelopes; F
// (B, M_max, 1024) windowed frames.
void launch_gl_env(float* env, const float* win, const RowInts& lens, int B, int M_max, int hop, int wlo, int whi,
                   long env_stride, hipStream_t s);
void launch_gl_frames(bool start, const float* S, const float* u, const float* Fin, float* Fout, const float* env,
                      const float* W, const float* win, const RowInts& lens, int B, int M_max, int hop, int wlo,
                      int whi, long env_stride, hipStream_t s);
void launch_gl_finish(const float* F, const float* env, float* wav, const RowInts& lens, int B, int M_max, int hop,
                      int wlo, int whi, long env_stride, hipStream_t s);
void launch_mel_to_linear(const float* mel, const RowInts& lens, int B, int M_max, int n_mels, int F, const float* inv,
                          const float* scale, const float* offset, float clip_lo, float clip_hi, int use_clip,
                          float spec_gain, float power, float* S, hipStream_t s);

// wav_tail.hip. x (B, M_max, F) normalised linear spectrograms -> S, the same shape
void launch_spec_to_mag(const float* x, const RowInts& lens, int B, int M_max, int F, const float* scale,
                        const float* offset, float clip_lo, float clip_hi, int use_clip, float spec_gain, float power,
                        float* S, hipStream_t s);
// de-emphasis: a workgroup of DE_T threads per row, each thread DE_C samples of a tile. The powers
// of the coefficient the kernel multiplies by, rounded from double: pw[k] = a^k and
// pwc[s] = a^(DE_C 2^s)
constexpr int DE_T = 512, DE_C = 16, DE_LOG = 9;  // DE_T == 1 << DE_LOG
struct DeemphTable {
  float pw[DE_C + 1];
  float pwc[DE_LOG];
};
void launch_deemphasis(const float* in, float* out, const RowInts& ns, int B, int L_max, const DeemphTable& tab,
                       hipStream_t s);
// the four launches of tts_wav_finish; smax, amax (B, nblk) hop-block maxima with nblk >=
// ceil(L_max / hop), offs (B) and factor (1) scratch
void launch_wav_finish(const float* wav, const RowInts& ns, int B, int L_max, int window, int hop, double thr, int gap,
                       float* smax, float* amax, int nblk, int* offs, float* factor, int16_t* pcm, int* ends,
                       int* total, hipStream_t s);

// stft.hip. nsamp holds the rows' sample counts (by value, as above); W = e^{-2 pi i m / n_fft}
// (n_fft complex), win = the window zero-padded to n_fft, nonzero inside [wlo, whi). fft: the
// 1024-point FFT kernel (n_fft must be 1024), else the direct DFT. out (B, M_max, n_fft / 2 + 1).
void launch_stft_frames(bool fft, const float* wav, long L_max, const RowInts& nsamp, int B, int M_max, int n_fft,
                        int hop, int wlo, int whi, float preemph, const float* W, const float* win, float* out,
                        hipStream_t s);
// mag (B, M_max, F) -> out (B, M_max, C); basis (C, F) or null (then C == F)
void launch_mag_to_feature(const float* mag, const RowInts& lens, int B, int M_max, int F, int C, const float* basis,
                           float gain, const float* scale, const float* offset, float clip_lo, float clip_hi,
                           int use_clip, float* out, hipStream_t s);

// voc_eval.hip. PQMF analysis: x (B, L_max) rows of lens samples, H (N, ntap) with ntap odd, y
// (B, N, Lout_max), row b zero past (lens[b] - 1) / N + 1 positions.
constexpr int PQ_NMAX = 8, PQ_NTAP_MAX = 255;
void launch_pqmf_analysis(const float* x, long L_max, const RowInts& lens, int B, const float* H, int N, int ntap,
                          float* y, int Lout_max, hipStream_t s);
// The windowed-DFT basis of one (n_fft, win_length) on the device, in the STFT GEMM's tile order:
// [bin tile][Kp][cos ST_TB | sin ST_TB], d[..][k][j] = hann(k) cos / -sin(2 pi f (k + woff) / n_fft),
// zero for k >= K = win_length and bins f >= F = n_fft / 2 + 1; Kp = K rounded up to the kernel's K chunk
constexpr int ST_TF = 64, ST_TB = 64, ST_KCHUNK = 32;
struct StftBasis {
  const float* d;
  int n_fft, K, Kp, woff, F, nbt;
};
// per-row sums {sum |log y_M - log yhat_M|, sum (y_M - yhat_M)^2, sum y_M^2} over the row's own frames
// into sums (B, 3) float64; partial: B * ceil(frames_max / ST_TF) * nbt * 3 floats of scratch;
// frames_max >= every row's frame count
void launch_stft_pair_sums(const float* yhat, const float* y, long L_max, const RowInts& nsamp, int B,
                           const StftBasis& W, int hop, int frames_max, float* partial, double* sums, hipStream_t s);
// mag (B, F, frames_max) = sqrt(max(re^2 + im^2, 1e-8)), zero past a row's own frames
void launch_stft_mag_store(const float* wav, long L_max, const RowInts& nsamp, int B, const StftBasis& W, int hop,
                           float* mag, int frames_max, hipStream_t s);
