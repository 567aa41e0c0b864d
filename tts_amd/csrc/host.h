// Host side of the library, shared by the api_*.hip files: device buffers, staged host tensors,
// packed conv layers, the models and their workspaces, the context, and the per-call helpers of
// the C ABI entry points. Everything but tts_ctx (an opaque type of ttship.h) is in namespace ttsh.
#pragma once
#include "common.h"
#include "launch.h"
#include "../../include/ttship.h"

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

struct DecCtlBlock;  // decoder.h
struct DecDev;

namespace ttsh {

constexpr int CHUNK = 8;  // decoder steps per captured graph (even: parity of t == parity of j)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  // grow-only; returns true when the address changed
  bool ensure(size_t n) {
    if (n <= bytes && p) return false;
    if (p) HIP_OK(hipFree(p));
    p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(n, 256)));
    bytes = std::max<size_t>(n, 256);
    return true;
  }
  template <class T>
  void upload(const std::vector<T>& v) {
    ensure(v.size() * sizeof(T));
    HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  void reset() {
    if (p) HIP_OK(hipFree(p));
    p = nullptr;
    bytes = 0;
  }
  float* f() const { return static_cast<float*>(p); }
  int* i() const { return static_cast<int*>(p); }
  const uint16_t* h() const { return static_cast<const uint16_t*>(p); }
};
template <class T>
void ensure(DevBuf& b, size_t n) {  // room for n elements of T
  b.ensure(n * sizeof(T));
}

// Per-call row values (lengths, ids) to the device, on stream s: a one-block kernel takes them by
// value (RowInts), BMAX per launch, so nothing reads the host array after the call returns and no
// copy from pageable memory stalls the stream. put_rows returns dst; fill_rows writes n copies of
// one value. The DevBuf forms grow dst to n ints first.
inline RowInts row_ints(const int32_t* h, int n) {  // n <= BMAX values, the rest zero
  RowInts r{};
  std::copy(h, h + n, r.v);
  return r;
}
const int* put_rows(int* dst, const int32_t* h, int n, hipStream_t s);
const int* put_rows(DevBuf& dst, const int32_t* h, int n, hipStream_t s);
const int* fill_rows(DevBuf& dst, int value, int n, hipStream_t s);
// every h[b], b < n, inside [lo, hi], or msg is thrown
void check_rows(const int32_t* h, int n, long lo, long hi, const std::string& msg);

// split-f16 A fragments (split16.h pack_split_a) of a row-major (rows x K) matrix, rows and K
// multiples of 16 and 32; the buffer stays empty when a weight is outside the f16 range (the
// kernels then take their fp32 path)
void upload_split_rows(DevBuf& d, const std::vector<float>& w, int rows, int K);

struct HostT {
  std::vector<float> d;
  std::vector<int64_t> shape;
};
using HostMap = std::map<std::string, HostT>;

const HostT& need(const HostMap& m, const std::string& k, std::vector<int64_t> shape);
// name.weight, or weight_norm's name.weight_v / name.weight_g folded
std::vector<float> wn_weight(const HostMap& m, const std::string& name, std::vector<int64_t> shape);
// the body of every tts_*_set_tensor: stages a host tensor in one model's map
int stage_tensor(tts_ctx* c, HostMap tts_ctx::*staged, const char* name, const float* h, const int64_t* shape,
                 int ndim);
// finalize consumes the tensors staged by *_set_tensor, so the next model starts from an empty map
struct HostMapConsumer {
  HostMap& m;
  ~HostMapConsumer() { m.clear(); }
};

struct ConvLayer {
  DevBuf W, bias;
  int Cin = 0, Cout = 0, Cout_pad = 0, K = 1, dil = 1, tile = 0, nphase = 1;
  int pad_left[8] = {0};
  long phase_stride = 0;
  DevBuf W16;             // split-f16 A fragments (conv_x3.hip); empty when the shape is not covered
  long w16_stride = 0;    // bytes per phase
};

// Wm: nphase blocks of [Cout][Cin*K] row-major
void pack_conv(ConvLayer& L, const std::vector<float>& Wm, const std::vector<float>& bias, int Cin, int Cout,
               int K, int dil, int nphase, const int* pad_left);
// split-f16 weights only (a layer that has no fp32 form: the phase-merged ConvTranspose)
void pack_conv_x3_only(ConvLayer& L, const std::vector<float>& Wm, const std::vector<float>& bias, int Cin, int Cout,
                       int K);

// The two activation layouts as {batch, channel, time} strides in elements
struct Layout {
  long b;
  int c, t;
};
inline Layout bct(int C, long T) { return {(long)C * T, (int)T, 1}; }  // (B, C, T)
inline Layout btc(long T, int C) { return {T * C, 1, C}; }              // (B, T, C)

// One conv launch. conv_call() (below) starts a record; in / in2 / to / add set the sources, the
// output and the residual by pointer + layout; everything else is set by name at the site.
struct ConvCall {
  ConvCall& in(const float* p, Layout l, int C, int act = 0) { return s[0] = ConvSrc{p, l.b, l.c, l.t, C, act}, *this; }
  ConvCall& in2(const float* p, Layout l, int C) { return s[1] = ConvSrc{p, l.b, l.c, l.t, C, 0}, nsrc = 2, *this; }
  ConvCall& to(float* p, Layout l) { return out = p, ob = l.b, oc = l.c, ot = l.t, *this; }
  ConvCall& add(const float* p, Layout l) { return resid = p, rb = l.b, rc = l.c, rt = l.t, *this; }
  ConvSrc s[2];
  int nsrc = 1;
  int pad_mode = 0;
  const int* lens = nullptr;
  int len_add = 0, in_mul = 1, q_mul = 1, rep_pad = 0, out_mul = 1;
  float* out = nullptr;
  long ob = 0;
  int oc = 0, ot = 0;
  int epi = 0;
  const float* resid = nullptr;
  long rb = 0;
  int rc = 0, rt = 0, resid_rows = 0;
  const float* aux = nullptr;
  long auxb = 0;              // epi 3: batch stride of the per-utterance gate bias in aux
  int max_q = 0, B = 0;
  unsigned* oflow = nullptr;  // set: run the split-f16 kernel where the layer has split weights
  int merged_u = 0;           // phase-merged ConvTranspose (layer from pack_conv_x3_only)
};

// which kernel a run_conv launched: the split-f16 one (conv_x3.hip) or the fp32 one (conv.hip), and
// its tile width in output positions (0: nothing was launched)
struct ConvRan {
  bool x3 = false;
  int tq = 0;
};
ConvRan run_conv(const ConvLayer& L, const ConvCall& c, hipStream_t st);

// ConvTranspose1d(k = 2u, stride u, padding u / 2) from its weight wt (Cin, Cout, 2u) and bias:
// L = the u polyphase 2-tap convs (Wm [u][Cout][Cin][2], pad_left per phase), Lm = the phase-merged
// split-f16 form (ConvCall::merged_u), left without weights where the merged GEMM's u * Cout rows
// are not covered or a weight is outside the f16 range
void pack_convT(ConvLayer& L, ConvLayer& Lm, const std::vector<float>& wt, const std::vector<float>& bias, int u,
                int Cin, int Cout);

// weight layout helpers: LSTM gate rows regrouped per 4-unit tile, column blocks of matrices with
// equal row counts concatenated, a column range, swizzle_rows16 with the rows padded to 16, and a
// ConvBN block's batch norm folded into its conv
std::vector<float> lstm_tile_rows(const std::vector<float>& W, int H, int K);
std::vector<float> hcat(const std::vector<std::pair<const float*, int>>& parts, int rows);
std::vector<float> slice_cols(const std::vector<float>& W, int rows, int K, int c0, int c1);
std::vector<float> swz(const std::vector<float>& Wm, int rows, int K);
void fold_convbn(const HostMap& m, const std::string& pfx, int Cin, int Cout, int K, std::vector<float>& Wm,
                 std::vector<float>& bias);

// ---------------------------------------------------------------- Tacotron2 -----------
struct TacoModel {
  bool ready = false;
  int num_chars = 0, r_init = 7, softmax = 0;
  DevBuf emb;
  ConvLayer enc[3], lstm_in, penc, post[5];
  DevBuf whhT;
  DevBuf whhT16;  // W_hh split-f16 for the persistent BiLSTM (empty if out of the f16 range)
  DevBuf pre1, pre2, att_p, att_pre, att_bias, dec_w, dec_bias, WqT, Wloc, Wdense, v, proj_w, proj_b;
  // split-f16 forms for the persistent decoder (P3 prenet part, P5 ctx parts); empty if out of range
  DevBuf att_p_x3, dec_x3, apre_x3, pj_x3;
  DevBuf Wcomb;  // location_dense . location_conv folded, [64 taps (62 used)][128 dims]
  float bv = 0.f;
  // persistent decoder: projection rows [stop tile | W_p] (+ bias) and prenet layer 1 on the host,
  // folded per r into pj_w / pj_b = [stop tile | first 80r rows of W_p | W1 W_p,last frame]
  std::vector<float> proj_rows, proj_bias, pre1_host;
  DevBuf pj_w, pj_b;
  int pj_r = -1;
  // multi-speaker (models/tacotron2.py:50-58, 152-155): the speaker vector s is constant over the
  // encoder positions and the attention weights of a step sum to 1, so every ctx-fed GEMM splits
  // into its 512 encoder columns plus W_s s, a per-utterance bias. Host copies of the speaker
  // columns (rows in the kernels' order), spk_dim x ... each; spk_wT = [spk_dim][NSPK] for pj_r.
  int spk_dim = 0, num_spk = 0;
  // decoder variants (common_layers.py:25-74, 196-372): BN prenet folded into the prenet weights
  // (+ biases), windowing / forward attention / transition agent flags
  bool prenet_bn = false, windowing = false, forward_attn = false, trans_agent = false, forward_attn_mask = false;
  std::vector<float> pre1_bias;  // b1' (BN), folded into the projection's prenet rows
  DevBuf pre1_b0, pre2_b, ta_w;
  float ta_b = 0.f;
  bool variant() const { return prenet_bn || windowing || forward_attn || graves; }
  // Graves attention (common_layers.py:113-193): N_a layer 1 as 64 swizzled 16-row tiles of the
  // P3g GEMM (K = 1024), its bias, layer 2 (3K x 1024, row-major) and bias
  bool graves = false;
  int graves_K = 0;
  DevBuf na1_w, na1_b, na2_w, na2_b;
  DevBuf spk_table;  // speaker_embedding.weight (num_spk, 512) when learned
  std::vector<float> spk_att_h, spk_dec_h, spk_penc_h, proj_spk;
  DevBuf spk_wT;
  // Global Style Tokens (gst.hip; gst_layer.* present): the style vector of gst_dim sits in front of
  // the speaker vector in the decoder's input, so spk_dim = gst_dim + es is the conditioning width
  // and the per-row bias fold takes [style | speaker]. es = the speaker vector's own width.
  int gst_dim = 0, gst_heads = 0, gst_ntok = 0, gst_es_q = 0, es = 0;
  DevBuf gst_cw[6], gst_cb[6];  // reference-encoder convs [3][3][Cin][Cout], BatchNorm folded
  DevBuf gst_wihT, gst_whhT, gst_bih, gst_bhh, gst_wqT, gst_K, gst_V;
};

// style encoder workspace: the conv layers' ping-pong buffers (tts_taco_style_mel)
struct GstWS {
  DevBuf a, b;
};

// Tacotron2 status words (TacoWS::stat on the device, tts_ctx::pinned on the host; one copy after
// the call): BiLSTM barrier errors (one per recurrence: 2 directions x up to 2 row groups),
// persistent-decoder barrier errors (one per launch), the decoder results (done, steps, status per
// decode row: DecCtlBlock's three arrays), the range flag, the launches' end steps
constexpr int PMAX_LAUNCH = 4;  // persistent decoder launches per decode (MT = 4, 3, 2, 1)
constexpr int PBAR_CAND = 16;   // candidate barrier blocks timed for them
constexpr int ENC_NDOM_MAX = 4;  // BiLSTM recurrences (barrier blocks) per launch
constexpr int TS_ENC = 16, TS_DEC = TS_ENC + ENC_NDOM_MAX, TS_RES = TS_DEC + PMAX_LAUNCH, TS_FLAG = TS_RES + 3 * BMAX,
              TS_END = TS_FLAG + 1, TS_VERR = TS_END + PMAX_LAUNCH, TS_N = TS_VERR + 1;
// The pinned status page (tts_ctx::pinned, PIN_N ints), by region:
//   [PIN_CHUNK, + 4)            graph decoder chunk polling: {all_done, active_tiles} of chunk parity 0 / 1
//   [PIN_FLAG]                  range flag of the call (with_x3_fallback)
//   [TS_ENC, TS_N)              status words of the last Tacotron2 call (one copy of TacoWS::stat)
//   [PIN_ENC, + ENC_NDOM_MAX)   BiLSTM barrier error words of tts_taco_encoder
//   [TK_PIN, + NVT)             range flag of the vocoder of ticket slot k
constexpr int NVT = 4;  // fused-call ticket slots
constexpr int PIN_CHUNK = 0, PIN_FLAG = 12, PIN_ENC = 240, TK_PIN = 248, PIN_N = 256;
static_assert(PIN_CHUNK + 4 <= PIN_FLAG && PIN_FLAG < TS_ENC && TS_N <= PIN_ENC && PIN_ENC + ENC_NDOM_MAX <= TK_PIN &&
                  TK_PIN + NVT <= PIN_N,
              "pinned page regions overlap or leave the page");

struct TacoWS {
  int B = 0, T_max = 0, S_cap = 0, r = 0, MT = 0;
  long gen = 0;
  DevBuf lens, mlens, x0, ca, cb, gin, enc, penc;
  DevBuf lh, lc;  // BiLSTM h (2 buffers x 2 directions, fragment order) and c
  DevBuf p1, pb, gatt, hatt, catt, hdec0, hdec1, cdec, ctx, y, pq, spart, alpha, acum, energy, ctl;
  DevBuf dec, align, stop, pa, pbb;
  DevBuf aps, apm, apu, acnt;  // attention chunk partials + per-utterance arrival counters
  DevBuf post, map;            // rows in decode order (longest first); map = [perm | inverse]
  DevBuf stat;                 // status words for the host, laid out as tts_ctx::pinned (TS_*)
  DevBuf ypart, pbar;          // persistent decoder: projection halves, grid-barrier words
  // the decoder launches' barrier blocks: PBAR_CAND candidates in pbar, the PMAX_LAUNCH fastest
  // picked once per allocation (pick_barrier_blocks)
  int pslot[PMAX_LAUNCH] = {0, 1, 2, 3};
  const void* pslot_base = nullptr;
  bool pslot_cal = false;      // pslot timed (after enter(), on the first persistent decode of these blocks)
  DevBuf anorm;                // persistent decoder: per-utterance attention normaliser (deferred alignment)
  DevBuf spk, spkid, spkb;     // conditioning vectors (decode order), per-row biases [Bp][NSPK]
  DevBuf spk_only;             // GST models: the speaker vectors alone, before [style | speaker] is built
  DevBuf win_idx, fwd_u, apf;  // windowing argmax, transition probability, forward chunk sums
  DevBuf gh, gmu;              // Graves: N_a hidden (32 x 1024), mixture means (64 x 16)
  DevBuf teach;                // teacher-forced decode: prenet layer 1 of the ground-truth frames [S_cap][Bp][256]
  DevBuf trace, xdiag;         // TTS_PTRACE / TTS_DIAG_XCC diagnostics, on this context's device
  bool enc_persist = false;    // the last encoder ran the persistent BiLSTM (lc = its barrier words)
  int enc_ndom = 0;            // its recurrences (directions x row groups), one barrier block each
  // one CHUNK-step graph per batch-tile count MT' <= MT (the batch tile shrinks as the
  // longest-first rows finish); all share one configuration key
  hipGraphExec_t graphs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  long graph_gen = -1;
  int gB = -1, gT = -1, gS = -1, gr = -1;
  float thr = 0.5f, gthr = -1.f;
};

struct MelganModel {
  bool ready = false;
  int in_ch = 80, out_ch = 4, base = 384, nres = 4, pqmf = 1, taps = 62;
  std::vector<int> ups;
  ConvLayer conv_in, conv_out;
  std::vector<ConvLayer> convT;
  std::vector<ConvLayer> convTm;  // phase-merged split-f16 form (conv_x3.hip merged_u), W16 only
  std::vector<ConvLayer> dconv, fused;  // [stage*nres + block]
  std::vector<DevBuf> rb_wd16, rb_wf16;  // split-f16 block weights (resblock_x3.hip), empty if C unsupported
  std::vector<DevBuf> rb_wd16p;          // phase-1 weights in the packed order (C % 32 == 16), for resstack_x3
  DevBuf G;
  DevBuf out_w, out_b;  // conv_out as [c][k][o] for the fused output + PQMF kernel
  int C_last = 0;
};

// what run_generator leaves when the output conv is left to the fused PQMF kernel
struct GenTail {
  const float* x = nullptr;  // last ResidualStack output (B, C, Ls), before LReLU
  int C = 0;
  long Ls = 0;
  int mul = 1;
};

struct MelganWS {
  DevBuf lens, xa, xb, bands;
};

// GE2E speaker encoder (TTS/speaker_encoder/model.py:5-80): 3 x [LSTM(in -> 768), Linear(768 -> 256,
// no bias)] (use_lstm_with_projection) or one 3-layer LSTM + Linear(bias) + ReLU on the last hidden
// state; the embedding is the L2-normalised output at each sequence's last frame.
struct Ge2eModel {
  bool ready = false;
  int in_dim = 40, in_pad = 48, proj = 256, H = 768, nl = 3, with_proj = 1;
  ConvLayer gin[4];      // input projections (K = 1, Cout = 4H gate-interleaved tiles, b_ih + b_hh)
  DevBuf whh[4];         // W_hh, swizzled tiles
  DevBuf whh16[4];       // W_hh split-f16 (empty if out of the f16 range)
  ConvLayer proj_l[4];   // with_proj: Linear(768 -> proj) per layer as a K = 1 conv
  DevBuf lin_w, lin_b;   // without projection: final Linear (proj x H) + bias
  // layer pipeline (encoder.hip ge2e_pipe_kernel): layer l >= 1 as split-f16 [W_hh | W_in] rows
  // (W_in = W_ih^l W_proj^{l-1} folded in fp64, or W_ih^l) and b_ih + b_hh, tile order
  DevBuf wpipe[4], bpipe[4];
  bool pipe_ok = false;
};

struct Ge2eWS {
  DevBuf x, lens, g, o, p, bar, hbuf;
};

// Glow-TTS (TTS/tts/models/glow_tts.py, the reference configs' gated-conv encoder, mean_only,
// num_sqz 2, num_splits 4, dilation 1; optional speaker conditioning)
struct GlowModel {
  bool ready = false;
  int num_chars = 0, H = 192, Fdp = 256, C = 80, enc_layers = 9, flows = 12, wn_layers = 4;
  DevBuf emb;                                   // scaled by sqrt(H)
  std::vector<ConvLayer> enc_conv;              // H -> 2H, k5
  std::vector<DevBuf> enc_g, enc_b;             // LayerNorm(2H)
  // time-depth-separable encoder (configs/glow_tts_tdsep.json): ConvLayerNorm prenet, then per
  // layer time_conv (H -> 2H, BN folded, rows interleaved for the GLU epilogue), depthwise k5 (BN
  // folded) + swish, time_conv2 (BN folded) + residual
  bool tdsep = false, tfm = false;
  // transformer encoder: per layer q|k|v as one 1x1 conv (H -> 3H), o (1x1), FFN k3 (H -> 768 -> H)
  std::vector<ConvLayer> tfm_qkv, tfm_o, tfm_f1, tfm_f2;
  std::vector<DevBuf> tfm_g1, tfm_b1, tfm_g2, tfm_b2;
  std::vector<ConvLayer> pre_conv, tds_tc, tds_tc2;
  std::vector<DevBuf> pre_g, pre_b, tds_dw, tds_dwb;
  ConvLayer pre_proj;
  ConvLayer proj_m, dp1, dp2, dp_proj;
  DevBuf dp_g1, dp_b1, dp_g2, dp_b2;
  // per flow block (index = block): start (C -> H), WN in (H -> 2H, k5, rows interleaved), res+skip
  // (H -> 2H, last layer H -> H skip), end (H -> 2C, rows interleaved) whose epilogue also applies
  // the inverse InvConvNear + ActNorm from invtab (2C x {w[4], bias, exp(-logs)})
  std::vector<ConvLayer> start, end;
  std::vector<DevBuf> invtab;
  // forward direction (GlowTts.forward): per block 2C x {w[s'][0..3], actnorm bias, exp(actnorm logs)}
  // for the ActNorm + InvConvNear ahead of the block, and the weight-only part of the
  // log-determinant per squeezed frame, sum_k [sum_c actnorm.logs_k + logdet(W_k) * 2C / 4]
  std::vector<DevBuf> fwdtab;
  double fwd_logdet_frame = 0.0;
  std::vector<ConvLayer> wn_in, wn_rs;  // [block * wn_layers + i]
  // speaker conditioning (glow_tts.py:97-99,159-161; encoder.py:131-135; glow.py:87-91,119-130):
  // c_in channels of g padded to c_pad (multiple of 16); the duration predictor's conv_1 reads
  // [x; g] (g broadcast over time by a time stride of 0); every block's cond_layer stacked into one
  // 1x1 conv (c_pad -> flows * wn_layers * 2H, rows interleaved like wn_in) whose output is the
  // per-utterance gate bias of each WN in-layer
  int c_in = 0, c_pad = 0, n_spk = 0;
  DevBuf emb_g;
  ConvLayer cond;
};

struct GlowWS {
  int B = 0, Tx = 0, Ty = 0;
  DevBuf ids, lens, klens, ylens, xa, xb, h2, hdp, logw, cum, wceil, om, z, sq, sq2, whs, wacts, big;
  DevBuf spk, ones, g, gcond;  // speaker ids, unit lengths, normalized g (B, c_pad), cond biases
  bool has_g = false;          // the last glow_encode was given speaker ids
  std::vector<int> h_xlens, h_ylens;  // the last glow_encode's lengths, for glow_decode / glow_align
  // GlowTts.forward (glow_align) and the stand-alone alignment search (glow_mas): even mel lengths,
  // their halves, the end conv's plain output, log-determinant partials, the likelihood matrix, the
  // search's decision words and the frame -> token map
  DevBuf aylens, aklens, eo, ldpart, logp, masbits, xof, mxl, myl;
};

// ParallelWaveGAN generator (TTS/vocoder/models/parallel_wavegan_generator.py, setup_generator's
// configuration: 64 res / 128 gate / 64 skip / 80 aux channels, kernel 3)
struct PwganModel {
  bool ready = false;
  int layers = 30, stacks = 3;
  std::vector<int> ups;
  DevBuf first_w, first_b;
  ConvLayer conv_in;                 // 80 -> 80, k1, no bias
  std::vector<DevBuf> up_h;          // per factor s: 2s + 1 taps
  std::vector<DevBuf> W1, b1, W2, b2;  // per residual block (pw_layer_kernel layouts)
  std::vector<DevBuf> W1x, W2x;        // split-f16 forms (pw_layer_x3_kernel); empty if out of range
  DevBuf W3, b3, w4, b4;
};

struct PwganWS {
  DevBuf lens, ca, cb, xa, xb, skip, zeros;
};

// Tacotron v1 (TTS/tts/models/tacotron.py; api_tacotron1.hip, tacotron1.hip): CBHG encoder, GRU
// decoder, CBHG postnet + last_linear. Conv weights are [K][Cin][Cout] with their BatchNorm folded,
// linear and GRU matrices transposed ([in][out]) except the sequence GRU's W_hh ([dir][384][128]).
struct T1Cbhg {
  int Cin = 0, K = 0, P0 = 0, P1 = 0;
  std::vector<DevBuf> bank_w, bank_b;
  DevBuf pj1_w, pj1_b, pj2_w, pj2_b, pre_hw, hw_w, hw_b, gru_wih, gru_bih, gru_whh, gru_bhh;
};

struct T1Model {
  bool ready = false;
  int num_chars = 0, r_init = 5, mem_frames = 5, softmax = 0, post_dim = 1025;
  DevBuf emb, epre1_w, epre1_b, epre2_w, epre2_b;
  T1Cbhg enc, post;
  DevBuf pre1, pre1_b, pre2, pre2_b, att_ih, att_hh, att_bih, att_bhh, wq, win, wcomb, v, pdi, pdi_b;
  DevBuf rnn_ih[2], rnn_hh[2], rnn_bih[2], rnn_bhh[2], mel, mel_b, stop_w, last_w, last_b;
  float bv = 0.f, stop_b = 0.f;
};

struct T1WS {
  DevBuf lens, msteps, ctl, x0, x1, x2, bank, p1, p2, hw, gin, enc, pin, gout;
};

// Griffin-Lim (griffin_lim.hip): twiddles, the window of the last call's win_length, the two
// ping-pong frame buffers (B, M_max, 1024) and the rows' window-square envelopes
struct AudioWS {
  DevBuf W, win, fa, fb, env;
  int win_length = -1;
  // analysis (stft.hip): twiddles e^{-2 pi i m / n_fft} and the window of the last tts_stft_mag call
  DevBuf sW, swin;
  int s_nfft = -1, s_win = -1;
  // tts_wav_finish (wav_tail.hip): hop-block maxima, row offsets and the scale factor
  DevBuf tail;
};

// Vocoder scoring (voc_eval.hip): the DFT bases by (n_fft, win_length), kept for the context's
// life, and the per-tile partial sums of the last tts_stft_pair_sums call
struct VocEvalWS {
  struct Basis {
    DevBuf d;
    int Kp = 0, nbt = 0;
  };
  std::map<std::pair<int, int>, Basis> bases;
  DevBuf partial;
};

// one submitted fused call: what its fp32 re-run needs if the split-f16 vocoder raised the range
// flag (the caller keeps d_post and d_wav untouched until the ticket is finished)
struct VocTicket {
  int64_t id = 0;
  bool pending = false;       // not finished: the caller's stream is not yet ordered after the vocoder
  bool x3 = false;            // vocoder launched on split-f16 kernels: its range flag is to be looked at
  hipEvent_t ev = nullptr;    // recorded after the vocoder, the copy of its flag and the row packing
  const float* d_post = nullptr;
  int64_t st[3] = {0, 0, 0};
  std::vector<int32_t> lens;  // decoded mel lengths, caller order
  int B = 0, M = 0, pad = 0;
  float* d_wav = nullptr;
};

}  // namespace ttsh

struct tts_ctx {
  std::recursive_mutex mu;  // held by every entry point (guarded_ctx)
  int device = 0;
  hipStream_t s = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_chunk[2] = {nullptr, nullptr};
  hipEvent_t ev_dec[ttsh::PMAX_LAUNCH + 1] = {};  // around the persistent decoder launches
  hipEvent_t ev_status = nullptr;  // a fused call's decode status words are on the host
  int* pinned = nullptr;  // [PIN_N] host-pinned status page (regions: PIN_* / TS_* / TK_PIN above)
  bool flag_read = false; // the entry point already fetched the range flag into pinned[PIN_FLAG]
  int dec_end[ttsh::PMAX_LAUNCH] = {};  // step index after each persistent launch of the last decode
  int dec_path = 0;       // last decode: 0 = step graphs, 1 = persistent kernel
  bool dec_presplit = false;  // last persistent decode published h_att / ctx / h_dec pre-split
  // GEMM arithmetic: true = split-f16 MFMA kernels where built (fp32-accurate, split16.h), false =
  // fp32 MFMA everywhere (tts_set_gemm_mode; TTS_GEMM=f32 in the environment starts a context so)
  bool gemm_x3 = true;
  long x3_fallbacks = 0;  // calls re-run in fp32 because an operand left the f16 range
  ttsh::DevBuf x3flag;    // range flag raised by split-f16 kernels during one call (with_x3_fallback)
  int dec_nlaunch = 0;
  ttsh::HostMap taco_host, mg_host;
  ttsh::TacoModel taco;
  ttsh::TacoWS tws;
  ttsh::GstWS gstws;
  ttsh::MelganModel mg;
  ttsh::MelganWS mws;
  ttsh::HostMap ge2e_host;
  ttsh::Ge2eModel ge2e;
  ttsh::Ge2eWS gws;
  ttsh::HostMap pw_host;
  ttsh::PwganModel pw;
  ttsh::PwganWS pws;
  ttsh::HostMap glow_host;
  ttsh::GlowModel glow;
  ttsh::GlowWS glws;
  ttsh::AudioWS aws;
  ttsh::VocEvalWS vews;
  ttsh::HostMap t1_host;
  ttsh::T1Model t1;
  ttsh::T1WS t1ws;
  // last decode configuration (for tts_time_decoder_kernel)
  int last_B = 0, last_T = 0, last_S = 0, last_r = 0;
  // fused Tacotron2 + MB-MelGAN submissions whose vocoder may still run (tts_taco_mbmelgan_submit)
  ttsh::VocTicket vt[ttsh::NVT];
  int64_t next_ticket = 1;
  // the fused submissions' vocoders run on sv (TTS_VOC_STREAM=0: sv is s), behind their decode's
  // status event, so the next submission's Tacotron2 on s overlaps them. Each ticket slot has its own
  // device lengths and range flag (vslot: [NVT][BMAX] lengths, then NVT flags). Every other entry
  // joins sv first (enter); a fused submission's Tacotron2 does not (enter's join_voc).
  hipStream_t sv = nullptr;
  hipEvent_t ev_sv = nullptr;  // after the last vocoder enqueued on sv
  bool sv_live = false;        // sv may hold work that s has not joined
  ttsh::DevBuf vslot;
};

namespace ttsh {

inline int* vslot_lens(tts_ctx* c, int k) {
  c->vslot.ensure((size_t)NVT * (BMAX + 1) * 4);
  return reinterpret_cast<int*>(c->vslot.p) + k * BMAX;
}
inline unsigned* vslot_flag(tts_ctx* c, int k) {
  c->vslot.ensure((size_t)NVT * (BMAX + 1) * 4);
  return reinterpret_cast<unsigned*>(c->vslot.p) + NVT * BMAX + k;
}

// range flag for the split-f16 kernels of the current call, or null (fp32 kernels)
inline unsigned* x3_flag(tts_ctx* c) {
  if (!c->gemm_x3) return nullptr;
  c->x3flag.ensure(4);
  return reinterpret_cast<unsigned*>(c->x3flag.p);
}

// a conv over B rows of lens (device) positions, max_q of them at most, on the context's kernels:
// split-f16 with the call's range flag, or fp32
inline ConvCall conv_call(tts_ctx* c, const int* lens, int B, int max_q) {
  ConvCall cc;
  cc.lens = lens;
  cc.B = B;
  cc.max_q = max_q;
  cc.oflow = x3_flag(c);
  return cc;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int d) {
    HIP_OK(hipGetDevice(&prev));
    if (prev != d) HIP_OK(hipSetDevice(d));
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// stream ordering with the caller's stream (nothing to wait for when all of its work is complete:
// a server loop's stream holds only waits on this context's own finished events)
// join_voc: wait for the fused submissions' vocoders on sv first (all but a fused submission's decode)
void enter(tts_ctx* c, void* stream, bool join_voc = true);
void leave(tts_ctx* c, void* stream);

// the Tacotron2 workspace's form of ensure<T>: counts the reallocations its cached graphs depend on
template <class T>
bool grow(DevBuf& b, size_t n, long& gen) {
  if (b.ensure(n * sizeof(T))) {
    gen++;
    return true;
  }
  return false;
}

// The fp32 re-run of work whose split-f16 kernels raised the range flag: counts the fallback and
// keeps the context on the fp32 kernels for the guard's lifetime
struct Fp32Rerun {
  tts_ctx* c;
  explicit Fp32Rerun(tts_ctx* c_) : c(c_) {
    c->x3_fallbacks++;
    c->gemm_x3 = false;
  }
  ~Fp32Rerun() { c->gemm_x3 = true; }
};

// Runs fn, which enqueues vocoder kernels on c->s; split-f16 kernels among them raise the
// workspace's range flag when an operand falls outside the f16 range (split16.h). If it was
// raised, fn runs again on the fp32 kernels, so results are always fp32-accurate. Costs one
// stream synchronisation per call while split-f16 is on. fn must be re-runnable (it rewrites
// all of its outputs).
template <class F>
void with_x3_fallback(tts_ctx* c, F&& fn) {
  if (!c->gemm_x3) {
    fn();
    return;
  }
  unsigned* flag = x3_flag(c);
  HIP_OK(hipMemsetAsync(flag, 0, 4, c->s));
  c->flag_read = false;
  fn();
  if (!c->flag_read) {  // fn may have fetched it with its own status words (taco_run)
    HIP_OK(hipMemcpyAsync(&c->pinned[PIN_FLAG], flag, 4, hipMemcpyDeviceToHost, c->s));
    HIP_OK(hipStreamSynchronize(c->s));
  }
  c->flag_read = false;
  if (c->pinned[PIN_FLAG]) {
    Fp32Rerun f32(c);
    fn();
  }
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    tts_set_error(e.what());
    return 1;
  } catch (...) {
    tts_set_error("unknown error");
    return 1;
  }
}

// Entry points that take a context hold its mutex for the whole call: a context owns one
// workspace, one internal stream, cached graphs and pinned polling words, so two host threads
// (ctypes releases the GIL) must not interleave inside it. Recursive so that helpers may re-enter.
template <class F>
int guarded_ctx(tts_ctx* c, F&& f) {
  if (!c) {
    tts_set_error("null ctx");
    return 1;
  }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  return guarded(std::forward<F>(f));
}

// The common frame of an inference entry point: `pre` holds the argument checks, which run before
// anything touches a device or a stream; `fn` enqueues the work on c->s.
template <class Pre, class F>
int ctx_call(tts_ctx* c, void* stream, Pre&& pre, F&& fn) {
  return guarded_ctx(c, [&] {
    pre();
    DeviceGuard g(c->device);
    enter(c, stream);
    with_x3_fallback(c, fn);
    leave(c, stream);
  });
}

// --- Tacotron2: api_taco_load.hip (workspace, per-r projection fold), api_taco.hip (taco_run),
// api_taco_graph.hip (the captured-graph decoder), api_gst.hip (Global Style Tokens)
void taco_workspace(tts_ctx* c, int B, int T_max, int S_cap, int r);
void build_pj(tts_ctx* c, int r);
// the decoder's control block and per-launch device view (decoder.h), shared by both decoders
DecCtlBlock* ctl_block(const TacoWS& W);
DecDev make_dev(tts_ctx* c, int Bact);
// the decode as captured CHUNK-step graphs (decoder.hip's per-step kernels), polled by the host
void run_graph_decoder(tts_ctx* c, int B, int T_max, int S_cap, int r, float thr, int max_ms, hipStream_t s);
// the vocoder half of a fused Tacotron2 + MB-MelGAN call: the decode's status kernel writes the
// vocoder's lengths into vlens (device, caller order), and enqueue() launches the vocoder on them
// before the host waits for the status words, so the GPU runs both models back to back
constexpr const char* VOC_SHORT_MSG =
    "MB-MelGAN: a decoded mel is shorter than the vocoder's reflection pads allow (ReflectionPad1d(3): mel frames "
    "+ 2*padding must be >= 4; a residual stack's dilation must be < the first stage's length)";
struct FusedVoc {
  int* vlens;
  int Lmin;
  std::function<void()> enqueue;
};

// One Tacotron2 call, filled once by its extern "C" entry point (d_*: device, h_*: host; rows in the
// caller's order). Free-running part: a row stops at its stop token (thr) or after h_max_steps[b] <=
// S_cap steps, h_steps / h_status receive the rows' results; fv: a fused call's vocoder, or null.
struct TacoFree {
  const int32_t* h_max_steps = nullptr;
  int S_cap = 0;
  float thr = 0.5f;
  int32_t *h_steps = nullptr, *h_status = nullptr;
  const FusedVoc* fv = nullptr;
};
// Teacher-forced part (Tacotron2.forward in eval): d_mel (B, M_max, 80), M_max a multiple of r; row b
// runs ceil(h_mel_lens[b] / r) steps.
struct TacoTeach {
  const float* d_mel = nullptr;
  const int32_t* h_mel_lens = nullptr;
  int M_max = 0;
};
struct TacoCall {
  const int64_t* ids = nullptr;
  const int32_t* h_lens = nullptr;
  int B = 0, T_max = 0, r = 0;
  const int64_t* d_spk_ids = nullptr;  // speaker ids or embeddings: multi-speaker models
  const float* d_spk_emb = nullptr;
  const float* d_style = nullptr;  // (B, gst_dim), or null (zeros): GST models only
  float *d_dec = nullptr, *d_post = nullptr, *d_align = nullptr, *d_stop = nullptr;
  void* stream = nullptr;
  TacoFree run;                      // read when teach is null
  const TacoTeach* teach = nullptr;  // set: the teacher-forced decode
};
void taco_run(tts_ctx* c, const TacoCall& k);

// Global Style Tokens, load: gst_layer.* folded and uploaded, key / value tables built (api_gst.hip)
void gst_load(tts_ctx* c);

// --- MelGAN: api_melgan.hip, for the fused path
// One vocoder run. dev_lens: the device lengths buffer already holds the lengths (a fused call's
// decode wrote them, checked there against vocoder_min_len); h_lens are then per-row upper bounds,
// used for tile counts. A fused submission's vocoder brings its ticket slot's buffers.
struct VocCall {
  const float* mel = nullptr;
  const int64_t* mel_strides = nullptr;  // {batch, channel, frame}, or null: (B, in_ch, M_max) contiguous
  const int32_t* h_lens = nullptr;
  int B = 0, M_max = 0, pad = 0;
  bool dev_lens = false;
  hipStream_t s = nullptr;   // null: c->s
  int* d_lens = nullptr;     // device lengths buffer; null: the workspace's
  unsigned* flag = nullptr;  // range flag of the split-f16 kernels; null: the context's
};
// returns total upsampling factor; writes bands (B, out_ch, up*(M_max+2pad)) into `out`
int run_generator(tts_ctx* c, const VocCall& v, float* out, GenTail* tail = nullptr);
// MultibandMelganGenerator.inference body: generator, output conv and PQMF synthesis into
// d_wav (B, 1, hop * (M_max + 2 pad)), rows zero past their own length
void mbmelgan_body(tts_ctx* c, const VocCall& v, float* d_wav);
// the shortest mel (frames) the vocoder accepts at inference padding pad: run_generator's checks
int vocoder_min_len(const MelganModel& G, int pad);

}  // namespace ttsh
