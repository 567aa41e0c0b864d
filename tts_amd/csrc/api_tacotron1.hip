// Tacotron (v1) host side: named tensors -> packed device weights (BatchNorm folded at finalize),
// the growing workspace, and tts_tacotron1_{encoder,postnet,infer}. Kernels: tacotron1.hip.
#include "host.h"

#include <cmath>

using namespace ttsh;

namespace {

// W (N x K row-major) -> [K][N]
std::vector<float> transposed(const std::vector<float>& W, int N, int K) {
  std::vector<float> out((size_t)N * K);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) out[(size_t)k * N + n] = W[(size_t)n * K + k];
  return out;
}

void up_linear(const HostMap& m, const std::string& name, int N, int K, DevBuf& w, DevBuf* b) {
  w.upload(transposed(need(m, name + ".weight", {N, K}).d, N, K));
  if (b) b->upload(need(m, name + ".bias", {N}).d);
}

// BatchNormConv1d (layers/tacotron.py:7-66): conv without bias -> BatchNorm(eps 1e-3) -> activation,
// so the norm folds into the conv: W' = W g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps).
// Packed as [K][Cin][Cout].
void up_bnconv(const HostMap& m, const std::string& pfx, int Cin, int Cout, int K, DevBuf& w, DevBuf& b) {
  const auto& W = need(m, pfx + ".conv1d.weight", {Cout, Cin, K}).d;
  const auto& g = need(m, pfx + ".bn.weight", {Cout}).d;
  const auto& be = need(m, pfx + ".bn.bias", {Cout}).d;
  const auto& mu = need(m, pfx + ".bn.running_mean", {Cout}).d;
  const auto& var = need(m, pfx + ".bn.running_var", {Cout}).d;
  std::vector<float> Wp((size_t)K * Cin * Cout), bp(Cout);
  for (int co = 0; co < Cout; ++co) {
    const double sc = (double)g[co] / std::sqrt((double)var[co] + 1e-3);
    bp[co] = (float)((double)be[co] - (double)mu[co] * sc);
    for (int ci = 0; ci < Cin; ++ci)
      for (int k = 0; k < K; ++k)
        Wp[((size_t)k * Cin + ci) * Cout + co] = (float)((double)W[((size_t)co * Cin + ci) * K + k] * sc);
  }
  w.upload(Wp);
  b.upload(bp);
}

void up_cbhg(const HostMap& m, const std::string& pfx, int Cin, int K, int P0, int P1, T1Cbhg& c) {
  c.Cin = Cin, c.K = K, c.P0 = P0, c.P1 = P1;
  c.bank_w.clear();
  c.bank_b.clear();
  c.bank_w.resize(K);
  c.bank_b.resize(K);
  for (int k = 1; k <= K; ++k)
    up_bnconv(m, pfx + ".conv1d_banks." + std::to_string(k - 1), Cin, 128, k, c.bank_w[k - 1], c.bank_b[k - 1]);
  up_bnconv(m, pfx + ".conv1d_projections.0", 128 * K, P0, 3, c.pj1_w, c.pj1_b);
  up_bnconv(m, pfx + ".conv1d_projections.1", P0, P1, 3, c.pj2_w, c.pj2_b);
  TTS_CHECK(P1 == Cin, "CBHG: the last projection must have the input's channels (residual)");
  if (P1 != 128)
    c.pre_hw.upload(transposed(need(m, pfx + ".pre_highway.weight", {128, P1}).d, 128, P1));
  else
    c.pre_hw.reset();
  std::vector<float> hw, hb;
  for (int l = 0; l < 4; ++l)
    for (const char* g : {"H", "T"}) {
      const std::string n = pfx + ".highways." + std::to_string(l) + "." + g;
      const auto t = transposed(need(m, n + ".weight", {128, 128}).d, 128, 128);
      hw.insert(hw.end(), t.begin(), t.end());
      const auto& b = need(m, n + ".bias", {128}).d;
      hb.insert(hb.end(), b.begin(), b.end());
    }
  c.hw_w.upload(hw);
  c.hw_b.upload(hb);
  // input projections of both directions as one [128][768] matrix; W_hh stays row-major per direction
  std::vector<float> wih((size_t)128 * 768), bih, whh, bhh;
  int d = 0;
  for (const char* sfx : {"_l0", "_l0_reverse"}) {
    const auto& w = need(m, pfx + ".gru.weight_ih" + sfx, {384, 128}).d;
    for (int n = 0; n < 384; ++n)
      for (int k = 0; k < 128; ++k) wih[(size_t)k * 768 + d * 384 + n] = w[(size_t)n * 128 + k];
    const auto& bi = need(m, pfx + ".gru.bias_ih" + sfx, {384}).d;
    bih.insert(bih.end(), bi.begin(), bi.end());
    const auto& wh = need(m, pfx + ".gru.weight_hh" + sfx, {384, 128}).d;
    whh.insert(whh.end(), wh.begin(), wh.end());
    const auto& bh = need(m, pfx + ".gru.bias_hh" + sfx, {384}).d;
    bhh.insert(bhh.end(), bh.begin(), bh.end());
    ++d;
  }
  c.gru_wih.upload(wih);
  c.gru_bih.upload(bih);
  c.gru_whh.upload(whh);
  c.gru_bhh.upload(bhh);
}

void up_grucell(const HostMap& m, const std::string& n, int H, int In, DevBuf& ih, DevBuf& hh, DevBuf& bih,
                DevBuf& bhh) {
  ih.upload(transposed(need(m, n + ".weight_ih", {3 * H, In}).d, 3 * H, In));
  hh.upload(transposed(need(m, n + ".weight_hh", {3 * H, H}).d, 3 * H, H));
  bih.upload(need(m, n + ".bias_ih", {3 * H}).d);
  bhh.upload(need(m, n + ".bias_hh", {3 * H}).d);
}

void t1_finalize(tts_ctx* c, int num_chars, int r_init, int memory_size, int attn_norm, int post_dim) {
  T1Model& M = c->t1;
  const HostMap& m = c->t1_host;
  M.ready = false;
  TTS_CHECK(num_chars > 0 && post_dim > 0, "tacotron1: num_chars and postnet_output_dim must be positive");
  TTS_CHECK(r_init >= 1 && r_init <= T1_R_MAX, "tacotron1: r must be in [1, " + std::to_string(T1_R_MAX) + "]");
  TTS_CHECK(memory_size <= T1_MEM_MAX, "tacotron1: memory_size above " + std::to_string(T1_MEM_MAX));
  TTS_CHECK(attn_norm == 0 || attn_norm == 1, "tacotron1: attn_norm must be 0 (sigmoid) or 1 (softmax)");
  M.num_chars = num_chars, M.r_init = r_init, M.mem_frames = memory_size > 0 ? memory_size : 0;
  M.softmax = attn_norm, M.post_dim = post_dim;
  M.emb.upload(need(m, "embedding.weight", {num_chars, 256}).d);
  up_linear(m, "encoder.prenet.linear_layers.0.linear_layer", 256, 256, M.epre1_w, &M.epre1_b);
  up_linear(m, "encoder.prenet.linear_layers.1.linear_layer", 128, 256, M.epre2_w, &M.epre2_b);
  up_cbhg(m, "encoder.cbhg.cbhg", 128, 16, 128, 128, M.enc);
  const std::string d = "decoder.";
  const int memw = 80 * (M.mem_frames > 0 ? M.mem_frames : 1), Y = 80 * r_init;
  up_linear(m, d + "prenet.linear_layers.0.linear_layer", 256, memw, M.pre1, &M.pre1_b);
  up_linear(m, d + "prenet.linear_layers.1.linear_layer", 128, 256, M.pre2, &M.pre2_b);
  up_grucell(m, d + "attention_rnn", 256, 384, M.att_ih, M.att_hh, M.att_bih, M.att_bhh);
  up_linear(m, d + "attention.query_layer.linear_layer", 128, 256, M.wq, nullptr);
  up_linear(m, d + "attention.inputs_layer.linear_layer", 128, 256, M.win, nullptr);
  M.v.upload(need(m, d + "attention.v.linear_layer.weight", {1, 128}).d);
  M.bv = need(m, d + "attention.v.linear_layer.bias", {1}).d[0];
  {  // location_dense . location_conv1d folded: wcomb[ch][tap][dim]
    const auto& wc = need(m, d + "attention.location_layer.location_conv1d.weight", {32, 2, 31}).d;
    const auto& wd = need(m, d + "attention.location_layer.location_dense.linear_layer.weight", {128, 32}).d;
    std::vector<float> comb((size_t)2 * 31 * 128);
    for (int ch = 0; ch < 2; ++ch)
      for (int k = 0; k < 31; ++k)
        for (int dm = 0; dm < 128; ++dm) {
          double s = 0.0;
          for (int f = 0; f < 32; ++f) s += (double)wd[dm * 32 + f] * (double)wc[(f * 2 + ch) * 31 + k];
          comb[((size_t)ch * 31 + k) * 128 + dm] = (float)s;
        }
    M.wcomb.upload(comb);
  }
  up_linear(m, d + "project_to_decoder_in", 256, 512, M.pdi, &M.pdi_b);
  for (int l = 0; l < 2; ++l)
    up_grucell(m, d + "decoder_rnns." + std::to_string(l), 256, 256, M.rnn_ih[l], M.rnn_hh[l], M.rnn_bih[l],
               M.rnn_bhh[l]);
  up_linear(m, d + "proj_to_mel", Y, 256, M.mel, &M.mel_b);
  M.stop_w.upload(need(m, d + "stopnet.linear.weight", {1, 256 + Y}).d);
  M.stop_b = need(m, d + "stopnet.linear.bias", {1}).d[0];
  up_cbhg(m, "postnet.cbhg", 80, 8, 256, 80, M.post);
  up_linear(m, "last_linear", post_dim, 256, M.last_w, &M.last_b);
  M.ready = true;
}

T1Conv conv_of(const float* x, long xb, int ldx, int Cin, const DevBuf& w, const float* bias, int K, int padl,
               int Cout, int act, float* out, long ob, int ldo, int oc0 = 0) {
  return T1Conv{x, xb, ldx, Cin, w.f(), bias, K, padl, Cout, act, nullptr, 0, 0, out, ob, ldo, oc0};
}

// CBHG.forward on x (B, T, Cin) -> out (B, T, 256), rows bounded by the device lengths
void run_cbhg(tts_ctx* c, const T1Cbhg& C, const float* x, long xb, int ldx, const int* lens, int B, int T, float* out,
              long ob) {
  T1WS& W = c->t1ws;
  hipStream_t s = c->s;
  const size_t n = (size_t)B * T;
  const int NB = 128 * C.K;
  W.bank.ensure(n * NB * 4);
  W.p1.ensure(n * C.P0 * 4);
  W.p2.ensure(n * C.P1 * 4);
  W.hw.ensure(n * 128 * 4);
  W.gin.ensure(n * 768 * 4);
  for (int k = 1; k <= C.K; ++k)  // asymmetric zero padding [(k - 1) / 2, k / 2]
    launch_t1_conv(conv_of(x, xb, ldx, C.Cin, C.bank_w[k - 1], C.bank_b[k - 1].f(), k, (k - 1) / 2, 128, 1,
                           W.bank.f(), (long)T * NB, NB, (k - 1) * 128),
                   lens, B, T, s);
  launch_t1_conv(conv_of(W.bank.f(), (long)T * NB, NB, NB, C.pj1_w, C.pj1_b.f(), 3, 1, C.P0, 1, W.p1.f(),
                         (long)T * C.P0, C.P0),
                 lens, B, T, s);
  T1Conv pj2 = conv_of(W.p1.f(), (long)T * C.P0, C.P0, C.P0, C.pj2_w, C.pj2_b.f(), 3, 1, C.P1, 0, W.p2.f(),
                       (long)T * C.P1, C.P1);
  pj2.resid = x, pj2.rb = xb, pj2.ldr = ldx;  // x += inputs
  launch_t1_conv(pj2, lens, B, T, s);
  float* h = W.p2.f();
  if (C.P1 != 128) {  // pre_highway, no bias
    launch_t1_conv(conv_of(W.p2.f(), (long)T * C.P1, C.P1, C.P1, C.pre_hw, nullptr, 1, 0, 128, 0, W.hw.f(),
                           (long)T * 128, 128),
                   lens, B, T, s);
    h = W.hw.f();
  }
  launch_t1_highway(h, (long)T * 128, C.hw_w.f(), C.hw_b.f(), lens, B, T, s);
  launch_t1_conv(conv_of(h, (long)T * 128, 128, 128, C.gru_wih, C.gru_bih.f(), 1, 0, 768, 0, W.gin.f(),
                         (long)T * 768, 768),
                 lens, B, T, s);
  launch_t1_bigru(W.gin.f(), (long)T * 768, C.gru_whh.f(), C.gru_bhh.f(), lens, B, T, out, ob, s);
}

void check_batch(const tts_ctx* c, const int32_t* h_lens, int B, int T_max, const char* what) {
  TTS_CHECK(c->t1.ready, "tacotron1: model not finalized");
  TTS_CHECK(B >= 1 && B <= BMAX, "tacotron1: B must be in [1, " + std::to_string(BMAX) + "]");
  TTS_CHECK(T_max >= 1, std::string("tacotron1: empty ") + what);
  check_rows(h_lens, B, 1, T_max, std::string("tacotron1: ") + what + " length out of range");
}

// embedding -> Prenet(256 -> 256 -> 128, bias, ReLU) -> CBHG into out (B, T, 256); W.lens holds the lengths
void run_encoder(tts_ctx* c, const int64_t* d_ids, int B, int T, float* out) {
  const T1Model& M = c->t1;
  T1WS& W = c->t1ws;
  const size_t n = (size_t)B * T;
  W.x0.ensure(n * 256 * 4);
  W.x1.ensure(n * 256 * 4);
  W.x2.ensure(n * 128 * 4);
  launch_embed_gather(d_ids, T, M.emb.f(), M.num_chars, 256, W.lens.i(), B, W.x0.f(), c->s);
  launch_t1_conv(conv_of(W.x0.f(), (long)T * 256, 256, 256, M.epre1_w, M.epre1_b.f(), 1, 0, 256, 1, W.x1.f(),
                         (long)T * 256, 256),
                 W.lens.i(), B, T, c->s);
  launch_t1_conv(conv_of(W.x1.f(), (long)T * 256, 256, 256, M.epre2_w, M.epre2_b.f(), 1, 0, 128, 1, W.x2.f(),
                         (long)T * 128, 128),
                 W.lens.i(), B, T, c->s);
  run_cbhg(c, M.enc, W.x2.f(), (long)T * 128, 128, W.lens.i(), B, T, out, (long)T * 256);
}

// PostCBHG + last_linear on dec (B, *, 80) with batch stride db, rows bounded by the device lengths
void run_postnet(tts_ctx* c, const float* d_dec, long db, const int* lens, int B, int M_max, float* d_post, long pb) {
  const T1Model& M = c->t1;
  T1WS& W = c->t1ws;
  W.gout.ensure((size_t)B * M_max * 256 * 4);
  run_cbhg(c, M.post, d_dec, db, 80, lens, B, M_max, W.gout.f(), (long)M_max * 256);
  launch_t1_conv(conv_of(W.gout.f(), (long)M_max * 256, 256, 256, M.last_w, M.last_b.f(), 1, 0, M.post_dim, 0, d_post,
                         pb, M.post_dim),
                 lens, B, M_max, c->s);
}

void t1_infer(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T, int r,
              const int32_t* h_max_steps, int S_cap, float* d_dec, float* d_post, float* d_align, float* d_stop,
              int32_t* h_steps, int32_t* h_status) {
  const T1Model& M = c->t1;
  T1WS& W = c->t1ws;
  hipStream_t s = c->s;
  put_rows(W.lens, h_lens, B, s);
  put_rows(W.msteps, h_max_steps, B, s);
  W.ctl.ensure((size_t)3 * B * 4);
  W.enc.ensure((size_t)B * T * 256 * 4);
  W.pin.ensure((size_t)B * T * 128 * 4);
  const size_t Mcap = (size_t)S_cap * r;
  HIP_OK(hipMemsetAsync(d_dec, 0, (size_t)B * Mcap * 80 * 4, s));
  HIP_OK(hipMemsetAsync(d_post, 0, (size_t)B * Mcap * M.post_dim * 4, s));
  HIP_OK(hipMemsetAsync(d_align, 0, (size_t)B * S_cap * T * 4, s));
  HIP_OK(hipMemsetAsync(d_stop, 0, (size_t)B * S_cap * 4, s));
  run_encoder(c, d_ids, B, T, W.enc.f());
  launch_t1_conv(conv_of(W.enc.f(), (long)T * 256, 256, 256, M.win, nullptr, 1, 0, 128, 0, W.pin.f(), (long)T * 128,
                         128),
                 W.lens.i(), B, T, s);
  T1DecArgs a{};
  a.enc = W.enc.f(), a.pin = W.pin.f(), a.lens = W.lens.i(), a.max_steps = W.msteps.i();
  a.T_max = T, a.S_cap = S_cap, a.r = r, a.r_init = M.r_init, a.mem_frames = M.mem_frames, a.softmax = M.softmax;
  a.pre1 = M.pre1.f(), a.pre1_b = M.pre1_b.f(), a.pre2 = M.pre2.f(), a.pre2_b = M.pre2_b.f();
  a.att_ih = M.att_ih.f(), a.att_hh = M.att_hh.f(), a.att_bih = M.att_bih.f(), a.att_bhh = M.att_bhh.f();
  a.wq = M.wq.f(), a.wcomb = M.wcomb.f(), a.v = M.v.f(), a.bv = M.bv;
  a.pdi = M.pdi.f(), a.pdi_b = M.pdi_b.f();
  for (int l = 0; l < 2; ++l)
    a.rnn_ih[l] = M.rnn_ih[l].f(), a.rnn_hh[l] = M.rnn_hh[l].f(), a.rnn_bih[l] = M.rnn_bih[l].f(),
    a.rnn_bhh[l] = M.rnn_bhh[l].f();
  a.mel = M.mel.f(), a.mel_b = M.mel_b.f(), a.stop_w = M.stop_w.f(), a.stop_b = M.stop_b;
  a.dec = d_dec, a.align = d_align, a.stop = d_stop;
  a.steps = W.ctl.i(), a.status = W.ctl.i() + B, a.mlens = W.ctl.i() + 2 * B;
  launch_t1_decoder(a, B, s);
  // the postnet's grid covers the longest decoded row: one host round trip for the step counts
  std::vector<int32_t> ctl((size_t)2 * B);
  HIP_OK(hipMemcpyAsync(ctl.data(), W.ctl.p, (size_t)2 * B * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  int S = 0;
  for (int b = 0; b < B; ++b) {
    h_steps[b] = ctl[b];
    h_status[b] = ctl[B + b];
    TTS_CHECK(ctl[b] >= 1 && ctl[b] <= S_cap && (ctl[B + b] == 1 || ctl[B + b] == 2),
              "tacotron1: the decoder left an invalid step count or status");
    S = std::max(S, (int)ctl[b]);
  }
  run_postnet(c, d_dec, (long)Mcap * 80, W.ctl.i() + 2 * B, B, S * r, d_post, (long)Mcap * M.post_dim);
}

template <class Pre, class F>
int t1_call(tts_ctx* c, void* stream, Pre&& pre, F&& fn) {  // plain fp32 kernels: no range flag to read back
  return guarded_ctx(c, [&] {
    pre();
    DeviceGuard g(c->device);
    enter(c, stream);
    fn();
    leave(c, stream);
  });
}

}  // namespace

extern "C" {

int tts_tacotron1_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::t1_host, name, h, shape, ndim);
}

int tts_tacotron1_finalize(tts_ctx* c, int num_chars, int r_init, int memory_size, int attn_norm,
                           int postnet_output_dim) {
  return guarded_ctx(c, [&] {
    DeviceGuard g(c->device);
    HostMapConsumer consume{c->t1_host};
    t1_finalize(c, num_chars, r_init, memory_size, attn_norm, postnet_output_dim);
  });
}

int tts_tacotron1_encoder(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, float* d_out,
                          void* stream) {
  return t1_call(
      c, stream,
      [&] {
        TTS_CHECK(d_ids && h_lens && d_out, "null argument");
        check_batch(c, h_lens, B, T_max, "text");
      },
      [&] {
        put_rows(c->t1ws.lens, h_lens, B, c->s);
        run_encoder(c, d_ids, B, T_max, d_out);
        HIP_OK(hipStreamSynchronize(c->s));
      });
}

int tts_tacotron1_postnet(tts_ctx* c, const float* d_dec, const int32_t* h_lens, int B, int M_max, float* d_out,
                          void* stream) {
  return t1_call(
      c, stream,
      [&] {
        TTS_CHECK(d_dec && h_lens && d_out, "null argument");
        check_batch(c, h_lens, B, M_max, "mel");
      },
      [&] {
        put_rows(c->t1ws.lens, h_lens, B, c->s);
        run_postnet(c, d_dec, (long)M_max * 80, c->t1ws.lens.i(), B, M_max, d_out, (long)M_max * c->t1.post_dim);
        HIP_OK(hipStreamSynchronize(c->s));
      });
}

int tts_tacotron1_infer(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                        const int32_t* h_max_steps, int S_cap, float* d_dec, float* d_post, float* d_align,
                        float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream) {
  return t1_call(
      c, stream,
      [&] {
        TTS_CHECK(d_ids && h_lens && h_max_steps && d_dec && d_post && d_align && d_stop && h_steps && h_status,
                  "null argument");
        check_batch(c, h_lens, B, T_max, "text");
        TTS_CHECK(T_max <= T1_T_MAX, "tacotron1: more than " + std::to_string(T1_T_MAX) + " input positions");
        TTS_CHECK(r >= 1 && r <= c->t1.r_init, "tacotron1: r must be in [1, r_init]");
        // a row that never stops runs max_decoder_steps + 1 steps
        check_rows(h_max_steps, B, 1, (long)S_cap - 1, "tacotron1: S_cap must be > max_decoder_steps >= 1");
      },
      [&] {
        t1_infer(c, d_ids, h_lens, B, T_max, r, h_max_steps, S_cap, d_dec, d_post, d_align, d_stop, h_steps,
                 h_status);
      });
}

}  // extern "C"
