// Global Style Tokens on Tacotron2: gst_layer.* folded at load (gst_load), and the style entry
// points: the style encoder over a reference mel (gst.hip) and the weighted sum of style tokens.
#include "host.h"

#include <cmath>

using namespace ttsh;

// Global Style Tokens (gst_layers.py): the reference encoder's convs with their BatchNorm2d (eval,
// eps 1e-5) and bias folded in double, as [kt][kh][ci][co]; the GRU matrices transposed, W_ih's
// columns reordered from the reference's [channel][mel bin] features to the kernels' [mel bin][channel];
// W_query transposed; and the attention's keys and values, which depend on the weights alone:
// K = tanh(tokens) W_key^T, V = tanh(tokens) W_value^T, (ntok, G) each. V's row k is also what a
// {token k: 1} dict yields (one key: the softmax is 1).
void ttsh::gst_load(tts_ctx* c) {
  auto& M = c->taco;
  const auto& h = c->taco_host;
  const std::string P = "gst_layer.";
  const auto& tok = need(h, P + "style_token_layer.style_tokens", {});
  TTS_CHECK(tok.shape.size() == 2, "gst style_tokens must be (tokens, gst_embedding_dim / heads)");
  const int ntok = (int)tok.shape[0], dk = (int)tok.shape[1];
  const auto& wv = need(h, P + "style_token_layer.attention.W_value.weight", {});
  TTS_CHECK(wv.shape.size() == 2 && wv.shape[1] == dk, "gst W_value must be (gst_embedding_dim, key dim)");
  const int G = (int)wv.shape[0], Hg = G / 2;
  TTS_CHECK(G == 128 || G == 256 || G == 512, "gst_embedding_dim must be 128, 256 or 512");
  TTS_CHECK(dk >= 4 && G % dk == 0 && (G / dk == 2 || G / dk == 4 || G / dk == 8), "gst_num_heads must be 2, 4 or 8");
  TTS_CHECK(ntok >= 1 && ntok <= GST_TOK_MAX, "gst_style_tokens must be in [1, 32]");
  TTS_CHECK(M.spk_dim > G, "GST is built for multi-speaker models only (a speaker vector behind the style vector)");
  const auto& wq = need(h, P + "style_token_layer.attention.W_query.weight", {});
  TTS_CHECK(wq.shape.size() == 2 && wq.shape[0] == G && wq.shape[1] >= Hg, "gst W_query must be (G, G / 2 [+ Es])");
  const int Kq = (int)wq.shape[1], Esq = Kq - Hg;
  TTS_CHECK(Esq == 0 || Esq == M.spk_dim - G, "gst W_query: its speaker columns must match the speaker embedding dim");
  TTS_CHECK(Esq % 4 == 0 && Esq <= GST_ES_MAX, "gst W_query: speaker embedding dim must be a multiple of 4, <= 1024");
  const auto& wk = need(h, P + "style_token_layer.attention.W_key.weight", {G, dk}).d;
  const int filt[7] = {1, 32, 32, 64, 64, 128, 128};
  for (int l = 0; l < 6; ++l) {
    const int ci_n = filt[l], co_n = filt[l + 1];
    const std::string cn = P + "encoder.convs." + std::to_string(l), bn = P + "encoder.bns." + std::to_string(l);
    const auto& w = need(h, cn + ".weight", {co_n, ci_n, 3, 3}).d;
    const auto& b = need(h, cn + ".bias", {co_n}).d;
    const auto& g_ = need(h, bn + ".weight", {co_n}).d;
    const auto& be = need(h, bn + ".bias", {co_n}).d;
    const auto& mu = need(h, bn + ".running_mean", {co_n}).d;
    const auto& var = need(h, bn + ".running_var", {co_n}).d;
    std::vector<float> wt((size_t)9 * ci_n * co_n), bt(co_n);
    for (int co = 0; co < co_n; ++co) {
      const double sc = (double)g_[co] / std::sqrt((double)var[co] + 1e-5);
      bt[co] = (float)(((double)b[co] - mu[co]) * sc + be[co]);
      for (int ci = 0; ci < ci_n; ++ci)
        for (int k = 0; k < 9; ++k)
          wt[((size_t)k * ci_n + ci) * co_n + co] = (float)(sc * w[((size_t)co * ci_n + ci) * 9 + k]);
    }
    M.gst_cw[l].upload(wt);
    M.gst_cb[l].upload(bt);
  }
  {
    const std::string rn = P + "encoder.recurrence.";
    const auto& wih = need(h, rn + "weight_ih_l0", {3 * Hg, 256}).d;
    const auto& whh = need(h, rn + "weight_hh_l0", {3 * Hg, Hg}).d;
    std::vector<float> it((size_t)256 * 3 * Hg), ht((size_t)Hg * 3 * Hg);
    for (int g = 0; g < 3 * Hg; ++g) {
      for (int ch = 0; ch < 128; ++ch)
        for (int hb = 0; hb < 2; ++hb) it[(size_t)(hb * 128 + ch) * 3 * Hg + g] = wih[(size_t)g * 256 + ch * 2 + hb];
      for (int k = 0; k < Hg; ++k) ht[(size_t)k * 3 * Hg + g] = whh[(size_t)g * Hg + k];
    }
    M.gst_wihT.upload(it);
    M.gst_whhT.upload(ht);
    M.gst_bih.upload(need(h, rn + "bias_ih_l0", {3 * Hg}).d);
    M.gst_bhh.upload(need(h, rn + "bias_hh_l0", {3 * Hg}).d);
  }
  std::vector<float> qt((size_t)Kq * G), kt((size_t)ntok * G), vt((size_t)ntok * G);
  for (int j = 0; j < G; ++j)
    for (int k = 0; k < Kq; ++k) qt[(size_t)k * G + j] = wq.d[(size_t)j * Kq + k];
  for (int k = 0; k < ntok; ++k)
    for (int j = 0; j < G; ++j) {
      double ak = 0.0, av = 0.0;
      for (int d = 0; d < dk; ++d) {
        const double t = std::tanh((double)tok.d[(size_t)k * dk + d]);
        ak += t * wk[(size_t)j * dk + d];
        av += t * wv.d[(size_t)j * dk + d];
      }
      kt[(size_t)k * G + j] = (float)ak;
      vt[(size_t)k * G + j] = (float)av;
    }
  M.gst_wqT.upload(qt);
  M.gst_K.upload(kt);
  M.gst_V.upload(vt);
  M.gst_dim = G;
  M.gst_heads = G / dk;
  M.gst_ntok = ntok;
  M.gst_es_q = Esq;
}

extern "C" {

int tts_taco_gst_info(tts_ctx* c, int* gst_dim, int* num_tokens, int* query_uses_speaker) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(gst_dim && num_tokens && query_uses_speaker, "null argument");
    TTS_CHECK(c->taco.ready, "tacotron2 weights not finalized");
    *gst_dim = c->taco.gst_dim;
    *num_tokens = c->taco.gst_dim ? c->taco.gst_ntok : 0;
    *query_uses_speaker = c->taco.gst_dim && c->taco.gst_es_q ? 1 : 0;
  });
}

int tts_taco_style_mel(tts_ctx* c, const float* d_mel, const int32_t* h_lens, int B, int N_max, const float* d_spk_emb,
                       float* d_style, void* stream) {
  return guarded_ctx(c, [&] {
    auto& M = c->taco;
    TTS_CHECK(d_mel && h_lens && d_style, "null argument");
    TTS_CHECK(M.ready && M.gst_dim, "the loaded tacotron2 model has no gst_layer");
    TTS_CHECK(B >= 1 && B <= BMAX, "B must be in [1, 64]");
    TTS_CHECK(N_max >= 1 && N_max <= (1 << 16), "N_max must be in [1, 65536]");
    TTS_CHECK(!M.gst_es_q || d_spk_emb, "this model's style query takes the speaker embeddings: pass them");
    check_rows(h_lens, B, 1, N_max, "style mel lens out of range");
    const RowInts lens = row_ints(h_lens, B);
    DeviceGuard g(c->device);
    // layer 1's output (B, W1, 40, 32) and layer 2's (B, W2, 20, 32); the later, smaller layers alternate
    const int W1 = (N_max + 1) / 2, W2 = (W1 + 1) / 2;
    int W6 = W2;
    for (int l = 2; l < 6; ++l) W6 = (W6 + 1) / 2;
    c->gstws.a.ensure((size_t)B * W1 * 40 * 32 * 4);
    c->gstws.b.ensure((size_t)B * W2 * 20 * 32 * 4);
    enter(c, stream);
    const float *cw[6], *cb[6];
    for (int l = 0; l < 6; ++l) cw[l] = M.gst_cw[l].f(), cb[l] = M.gst_cb[l].f();
    launch_gst_convs(d_mel, lens, B, N_max, cw, cb, c->gstws.a.f(), c->gstws.b.f(), c->s);
    GstHeadArgs a{};
    a.x = c->gstws.b.f();
    a.xb = (long)W6 * 256;
    a.lens = lens;
    a.wihT = M.gst_wihT.f(), a.whhT = M.gst_whhT.f(), a.bih = M.gst_bih.f(), a.bhh = M.gst_bhh.f();
    a.wqT = M.gst_wqT.f(), a.Kt = M.gst_K.f(), a.Vt = M.gst_V.f();
    a.spk = M.gst_es_q ? d_spk_emb : nullptr;
    a.Hg = M.gst_dim / 2, a.G = M.gst_dim, a.heads = M.gst_heads, a.ntok = M.gst_ntok, a.Es = M.gst_es_q;
    a.scale = (float)std::sqrt((double)(M.gst_dim / M.gst_heads));
    a.out = d_style;
    launch_gst_head(a, B, c->s);
    leave(c, stream);
  });
}

int tts_taco_style_tokens(tts_ctx* c, const int32_t* h_token_ids, const float* h_weights, int n, float* d_style,
                          void* stream) {
  return guarded_ctx(c, [&] {
    auto& M = c->taco;
    TTS_CHECK(d_style && (n == 0 || (h_token_ids && h_weights)), "null argument");
    TTS_CHECK(M.ready && M.gst_dim, "the loaded tacotron2 model has no gst_layer");
    TTS_CHECK(n >= 0 && n <= GST_DICT_MAX, "at most 64 token weights");
    GstTokenArgs a{};
    a.n = n;
    for (int i = 0; i < n; ++i) {
      TTS_CHECK(h_token_ids[i] >= 0 && h_token_ids[i] < M.gst_ntok, "style token index out of range");
      a.id[i] = h_token_ids[i];
      a.w[i] = h_weights[i];
    }
    DeviceGuard g(c->device);
    enter(c, stream);
    launch_gst_tokens(a, M.gst_V.f(), M.gst_dim, M.gst_ntok, d_style, c->s);
    leave(c, stream);
  });
}

}  // extern "C"
