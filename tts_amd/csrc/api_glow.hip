// Glow-TTS: weight packing, encoder + durations, flow decoder, and the tts_glow_* entry points.
#include "host.h"

#include <cmath>
#include <cstdlib>

using namespace ttsh;

namespace {

// rows (r, half + r) -> (2r, 2r + 1) of a (2 * half, rowlen) weight and its bias
std::pair<std::vector<float>, std::vector<float>> interleave_halves(const std::vector<float>& w,
                                                                           const std::vector<float>& b, int half,
                                                                           int rowlen) {
  std::vector<float> wo(w.size()), bo(b.size());
  for (int r = 0; r < 2 * half; ++r) {
    const int src = (r & 1) ? half + r / 2 : r / 2;
    std::copy(w.begin() + (size_t)src * rowlen, w.begin() + (size_t)(src + 1) * rowlen, wo.begin() + (size_t)r * rowlen);
    bo[r] = b[src];
  }
  return {wo, bo};
}

void glow_finalize(tts_ctx* c, int num_chars, int enc_layers, int flows, int wn_layers) {
  auto& G = c->glow;
  const auto& h = c->glow_host;
  G.ready = false;
  const int H = G.H, C = G.C, F = G.Fdp, C2 = 2 * C;
  TTS_CHECK(enc_layers >= 1 && enc_layers <= 32 && flows >= 1 && flows <= 32 && wn_layers >= 1 && wn_layers <= 8,
            "glow: layer counts");
  G.num_chars = num_chars;
  G.enc_layers = enc_layers;
  G.flows = flows;
  G.wn_layers = wn_layers;
  int p2[8] = {2}, p1[8] = {1}, p0[8] = {0};
  {
    auto e = need(h, "encoder.emb.weight", {num_chars, H}).d;
    const float sc = std::sqrt((float)H);  // encoder.py:107, x * math.sqrt(hidden) in fp32
    for (auto& v : e) v *= sc;
    G.emb.upload(e);
  }
  G.enc_conv.clear();
  G.enc_g.clear();
  G.enc_b.clear();
  G.tdsep = h.count("encoder.encoder.layers.0.time_conv.weight") > 0;
  G.tfm = h.count("encoder.encoder.attn_layers.0.conv_q.weight") > 0;
  if (G.tdsep || G.tfm) {
    G.pre_conv.clear();
    G.pre_conv.resize(3);
    G.pre_g.clear();
    G.pre_g.resize(3);
    G.pre_b.clear();
    G.pre_b.resize(3);
    for (int i = 0; i < 3; ++i) {
      const std::string q = "encoder.pre.";
      pack_conv(G.pre_conv[i], need(h, q + "conv_layers." + std::to_string(i) + ".weight", {H, H, 5}).d,
                need(h, q + "conv_layers." + std::to_string(i) + ".bias", {H}).d, H, H, 5, 1, 1, p2);
      G.pre_g[i].upload(need(h, q + "norm_layers." + std::to_string(i) + ".gamma", {1, H, 1}).d);
      G.pre_b[i].upload(need(h, q + "norm_layers." + std::to_string(i) + ".beta", {1, H, 1}).d);
    }
    pack_conv(G.pre_proj, need(h, "encoder.pre.proj.weight", {H, H, 1}).d, need(h, "encoder.pre.proj.bias", {H}).d, H,
              H, 1, 1, 1, p0);
  }
  if (G.tfm) {  // transformer.py:265-319, num_layers = enc_layers
    for (auto* v : {&G.tfm_qkv, &G.tfm_o, &G.tfm_f1, &G.tfm_f2}) {
      v->clear();
      v->resize(enc_layers);
    }
    for (auto* v : {&G.tfm_g1, &G.tfm_b1, &G.tfm_g2, &G.tfm_b2}) {
      v->clear();
      v->resize(enc_layers);
    }
    const int Fc = 768;
    for (int i = 0; i < enc_layers; ++i) {
      const std::string a = "encoder.encoder.attn_layers." + std::to_string(i) + ".";
      std::vector<float> wqkv, bqkv;
      for (const char* n : {"q", "k", "v"}) {
        const auto& w = need(h, a + "conv_" + n + ".weight", {H, H, 1}).d;
        const auto& bb = need(h, a + "conv_" + n + ".bias", {H}).d;
        wqkv.insert(wqkv.end(), w.begin(), w.end());
        bqkv.insert(bqkv.end(), bb.begin(), bb.end());
      }
      pack_conv(G.tfm_qkv[i], wqkv, bqkv, H, 3 * H, 1, 1, 1, p0);
      pack_conv(G.tfm_o[i], need(h, a + "conv_o.weight", {H, H, 1}).d, need(h, a + "conv_o.bias", {H}).d, H, H, 1, 1,
                1, p0);
      const std::string f = "encoder.encoder.ffn_layers." + std::to_string(i) + ".";
      pack_conv(G.tfm_f1[i], need(h, f + "conv_1.weight", {Fc, H, 3}).d, need(h, f + "conv_1.bias", {Fc}).d, H, Fc, 3,
                1, 1, p1);
      pack_conv(G.tfm_f2[i], need(h, f + "conv_2.weight", {H, Fc, 3}).d, need(h, f + "conv_2.bias", {H}).d, Fc, H, 3,
                1, 1, p1);
      const std::string n1 = "encoder.encoder.norm_layers_1." + std::to_string(i) + ".";
      const std::string n2 = "encoder.encoder.norm_layers_2." + std::to_string(i) + ".";
      G.tfm_g1[i].upload(need(h, n1 + "gamma", {1, H, 1}).d);
      G.tfm_b1[i].upload(need(h, n1 + "beta", {1, H, 1}).d);
      G.tfm_g2[i].upload(need(h, n2 + "gamma", {1, H, 1}).d);
      G.tfm_b2[i].upload(need(h, n2 + "beta", {1, H, 1}).d);
    }
  }
  if (G.tdsep) {
    // eval BatchNorm: y = (x - mean) * w / sqrt(var + 1e-5) + b, folded in double
    auto bn_fold = [&](const std::string& name, int n, std::vector<float>& W, std::vector<float>& bias, int rowlen) {
      const auto& w = need(h, name + ".weight", {n}).d;
      const auto& bb = need(h, name + ".bias", {n}).d;
      const auto& mu = need(h, name + ".running_mean", {n}).d;
      const auto& var = need(h, name + ".running_var", {n}).d;
      for (int r = 0; r < n; ++r) {
        const double sc = (double)w[r] / std::sqrt((double)var[r] + 1e-5);
        for (int k = 0; k < rowlen; ++k) W[(size_t)r * rowlen + k] = (float)(W[(size_t)r * rowlen + k] * sc);
        bias[r] = (float)(((double)bias[r] - mu[r]) * sc + bb[r]);
      }
    };
    G.tds_tc.clear();
    G.tds_tc.resize(enc_layers);
    G.tds_tc2.clear();
    G.tds_tc2.resize(enc_layers);
    G.tds_dw.clear();
    G.tds_dw.resize(enc_layers);
    G.tds_dwb.clear();
    G.tds_dwb.resize(enc_layers);
    for (int i = 0; i < enc_layers; ++i) {
      const std::string q = "encoder.encoder.layers." + std::to_string(i) + ".";
      auto w1 = need(h, q + "time_conv.weight", {2 * H, H, 1}).d;
      auto b1 = need(h, q + "time_conv.bias", {2 * H}).d;
      bn_fold(q + "norm1", 2 * H, w1, b1, H);
      auto [w1i, b1i] = interleave_halves(w1, b1, H, H);  // (a_c, g_c) pairs for the GLU epilogue
      pack_conv(G.tds_tc[i], w1i, b1i, H, 2 * H, 1, 1, 1, p0);
      auto wd = need(h, q + "depth_conv.weight", {H, 1, 5}).d;
      auto bd = need(h, q + "depth_conv.bias", {H}).d;
      bn_fold(q + "norm2", H, wd, bd, 5);
      G.tds_dw[i].upload(wd);
      G.tds_dwb[i].upload(bd);
      auto w2 = need(h, q + "time_conv2.weight", {H, H, 1}).d;
      auto b2 = need(h, q + "time_conv2.bias", {H}).d;
      bn_fold(q + "norm3", H, w2, b2, H);
      pack_conv(G.tds_tc2[i], w2, b2, H, H, 1, 1, 1, p0);
    }
  }
  const bool gated = !G.tdsep && !G.tfm;
  G.enc_conv.resize(gated ? enc_layers : 0);
  G.enc_g.resize(gated ? enc_layers : 0);
  G.enc_b.resize(gated ? enc_layers : 0);
  for (int i = 0; i < (gated ? enc_layers : 0); ++i) {
    const std::string pf = "encoder.encoder.";
    pack_conv(G.enc_conv[i], need(h, pf + "conv_layers." + std::to_string(i) + ".weight", {2 * H, H, 5}).d,
              need(h, pf + "conv_layers." + std::to_string(i) + ".bias", {2 * H}).d, H, 2 * H, 5, 1, 1, p2);
    G.enc_g[i].upload(need(h, pf + "norm_layers." + std::to_string(i) + ".gamma", {1, 2 * H, 1}).d);
    G.enc_b[i].upload(need(h, pf + "norm_layers." + std::to_string(i) + ".beta", {1, 2 * H, 1}).d);
  }
  pack_conv(G.proj_m, need(h, "encoder.proj_m.weight", {C, H, 1}).d, need(h, "encoder.proj_m.bias", {C}).d, H, C, 1, 1,
            1, p0);
  const std::string dp = "encoder.duration_predictor.";
  {
    auto it = h.find(dp + "conv_1.weight");
    TTS_CHECK(it != h.end() && it->second.shape.size() == 3, "missing tensor: " + dp + "conv_1.weight");
    G.c_in = (int)it->second.shape[1] - H;
    TTS_CHECK(G.c_in >= 0 && G.c_in <= 4096, "glow: duration predictor input channels");
  }
  const int cin = G.c_in, cpad = (cin + 15) / 16 * 16;
  G.c_pad = cpad;
  {
    // [x; g] input of conv_1, g's channels zero-padded to c_pad
    const auto& w = need(h, dp + "conv_1.weight", {F, H + cin, 3}).d;
    std::vector<float> wp((size_t)F * (H + cpad) * 3, 0.f);
    for (int o = 0; o < F; ++o)
      std::copy(w.begin() + (size_t)o * (H + cin) * 3, w.begin() + (size_t)(o + 1) * (H + cin) * 3,
                wp.begin() + (size_t)o * (H + cpad) * 3);
    pack_conv(G.dp1, wp, need(h, dp + "conv_1.bias", {F}).d, H + cpad, F, 3, 1, 1, p1);
  }
  G.n_spk = 0;
  G.emb_g.reset();
  if (h.count("emb_g.weight")) {
    auto it = h.find("emb_g.weight");
    TTS_CHECK(it->second.shape.size() == 2 && it->second.shape[1] == cin && it->second.shape[0] >= 1,
              "glow: emb_g.weight must be (num_speakers, c_in_channels)");
    G.n_spk = (int)it->second.shape[0];
    if (cin > 0) G.emb_g.upload(it->second.d);
  }
  pack_conv(G.dp2, need(h, dp + "conv_2.weight", {F, F, 3}).d, need(h, dp + "conv_2.bias", {F}).d, F, F, 3, 1, 1, p1);
  pack_conv(G.dp_proj, need(h, dp + "proj.weight", {1, F, 1}).d, need(h, dp + "proj.bias", {1}).d, F, 1, 1, 1, 1, p0);
  G.dp_g1.upload(need(h, dp + "norm_1.gamma", {1, F, 1}).d);
  G.dp_b1.upload(need(h, dp + "norm_1.beta", {1, F, 1}).d);
  G.dp_g2.upload(need(h, dp + "norm_2.gamma", {1, F, 1}).d);
  G.dp_b2.upload(need(h, dp + "norm_2.beta", {1, F, 1}).d);
  G.start.clear();
  G.start.resize(flows);
  G.end.clear();
  G.end.resize(flows);
  G.invtab.clear();
  G.invtab.resize(flows);
  G.fwdtab.clear();
  G.fwdtab.resize(flows);
  G.fwd_logdet_frame = 0.0;
  G.wn_in.clear();
  G.wn_in.resize(flows * wn_layers);
  G.wn_rs.clear();
  G.wn_rs.resize(flows * wn_layers);
  std::vector<float> cond_w(cin > 0 ? (size_t)flows * wn_layers * 2 * H * cpad : 0, 0.f);
  std::vector<float> cond_b(cin > 0 ? (size_t)flows * wn_layers * 2 * H : 0, 0.f);
  for (int k = 0; k < flows; ++k) {
    const std::string an = "decoder.flows." + std::to_string(3 * k) + ".";
    const std::string ic = "decoder.flows." + std::to_string(3 * k + 1) + ".";
    const std::string cp = "decoder.flows." + std::to_string(3 * k + 2) + ".";
    pack_conv(G.start[k], wn_weight(h, cp + "start", {H, C, 1}), need(h, cp + "start.bias", {H}).d, C, H, 1, 1, 1, p0);
    // end rows interleaved (m_c, logs_c) for the conv's coupling-pair epilogue
    auto [we, be] = interleave_halves(need(h, cp + "end.weight", {C2, H, 1}).d, need(h, cp + "end.bias", {C2}).d, C, H);
    pack_conv(G.end[k], we, be, H, C2, 1, 1, 1, p0);
    for (int i = 0; i < wn_layers; ++i) {
      const std::string wi = cp + "wn.in_layers." + std::to_string(i);
      const std::string wr = cp + "wn.res_skip_layers." + std::to_string(i);
      // in rows interleaved (tanh_c, sigmoid_c) for the gate-pair epilogue
      auto [wg, bg] = interleave_halves(wn_weight(h, wi, {2 * H, H, 5}), need(h, wi + ".bias", {2 * H}).d, H, H * 5);
      pack_conv(G.wn_in[k * wn_layers + i], wg, bg, H, 2 * H, 5, 1, 1, p2);
      // rows [0, H): residual, [H, 2H): skip -- one conv into the [hidden | skip] buffer; the last
      // layer has the skip rows only
      const int rsc = i == wn_layers - 1 ? H : 2 * H;
      pack_conv(G.wn_rs[k * wn_layers + i], wn_weight(h, wr, {rsc, H, 1}), need(h, wr + ".bias", {rsc}).d, H, rsc, 1,
                1, 1, p0);
    }
    if (cin > 0) {  // cond_layer (2H * wn_layers, c_in): per layer slice interleaved like wn_in
      const int L2 = 2 * H * wn_layers;
      const auto w = wn_weight(h, cp + "wn.cond_layer", {L2, cin, 1});
      const auto& cb = need(h, cp + "wn.cond_layer.bias", {L2}).d;
      for (int i = 0; i < wn_layers; ++i) {
        std::vector<float> wl(w.begin() + (size_t)i * 2 * H * cin, w.begin() + (size_t)(i + 1) * 2 * H * cin);
        std::vector<float> bl(cb.begin() + (size_t)i * 2 * H, cb.begin() + (size_t)(i + 1) * 2 * H);
        auto [wi, bi] = interleave_halves(wl, bl, H, cin);
        const size_t r0 = ((size_t)k * wn_layers + i) * 2 * H;
        for (int r = 0; r < 2 * H; ++r) {
          std::copy(wi.begin() + (size_t)r * cin, wi.begin() + (size_t)(r + 1) * cin,
                    cond_w.begin() + (r0 + r) * cpad);
          cond_b[r0 + r] = bi[r];
        }
      }
    }
    // reverse of [ActNorm, InvConvNear] (glow.py:48-58, 184-201): output channel c' = i*C + 2j + k
    // (split s' = 2i + k) = (sum_s winv[s'][s] x[c_s] - bias[c']) * exp(-logs[c']), c_s = i_s*C + 2j + k_s
    const auto& w4 = need(h, ic + "weight", {4, 4}).d;
    double a[4][8];
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 8; ++q) a[r][q] = q < 4 ? w4[r * 4 + q] : (q - 4 == r ? 1.0 : 0.0);
    double det = 1.0;  // product of the pivots, sign flipped per row swap
    for (int col = 0; col < 4; ++col) {  // Gauss-Jordan with partial pivoting
      int piv = col;
      for (int r = col + 1; r < 4; ++r)
        if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
      for (int q = 0; q < 8; ++q) std::swap(a[col][q], a[piv][q]);
      TTS_CHECK(std::fabs(a[col][col]) > 1e-12, "glow: singular InvConvNear weight");
      const double d = a[col][col];
      det *= piv == col ? d : -d;
      for (int q = 0; q < 8; ++q) a[col][q] /= d;
      for (int r = 0; r < 4; ++r)
        if (r != col) {
          const double f = a[r][col];
          for (int q = 0; q < 8; ++q) a[r][q] -= f * a[col][q];
        }
    }
    // the reference inverts in fp32 and casts (glow.py:190-193): round the inverse to float
    const auto& logs = need(h, an + "logs", {1, C2, 1}).d;
    const auto& abias = need(h, an + "bias", {1, C2, 1}).d;
    std::vector<float> tab((size_t)C2 * 6);
    for (int cp2 = 0; cp2 < C2; ++cp2) {
      const int s2 = 2 * (cp2 / C) + cp2 % 2;
      for (int s1 = 0; s1 < 4; ++s1) tab[cp2 * 6 + s1] = (float)a[s2][4 + s1];
      tab[cp2 * 6 + 4] = abias[cp2];
      tab[cp2 * 6 + 5] = std::exp(-logs[cp2]);
    }
    G.invtab[k].upload(tab);
    // forward of [ActNorm, InvConvNear] (glow.py:82, 192-203): the weight itself; logdet(W) is NaN
    // for det <= 0, as torch.logdet gives it (glow.py:196)
    std::vector<float> ftab((size_t)C2 * 6);
    double logs_sum = 0.0;
    for (int cp2 = 0; cp2 < C2; ++cp2) {
      const int s2 = 2 * (cp2 / C) + cp2 % 2;
      for (int s1 = 0; s1 < 4; ++s1) ftab[cp2 * 6 + s1] = w4[s2 * 4 + s1];
      ftab[cp2 * 6 + 4] = abias[cp2];
      ftab[cp2 * 6 + 5] = (float)std::exp((double)logs[cp2]);
      logs_sum += (double)logs[cp2];
    }
    G.fwdtab[k].upload(ftab);
    G.fwd_logdet_frame += logs_sum + std::log(det) * (C2 / 4);
  }
  if (cin > 0) pack_conv(G.cond, cond_w, cond_b, cpad, flows * wn_layers * 2 * H, 1, 1, 1, p0);
  HIP_OK(hipDeviceSynchronize());
  G.ready = true;
}

// encoder + duration predictor + durations: h_ylens out (per-utterance frames)
void glow_encode(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, const int32_t* h_spk, int B, int T,
                 float length_scale, int32_t* h_ylens) {
  auto& G = c->glow;
  auto& W = c->glws;
  TTS_CHECK(G.ready, "glow weights not finalized");
  TTS_CHECK(B >= 1 && B <= 64 && T >= 1 && T <= 4096, "glow: bad sizes");
  check_rows(h_lens, B, 1, T, "glow: lens out of range");
  if (h_spk) {
    // the reference looks g up in emb_g (absent unless num_speakers > 1) and feeds it to every WN
    // cond_layer (absent unless c_in_channels > 0): glow_tts.py:160, glow.py:119-120
    TTS_CHECK(G.n_spk > 1, "glow: speaker ids given but the model has no emb_g (num_speakers <= 1)");
    TTS_CHECK(G.c_in > 0, "glow: speaker ids given but the model has no cond_layer (c_in_channels = 0)");
    check_rows(h_spk, B, 0, G.n_spk - 1, "glow: speaker id out of range");
  } else {
    // without g the reference's duration predictor reads x alone (encoder.py:136), which its
    // conv_1 rejects when it was built for hidden + c_in_channels inputs
    TTS_CHECK(G.c_in == 0, "glow: this model's duration predictor expects speaker conditioning (c_in_channels > 0)");
  }
  hipStream_t s = c->s;
  const int H = G.H, C = G.C, F = G.Fdp;
  ensure<int>(W.lens, 64);
  ensure<int>(W.ylens, 64);
  ensure<int>(W.klens, 64);
  ensure<float>(W.xa, (size_t)B * 2 * H * T);
  ensure<float>(W.xb, (size_t)B * H * T);
  ensure<float>(W.h2, (size_t)B * 2 * H * T);
  ensure<float>(W.hdp, (size_t)B * F * T);
  ensure<float>(W.logw, (size_t)B * T);
  ensure<float>(W.cum, (size_t)B * T);
  ensure<float>(W.wceil, (size_t)B * T);
  ensure<float>(W.om, (size_t)B * C * T);
  if (G.tfm) ensure<float>(W.big, (size_t)B * 768 * T);
  W.B = B;
  W.Tx = T;
  W.has_g = h_spk != nullptr;
  W.h_xlens.assign(h_lens, h_lens + B);  // glow_align checks its mel lengths against them
  const int* dl = put_rows(W.lens, h_lens, B, s);
  if (W.has_g) {
    // g, then every WN layer's gate bias cond_layer(g) as one (B, flows * wn_layers * 2H) 1x1 conv
    // over a length-1 sequence
    const int NC = G.flows * G.wn_layers * 2 * H;
    ensure<int>(W.spk, 64);
    ensure<float>(W.g, (size_t)B * G.c_pad);
    ensure<float>(W.gcond, (size_t)B * NC);
    if (!W.ones.p) {
      std::vector<int> one(64, 1);
      W.ones.upload(one);
    }
    launch_glow_speaker(put_rows(W.spk, h_spk, B, s), G.emb_g.f(), G.c_in, G.c_pad, W.g.f(), B, s);
    run_conv(G.cond, conv_call(c, W.ones.i(), B, 1).in(W.g.f(), bct(G.c_pad, 1), G.c_pad).to(W.gcond.f(), bct(NC, 1)), s);
  }
  float* x = W.xa.f();   // (B, H, T) current activations
  float* x2 = W.xb.f();  // ping-pong
  launch_glow_embed(d_ids, T, G.emb.f(), G.num_chars, H, dl, x, B, s);
  auto conv = [&](const ConvLayer& L, const float* in, int cin, float* out, int cout, int epi,
                  const float* resid = nullptr) {
    ConvCall cc = conv_call(c, dl, B, T).in(in, bct(cin, T), cin).to(out, bct(cout, T)).add(resid, bct(cout, T));
    cc.epi = epi;
    run_conv(L, cc, s);
  };
  if (G.tdsep || G.tfm) {
    // ConvLayerNorm prenet (glow.py:43-50): 3 x (conv k5 -> LayerNorm -> ReLU), x + proj(.)
    float* h0 = W.h2.f();
    float* h1 = W.hdp.f();
    conv(G.pre_conv[0], x, H, h0, H, 0);
    launch_ln(h0, (long)H * T, H, G.pre_g[0].f(), G.pre_b[0].f(), dl, B, T, s, true);
    conv(G.pre_conv[1], h0, H, h1, H, 0);
    launch_ln(h1, (long)H * T, H, G.pre_g[1].f(), G.pre_b[1].f(), dl, B, T, s, true);
    conv(G.pre_conv[2], h1, H, h0, H, 0);
    launch_ln(h0, (long)H * T, H, G.pre_g[2].f(), G.pre_b[2].f(), dl, B, T, s, true);
    conv(G.pre_proj, h0, H, x2, H, 0, x);
    std::swap(x, x2);
    // Transformer (transformer.py:307-319): x = LN1(x + o(attn(x))), x = LN2(x + FFN(x))
    for (int i = 0; i < (G.tfm ? G.enc_layers : 0); ++i) {
      float* big = W.big.f();
      conv(G.tfm_qkv[i], x, H, big, 3 * H, 0);
      launch_glow_mha(big, H, H / 96, T, dl, h0, B, s);
      conv(G.tfm_o[i], h0, H, x2, H, 0, x);
      launch_ln(x2, (long)H * T, H, G.tfm_g1[i].f(), G.tfm_b1[i].f(), dl, B, T, s);
      conv(G.tfm_f1[i], x2, H, big, 768, 1);
      conv(G.tfm_f2[i], big, 768, x, H, 0, x2);
      launch_ln(x, (long)H * T, H, G.tfm_g2[i].f(), G.tfm_b2[i].f(), dl, B, T, s);
    }
    // TimeDepthSeparableConvBlock (time_depth_sep_conv.py:51-63, 93-96)
    for (int i = 0; i < (G.tdsep ? G.enc_layers : 0); ++i) {
      conv(G.tds_tc[i], x, H, h0, H, 6);  // time_conv + BN + GLU -> H rows
      launch_tds_depthwise(h0, H, T, G.tds_dw[i].f(), G.tds_dwb[i].f(), dl, h1, B, s);
      conv(G.tds_tc2[i], h1, H, x2, H, 0, x);  // time_conv2 + BN + residual
      std::swap(x, x2);
    }
  }
  for (int i = 0; i < (G.tdsep || G.tfm ? 0 : G.enc_layers); ++i) {  // GatedConvBlock (gated_conv.py:31-42)
    conv(G.enc_conv[i], x, H, W.h2.f(), 2 * H, 0);
    launch_glu_ln_res(W.h2.f(), (long)2 * H * T, 2 * H, G.enc_g[i].f(), G.enc_b[i].f(), x, (long)H * T, x2,
                      (long)H * T, dl, B, T, s);
    std::swap(x, x2);
  }
  conv(G.proj_m, x, H, W.om.f(), C, 0);  // o_mean (encoder.py:125)
  // DurationPredictor (duration_predictor.py:29-40): conv -> relu -> LN, twice, then proj; the
  // input is [x; g] with g constant over time (encoder.py:131-135), masked like x by the conv
  if (G.c_pad > 0) {
    // g: one vector per row, broadcast over time by a time stride of 0
    ConvCall cc = conv_call(c, dl, B, T).in(x, bct(H, T), H).in2(W.g.f(), Layout{G.c_pad, 1, 0}, G.c_pad);
    cc.to(W.hdp.f(), bct(F, T));
    cc.epi = 1;
    // two sources: the fp32 conv, no range flag (conv_x3 stages one source; this k3 conv over
    // ~T x (H + c_pad) inputs is a few microseconds of the call either way)
    cc.oflow = nullptr;
    run_conv(G.dp1, cc, s);
  } else {
    conv(G.dp1, x, H, W.hdp.f(), F, 1);
  }
  launch_ln(W.hdp.f(), (long)F * T, F, G.dp_g1.f(), G.dp_b1.f(), dl, B, T, s);
  conv(G.dp2, W.hdp.f(), F, W.h2.f(), F, 1);
  launch_ln(W.h2.f(), (long)F * T, F, G.dp_g2.f(), G.dp_b2.f(), dl, B, T, s);
  conv(G.dp_proj, W.h2.f(), F, W.logw.f(), 1, 0);
  launch_glow_durations(W.logw.f(), T, dl, length_scale, W.cum.f(), W.ylens.i(), W.wceil.f(), B, s);
  HIP_OK(hipMemcpyAsync(h_ylens, W.ylens.p, B * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  int mx = 1;
  W.h_ylens.assign(h_ylens, h_ylens + B);
  for (int b = 0; b < B; ++b) mx = std::max(mx, (int)h_ylens[b]);
  W.Ty = mx;
}

// One coupling block's network on the squeezed (B, rows, K) activations, shared by both directions
// (glow.py:249-251 up to `end`): start(x0) -> WN (glow.py:118-138) into the skip rows of W.whs, which
// the block's end conv reads next. Every buffer has its own batch stride (in rows).
struct FlowConvs {
  tts_ctx* c;
  const int* kl;  // squeezed lengths (device)
  int B, K;
  void conv(const ConvLayer& L, const float* in, int in_rows, float* out, int out_rows, const float* resid, int epi,
            int resid_rows = 0, const float* aux = nullptr) const {
    const auto& G = c->glow;
    ConvCall cc = conv_call(c, kl, B, K).in(in, bct(in_rows, K), L.Cin).to(out, bct(out_rows, K));
    cc.add(resid, bct(out_rows, K));
    cc.epi = epi;
    cc.resid_rows = resid_rows;
    cc.aux = aux;
    cc.auxb = (long)G.flows * G.wn_layers * 2 * G.H;  // epi 3: gcond's batch stride
    run_conv(L, cc, c->s);
  }
  // returns the skip rows (B, H of 2H, K)
  float* wn(int k, const float* x) const {
    const auto& G = c->glow;
    auto& W = c->glws;
    const int H = G.H;
    float* hid = W.whs.f();  // [hidden | skip] (B, 2H, K)
    float* skip = W.whs.f() + (size_t)H * K;
    conv(G.start[k], x, 2 * G.C, hid, 2 * H, nullptr, 0);
    for (int i = 0; i < G.wn_layers; ++i) {
      const int li = k * G.wn_layers + i;
      // gate fused; with g, cond_layer(g)'s slice for this layer is a per-utterance gate bias
      conv(G.wn_in[li], hid, 2 * H, W.wacts.f(), H, nullptr, 3, 0, W.has_g ? W.gcond.f() + (size_t)li * 2 * H : nullptr);
      // skip rows start at the first layer's output (no accumulate), hidden rows add the residual
      if (i < G.wn_layers - 1) conv(G.wn_rs[li], W.wacts.f(), H, hid, 2 * H, hid, 0, i == 0 ? H : 0);
      else conv(G.wn_rs[li], W.wacts.f(), H, skip, 2 * H, i == 0 ? nullptr : skip, 0);
    }
    return skip;
  }
};

// expand + noise + reverse flows after glow_encode: d_y (B, 80, 2*(Ty/2)), d_ymean (B, 80, Ty),
// d_attn (B, Ty, Tx), d_logw (B, Tx) = o_dur_log; d_noise (B, 80, Ty) standard normal or null
void glow_decode(tts_ctx* c, const float* d_noise, float noise_scale, int Ty, float* d_y, float* d_ymean,
                 float* d_attn, float* d_logw) {
  auto& G = c->glow;
  auto& W = c->glws;
  TTS_CHECK(W.B > 0 && Ty == W.Ty, "glow: decode after encode with Ty = max(y_lengths)");
  hipStream_t s = c->s;
  const int B = W.B, Tx = W.Tx, H = G.H, C = G.C, C2 = 2 * C, K = Ty / 2;
  const int K1 = std::max(K, 1);
  ensure<float>(W.z, (size_t)B * C * Ty);
  ensure<float>(W.sq, (size_t)B * C2 * K1);
  ensure<float>(W.sq2, (size_t)B * C2 * K1);
  ensure<float>(W.whs, (size_t)B * 2 * H * K1);
  ensure<float>(W.wacts, (size_t)B * H * K1);
  launch_glow_expand(W.om.f(), C, Tx, W.lens.i(), W.cum.f(), W.ylens.i(), Ty, d_noise, noise_scale, d_ymean, W.z.f(),
                     d_attn, B, s);
  HIP_OK(hipMemcpyAsync(d_logw, W.logw.p, (size_t)B * Tx * 4, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(d_y, 0, (size_t)B * C * 2 * K * 4, s));
  if (K == 0) return;
  // squeezed lengths floor(y_len / 2) (decoder.py:13-15)
  RowInts hk{};
  for (int b = 0; b < B; ++b) hk.v[b] = W.h_ylens[b] / 2;
  const int* kl = put_rows(W.klens, hk.v, B, s);
  launch_glow_squeeze(W.z.f(), C, Ty, W.ylens.i(), W.sq.f(), K, B, s);
  const FlowConvs fc{c, kl, B, K};
  float* x = W.sq.f();
  float* x2 = W.sq2.f();
  for (int k = G.flows - 1; k >= 0; --k) {
    // CouplingBlock reverse (glow.py:245-262): WN over start(x0), then z1 = (x1 - m) exp(-logs)
    const float* skip = fc.wn(k, x);
    // end conv + coupling + inverse InvConvNear / ActNorm: reads x, writes the next x
    fc.conv(G.end[k], skip, 2 * H, x2, C2, x, 5, 0, G.invtab[k].f());
    std::swap(x, x2);
  }
  launch_glow_unsqueeze(x, C2, K, W.ylens.i(), d_y, 2 * K, B, s);
  HIP_OK(hipStreamSynchronize(s));
}

// the alignment search and what follows it, on W.logp-shaped values: logp (B, Tx, Ty) with the rows'
// lengths on the device (xl, yl) -> W.xof (B, Ty)
void glow_search(tts_ctx* c, const float* d_logp, const int* xl, const int* yl, int max_xlen, int B, int Tx, int Ty) {
  auto& W = c->glws;
  ensure<unsigned long long>(W.masbits, (size_t)B * glow_mas_bits_words(Tx, Ty));
  ensure<int>(W.xof, (size_t)B * Ty);
  launch_glow_mas(d_logp, Tx, Ty, xl, yl, max_xlen, static_cast<unsigned long long*>(W.masbits.p), W.xof.i(), B, c->s);
}

// GlowTts.forward after glow_encode of the same batch (glow_tts.py:131-156): forward flows over the
// mel d_y (B, 80, Ty) -> d_z (B, 80, Te), d_logdet (B); logp (B, Tx, Te) (d_logp or the workspace);
// the monotonic path -> d_attn (B, Te, Tx), d_ymean (B, 80, Te), d_oattn_dur (B, Tx); d_logw (B, Tx).
// Te = 2 floor(Ty / 2), each y_len rounded down to even (preprocess, :187-194).
void glow_align(tts_ctx* c, const float* d_y, const int32_t* h_ylens, int Ty, float* d_z, float* d_logdet,
                float* d_logp, float* d_attn, float* d_ymean, float* d_oattn_dur, float* d_logw) {
  auto& G = c->glow;
  auto& W = c->glws;
  TTS_CHECK(G.ready, "glow weights not finalized");
  TTS_CHECK(W.B > 0, "glow: align after encode of the same batch");
  const int B = W.B, Tx = W.Tx, H = G.H, C = G.C, C2 = 2 * C, K = Ty / 2, Te = 2 * K;
  TTS_CHECK(Ty >= 2, "glow align: the mel needs at least 2 frames");
  RowInts ye2{}, ke{};  // even mel lengths and their halves
  TTS_CHECK((int)W.h_xlens.size() == B, "glow: align after encode of the same batch");
  int max_xlen = 1;
  for (int b = 0; b < B; ++b) {
    TTS_CHECK(h_ylens[b] >= 0 && h_ylens[b] <= Ty, "glow align: y_lengths out of range");
    const int ye = h_ylens[b] / 2 * 2, xl = W.h_xlens[b];
    // below that the reference's search reads outside its band (core.pyx:18-35)
    TTS_CHECK(ye >= 2 && ye >= xl, "glow align: row " + std::to_string(b) + " has " + std::to_string(ye) +
                                       " mel frames (rounded down to even) for " + std::to_string(xl) +
                                       " tokens; the alignment needs at least max(2, tokens)");
    ye2.v[b] = ye;
    ke.v[b] = ye / 2;
    max_xlen = std::max(max_xlen, xl);
  }
  hipStream_t s = c->s;
  const int tiles = (K + 63) / 64;
  ensure<int>(W.aylens, 64);
  ensure<int>(W.aklens, 64);
  ensure<float>(W.sq, (size_t)B * C2 * K);
  ensure<float>(W.sq2, (size_t)B * C2 * K);
  ensure<float>(W.eo, (size_t)B * C2 * K);
  ensure<float>(W.whs, (size_t)B * 2 * H * K);
  ensure<float>(W.wacts, (size_t)B * H * K);
  ensure<double>(W.ldpart, (size_t)G.flows * B * tiles);
  if (!d_logp) {
    ensure<float>(W.logp, (size_t)B * Tx * Te);
    d_logp = W.logp.f();
  }
  const int* yl = put_rows(W.aylens, ye2.v, B, s);
  const int* kl = put_rows(W.aklens, ke.v, B, s);
  launch_glow_squeeze(d_y, C, Ty, yl, W.sq.f(), K, B, s);
  const FlowConvs fc{c, kl, B, K};
  float* x = W.sq.f();
  float* x2 = W.sq2.f();
  // ActNorm + InvConvNear of block 0 on the squeezed mel
  launch_glow_fwd_glue(x, nullptr, G.fwdtab[0].f(), x2, C, K, kl, nullptr, B, s);
  std::swap(x, x2);
  for (int k = 0; k < G.flows; ++k) {
    // CouplingBlock forward (glow.py:247-266): the reverse direction's network, a plain end conv
    // ((m_c, logs_c) row pairs), then the coupling with ActNorm + InvConvNear of block k + 1
    const float* skip = fc.wn(k, x);
    fc.conv(G.end[k], skip, 2 * H, W.eo.f(), C2, nullptr, 0);
    launch_glow_fwd_glue(x, W.eo.f(), k + 1 < G.flows ? G.fwdtab[k + 1].f() : nullptr, x2, C, K, kl,
                         static_cast<double*>(W.ldpart.p) + (size_t)k * B * tiles, B, s);
    std::swap(x, x2);
  }
  launch_glow_unsqueeze(x, C2, K, yl, d_z, Te, B, s);
  launch_glow_logdet(static_cast<const double*>(W.ldpart.p), G.flows, tiles, B, kl, G.fwd_logdet_frame, d_logdet, s);
  launch_glow_logp(W.om.f(), C, Tx, W.lens.i(), d_z, Te, yl, d_logp, B, s);
  glow_search(c, d_logp, W.lens.i(), yl, max_xlen, B, Tx, Te);
  launch_glow_align_out(W.om.f(), C, Tx, W.lens.i(), W.xof.i(), Te, yl, d_ymean, d_attn, d_oattn_dur, B, s);
  HIP_OK(hipMemcpyAsync(d_logw, W.logw.p, (size_t)B * Tx * 4, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
}

// maximum_path (monotonic_align/__init__.py:34-49) alone: d_logp (B, Tx, Ty) -> d_path (B, Tx, Ty)
void glow_mas(tts_ctx* c, const float* d_logp, const int32_t* h_xlens, const int32_t* h_ylens, int B, int Tx, int Ty,
              float* d_path) {
  auto& W = c->glws;
  TTS_CHECK(B >= 1 && B <= 64 && Tx >= 1 && Tx <= 4096 && Ty >= 1, "glow mas: bad sizes");
  int max_xlen = 1;
  for (int b = 0; b < B; ++b) {
    const int xl = h_xlens[b], yl = h_ylens[b];
    TTS_CHECK(xl >= 1 && xl <= Tx && yl >= 1 && yl <= Ty, "glow mas: lengths out of range");
    // below that the reference's search reads outside its band (core.pyx:18-35)
    TTS_CHECK(yl >= xl, "glow mas: row " + std::to_string(b) + " has fewer frames than tokens");
    max_xlen = std::max(max_xlen, xl);
  }
  ensure<int>(W.mxl, 64);
  ensure<int>(W.myl, 64);
  const int* xl = put_rows(W.mxl, h_xlens, B, c->s);
  const int* yl = put_rows(W.myl, h_ylens, B, c->s);
  glow_search(c, d_logp, xl, yl, max_xlen, B, Tx, Ty);
  launch_glow_path(W.xof.i(), Tx, Ty, d_path, B, c->s);
  HIP_OK(hipStreamSynchronize(c->s));
}

}  // namespace

extern "C" {

int tts_glow_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::glow_host, name, h, shape, ndim);
}

int tts_glow_finalize(tts_ctx* c, int num_chars, int enc_layers, int num_flow_blocks, int num_block_layers) {
  return guarded_ctx(c, [&] {
    DeviceGuard g(c->device);
    HostMapConsumer consume{c->glow_host};
    glow_finalize(c, num_chars, enc_layers, num_flow_blocks, num_block_layers);
  });
}

int tts_glow_encode(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, float length_scale,
                    int32_t* h_ylens, void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_ids && h_lens && h_ylens, "null argument"); },
      [&] { glow_encode(c, d_ids, h_lens, nullptr, B, T_max, length_scale, h_ylens); });
}

int tts_glow_encode_spk(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, const int32_t* h_speaker_ids, int B,
                        int T_max, float length_scale, int32_t* h_ylens, void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_ids && h_lens && h_ylens, "null argument"); },
      [&] { glow_encode(c, d_ids, h_lens, h_speaker_ids, B, T_max, length_scale, h_ylens); });
}

int tts_glow_decode(tts_ctx* c, const float* d_noise, float noise_scale, int Ty, float* d_y, float* d_ymean,
                    float* d_attn, float* d_logw, void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_y && d_ymean && d_attn && d_logw, "null argument"); },
      [&] { glow_decode(c, d_noise, noise_scale, Ty, d_y, d_ymean, d_attn, d_logw); });
}

int tts_glow_align(tts_ctx* c, const float* d_y, const int32_t* h_ylens, int Ty, float* d_z, float* d_logdet,
                   float* d_logp, float* d_attn, float* d_ymean, float* d_oattn_dur, float* d_logw, void* stream) {
  return ctx_call(
      c, stream,
      [&] { TTS_CHECK(c && d_y && h_ylens && d_z && d_logdet && d_attn && d_ymean && d_oattn_dur && d_logw, "null argument"); },
      [&] { glow_align(c, d_y, h_ylens, Ty, d_z, d_logdet, d_logp, d_attn, d_ymean, d_oattn_dur, d_logw); });
}

int tts_glow_mas(tts_ctx* c, const float* d_logp, const int32_t* h_xlens, const int32_t* h_ylens, int B, int Tx,
                 int Ty, float* d_path, void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_logp && h_xlens && h_ylens && d_path, "null argument"); },
      [&] { glow_mas(c, d_logp, h_xlens, h_ylens, B, Tx, Ty, d_path); });
}

}  // extern "C"
