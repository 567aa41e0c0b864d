// Tacotron2, loading: weight folding and packing (taco_finalize), the workspace, and the
// projection tiles folded per reduction factor (build_pj).
#include "host.h"
#include "decoder.h"
#include "gsync.h"
#include "split16.h"

#include <cmath>
#include <cstring>

using namespace ttsh;

static void taco_finalize(tts_ctx* c, int num_chars, int r_init, int attn_norm) {
  auto& M = c->taco;
  M.graves = c->taco_host.count("decoder.attention.N_a.0.weight") > 0;
  if (M.graves) {
    // Graves attention has no location-sensitive tensors: zero stand-ins keep the shared packing
    // (processed inputs, query projection, location filters, energies) well defined; the Graves
    // variant of the persistent decoder never reads what they produce
    const auto it = c->taco_host.find("decoder.attention_rnn.weight_ih");
    TTS_CHECK(it != c->taco_host.end() && it->second.shape.size() == 2 && it->second.shape[1] > 256,
              "missing tensor: decoder.attention_rnn.weight_ih");
    const int64_t ES = it->second.shape[1] - 256;
    auto zero = [&](const std::string& k, std::vector<int64_t> shape) {
      size_t n = 1;
      for (auto d : shape) n *= (size_t)d;
      c->taco_host[k] = HostT{std::vector<float>(n, 0.f), shape};
    };
    zero("decoder.attention.inputs_layer.linear_layer.weight", {128, ES});
    zero("decoder.attention.query_layer.linear_layer.weight", {128, 1024});
    zero("decoder.attention.location_layer.location_conv1d.weight", {32, 2, 31});
    zero("decoder.attention.location_layer.location_dense.linear_layer.weight", {128, 32});
    zero("decoder.attention.v.linear_layer.weight", {1, 128});
    zero("decoder.attention.v.linear_layer.bias", {1});
  }
  const auto& h = c->taco_host;
  M.ready = false;
  if (M.graves) {
    const auto& w2 = need(h, "decoder.attention.N_a.2.weight", {}).d;
    M.graves_K = (int)(w2.size() / 1024 / 3);
    TTS_CHECK(M.graves_K >= 1 && M.graves_K <= 16 && (size_t)M.graves_K * 3 * 1024 == w2.size(),
              "Graves attention: N_a.2.weight must be (3K, 1024), K <= 16");
    std::vector<float> sw((size_t)1024 * 1024);
    swizzle_rows16(need(h, "decoder.attention.N_a.0.weight", {1024, 1024}).d.data(), 1024, 1024, 1024, sw.data());
    M.na1_w.upload(sw);
    M.na1_b.upload(need(h, "decoder.attention.N_a.0.bias", {1024}).d);
    M.na2_w.upload(w2);
    M.na2_b.upload(need(h, "decoder.attention.N_a.2.bias", {3 * M.graves_K}).d);
  }
  M.num_chars = num_chars;
  M.r_init = r_init;
  M.softmax = attn_norm;
  const int E = 512, H = 256, Q = 1024, D = 1024, P = 256, A = 128, F = 80;
  M.emb.upload(need(h, "embedding.weight", {num_chars, E}).d);
  // decoder_in_features = 512 + speaker dim (models/tacotron2.py:57-58), read off inputs_layer
  {
    auto it = h.find("decoder.attention.inputs_layer.linear_layer.weight");
    TTS_CHECK(it != h.end() && it->second.shape.size() == 2 && it->second.shape[1] >= E,
              "missing tensor: decoder.attention.inputs_layer.linear_layer.weight");
    M.spk_dim = (int)it->second.shape[1] - E;
    TTS_CHECK(M.spk_dim <= 1024, "speaker embedding dim must be <= 1024");
    M.gst_dim = 0;
    if (h.count("gst_layer.style_token_layer.style_tokens")) gst_load(c);  // sets gst_dim
    M.es = M.spk_dim - M.gst_dim;
    auto st = h.find("speaker_embedding.weight");
    M.num_spk = 0;
    if (st != h.end()) {
      TTS_CHECK(st->second.shape.size() == 2 && st->second.shape[1] == M.es,
                "speaker_embedding.weight must be (num_speakers, decoder_in_features - 512 - gst_embedding_dim)");
      M.num_spk = (int)st->second.shape[0];
      M.spk_table.upload(st->second.d);
    }
  }
  const int S = M.spk_dim, ES = E + S;
  int pl2[8] = {2}, pl0[8] = {0};
  for (int i = 0; i < 3; ++i) {
    std::vector<float> Wm, b;
    fold_convbn(h, "encoder.convolutions." + std::to_string(i), E, E, 5, Wm, b);
    pack_conv(M.enc[i], Wm, b, E, E, 5, 1, 1, pl2);
  }
  {  // BiLSTM input projection for both directions as one K=1 conv (Cout 2048), b_ih + b_hh folded
    // gate rows of both the input projection and W_hh in gate-interleaved tile order:
    // column dir*1024 + tile*16 + gate*4 + unit  (unit = 4*tile + u)
    std::vector<float> Wm((size_t)2048 * E), b(2048);
    std::vector<float> whh_all, whh_rows;
    for (int dir = 0; dir < 2; ++dir) {
      const std::string sfx = dir ? "_reverse" : "";
      const auto& wih = need(h, "encoder.lstm.weight_ih_l0" + sfx, {4 * H, E}).d;
      const auto& whh = need(h, "encoder.lstm.weight_hh_l0" + sfx, {4 * H, H}).d;
      const auto& bih = need(h, "encoder.lstm.bias_ih_l0" + sfx, {4 * H}).d;
      const auto& bhh = need(h, "encoder.lstm.bias_hh_l0" + sfx, {4 * H}).d;
      const auto wt = lstm_tile_rows(wih, H, E);
      std::memcpy(&Wm[(size_t)dir * 1024 * E], wt.data(), (size_t)1024 * E * 4);
      std::vector<float> bs(4 * H);
      for (int i = 0; i < 4 * H; ++i) bs[i] = bih[i] + bhh[i];
      const auto bt = lstm_tile_rows(bs, H, 1);
      std::copy(bt.begin(), bt.end(), b.begin() + dir * 1024);
      const auto rows = lstm_tile_rows(whh, H, H);
      const auto hs = swz(rows, 4 * H, H);
      whh_all.insert(whh_all.end(), hs.begin(), hs.end());
      whh_rows.insert(whh_rows.end(), rows.begin(), rows.end());
    }
    pack_conv(M.lstm_in, Wm, b, E, 2048, 1, 1, 1, pl0);
    M.whhT.upload(whh_all);
    upload_split_rows(M.whhT16, whh_rows, 2 * 4 * H, H);
  }
  {  // processed_inputs = inputs_layer(enc)  (common_layers.py:262-263), K=1 conv, no bias
    const auto& win_all = need(h, "decoder.attention.inputs_layer.linear_layer.weight", {A, ES}).d;
    const auto win = slice_cols(win_all, A, ES, 0, E);
    pack_conv(M.penc, win, std::vector<float>(A, 0.f), E, A, 1, 1, 1, pl0);
    M.spk_penc_h = slice_cols(win_all, A, ES, E, ES);
  }
  M.pre1_host = need(h, "decoder.prenet.linear_layers.0.linear_layer.weight", {P, F}).d;
  std::vector<float> w2 = need(h, "decoder.prenet.linear_layers.1.linear_layer.weight", {P, P}).d;
  // BN prenet (LinearBN, common_layers.py:25-46, eval): relu(s (W x - mu) + beta) = relu(W' x + b')
  M.prenet_bn = h.count("decoder.prenet.linear_layers.0.batch_normalization.weight") > 0;
  std::vector<float> b2;
  M.pre1_bias.assign(P, 0.f);
  if (M.prenet_bn) {
    for (int l = 0; l < 2; ++l) {
      const std::string bn = "decoder.prenet.linear_layers." + std::to_string(l) + ".batch_normalization.";
      const auto& g_ = need(h, bn + "weight", {P}).d;
      const auto& b_ = need(h, bn + "bias", {P}).d;
      const auto& mu = need(h, bn + "running_mean", {P}).d;
      const auto& var = need(h, bn + "running_var", {P}).d;
      std::vector<float>& W = l == 0 ? M.pre1_host : w2;
      const int din = l == 0 ? F : P;
      std::vector<float> bias(P);
      for (int o = 0; o < P; ++o) {
        const double sc = (double)g_[o] / std::sqrt((double)var[o] + 1e-5);
        for (int k = 0; k < din; ++k) W[(size_t)o * din + k] = (float)(sc * W[(size_t)o * din + k]);
        bias[o] = (float)((double)b_[o] - sc * mu[o]);
      }
      if (l == 0) M.pre1_bias = bias;
      else b2 = bias;
    }
    M.pre1_b0.upload(M.pre1_bias);
    M.pre2_b.upload(b2);
  }
  M.pre1.upload(swz(M.pre1_host, P, F));
  M.pre2.upload(swz(w2, P, P));
  // transition agent of forward attention (common_layers.py:215-217): ta over [context | query]
  M.trans_agent = h.count("decoder.attention.ta.weight") > 0;
  if (M.trans_agent) {
    M.ta_w.upload(need(h, "decoder.attention.ta.weight", {1, E + S + Q}).d);
    M.ta_b = need(h, "decoder.attention.ta.bias", {1}).d[0];
    TTS_CHECK(S == 0, "transition agent with speaker embeddings is not implemented");
  }
  {
    const auto& wih = need(h, "decoder.attention_rnn.weight_ih", {4 * Q, P + ES}).d;
    const auto& whh = need(h, "decoder.attention_rnn.weight_hh", {4 * Q, Q}).d;
    const auto& bih = need(h, "decoder.attention_rnn.bias_ih", {4 * Q}).d;
    const auto& bhh = need(h, "decoder.attention_rnn.bias_hh", {4 * Q}).d;
    auto wp = slice_cols(wih, 4 * Q, P + ES, 0, P);
    auto wc = slice_cols(wih, 4 * Q, P + ES, P, P + E);
    M.spk_att_h = S ? lstm_tile_rows(slice_cols(wih, 4 * Q, P + ES, P + E, P + ES), Q, S) : std::vector<float>();
    const auto wpt = lstm_tile_rows(wp, Q, P);
    M.att_p.upload(swz(wpt, 4 * Q, P));
    upload_split_rows(M.att_p_x3, wpt, 4 * Q, P);
    auto pre = hcat({{wc.data(), E}, {whh.data(), Q}}, 4 * Q);
    const auto pret = lstm_tile_rows(pre, Q, E + Q);
    M.att_pre.upload(swz(pret, 4 * Q, E + Q));
    upload_split_rows(M.apre_x3, pret, 4 * Q, E + Q);
    std::vector<float> bsum(4 * Q);
    for (int i = 0; i < 4 * Q; ++i) bsum[i] = bih[i] + bhh[i];
    M.att_bias.upload(lstm_tile_rows(bsum, Q, 1));
  }
  {
    const auto& wq = need(h, "decoder.attention.query_layer.linear_layer.weight", {A, Q}).d;
    std::vector<float> t((size_t)Q * A);
    for (int a = 0; a < A; ++a)
      for (int k = 0; k < Q; ++k) t[(size_t)k * A + a] = wq[(size_t)a * Q + k];
    M.WqT.upload(t);
    M.Wloc.upload(need(h, "decoder.attention.location_layer.location_conv1d.weight", {32, 2, 31}).d);
    {
      const auto& wd = need(h, "decoder.attention.location_layer.location_dense.linear_layer.weight", {A, 32}).d;
      std::vector<float> wdT((size_t)32 * A);
      for (int a = 0; a < A; ++a)
        for (int c = 0; c < 32; ++c) wdT[(size_t)c * A + a] = wd[(size_t)a * 32 + c];
      M.Wdense.upload(wdT);
      // location_dense(location_conv(.)) has no biases: one 62-tap filter per attention dim
      const auto& wl = need(h, "decoder.attention.location_layer.location_conv1d.weight", {32, 2, 31}).d;
      std::vector<float> wc((size_t)64 * A, 0.f);
      for (int j = 0; j < 62; ++j)
        for (int a = 0; a < A; ++a) {
          double acc = 0.0;
          for (int cf = 0; cf < 32; ++cf) acc += (double)wd[(size_t)a * 32 + cf] * wl[(size_t)cf * 62 + j];
          wc[(size_t)j * A + a] = (float)acc;
        }
      M.Wcomb.upload(wc);
    }
    M.v.upload(need(h, "decoder.attention.v.linear_layer.weight", {1, A}).d);
    M.bv = need(h, "decoder.attention.v.linear_layer.bias", {1}).d[0];
  }
  {
    const auto& wih_all = need(h, "decoder.decoder_rnn.weight_ih", {4 * D, Q + ES}).d;
    const auto& whh = need(h, "decoder.decoder_rnn.weight_hh", {4 * D, D}).d;
    const auto& bih = need(h, "decoder.decoder_rnn.bias_ih", {4 * D}).d;
    const auto& bhh = need(h, "decoder.decoder_rnn.bias_hh", {4 * D}).d;
    const auto wih = slice_cols(wih_all, 4 * D, Q + ES, 0, Q + E);
    M.spk_dec_h = S ? lstm_tile_rows(slice_cols(wih_all, 4 * D, Q + ES, Q + E, Q + ES), D, S) : std::vector<float>();
    auto w = hcat({{wih.data(), Q + E}, {whh.data(), D}}, 4 * D);
    const auto wt = lstm_tile_rows(w, D, Q + E + D);
    M.dec_w.upload(swz(wt, 4 * D, Q + E + D));
    upload_split_rows(M.dec_x3, wt, 4 * D, Q + E + D);
    std::vector<float> bsum(4 * D);
    for (int i = 0; i < 4 * D; ++i) bsum[i] = bih[i] + bhh[i];
    M.dec_bias.upload(lstm_tile_rows(bsum, D, 1));
  }
  {
    const int NP = F * r_init;
    const auto& wp_all = need(h, "decoder.linear_projection.linear_layer.weight", {NP, D + ES}).d;
    const auto& bp = need(h, "decoder.linear_projection.linear_layer.bias", {NP}).d;
    const auto& ws = need(h, "decoder.stopnet.1.linear_layer.weight", {1, D + NP}).d;
    const auto wp = slice_cols(wp_all, NP, D + ES, 0, D + E);
    // speaker columns of [stop tile | W_p] (stop row = sum_o w_y,o W_p,s[o]), same row order
    M.proj_spk.assign((size_t)(16 + NP) * S, 0.f);
    for (int o = 0; o < NP && S; ++o)
      for (int k = 0; k < S; ++k) {
        const float v = wp_all[(size_t)o * (D + ES) + D + E + k];
        M.proj_spk[(size_t)(16 + o) * S + k] = v;
      }
    for (int k = 0; k < S; ++k) {
      double acc = 0.0;
      for (int o = 0; o < NP; ++o) acc += (double)ws[D + o] * wp_all[(size_t)o * (D + ES) + D + E + k];
      M.proj_spk[k] = (float)acc;
    }

    // stopnet folded through the projection (tacotron2.py:286-295, the stopnet sees all r_init
    // frames): stop = [w_h + W_p,h^T w_y | W_p,ctx^T w_y] . [h | ctx] + (b_s + w_y . b_p)
    std::vector<double> sw(D + E, 0.0);
    for (int k = 0; k < D; ++k) sw[k] = ws[k];
    double sb = need(h, "decoder.stopnet.1.linear_layer.bias", {1}).d[0];
    for (int o = 0; o < NP; ++o) {
      const double wy = ws[D + o];
      for (int k = 0; k < D + E; ++k) sw[k] += wy * wp[(size_t)o * (D + E) + k];
      sb += wy * bp[o];
    }
    // projection weight with the stopnet tile in front: rows [w_stop, 0 x 15, W_p]
    std::vector<float> wx((size_t)(16 + NP) * (D + E), 0.f), bx(16 + NP, 0.f);
    for (int k = 0; k < D + E; ++k) wx[k] = (float)sw[k];
    std::copy(wp.begin(), wp.end(), wx.begin() + (size_t)16 * (D + E));
    bx[0] = (float)sb;
    std::copy(bp.begin(), bp.end(), bx.begin() + 16);
    M.proj_w.upload(swz(wx, 16 + NP, D + E));
    M.proj_b.upload(bx);
    M.proj_rows = std::move(wx);
    M.proj_bias = std::move(bx);
    M.pj_r = -1;
  }
  const int pc[6] = {F, 512, 512, 512, 512, F};
  for (int i = 0; i < 5; ++i) {
    std::vector<float> Wm, b;
    fold_convbn(h, "postnet.convolutions." + std::to_string(i), pc[i], pc[i + 1], 5, Wm, b);
    pack_conv(M.post[i], Wm, b, pc[i], pc[i + 1], 5, 1, 1, pl2);
  }
  HIP_OK(hipDeviceSynchronize());
  M.ready = true;
  c->tws.gen++;  // weights moved: captured graphs are stale
}

void ttsh::taco_workspace(tts_ctx* c, int B, int T_max, int S_cap, int r) {
  auto& W = c->tws;
  const int Bp = 16 * ((B + 15) / 16);
  long& g = W.gen;
  grow<int>(W.lens, BMAX, g);
  grow<int>(W.mlens, BMAX, g);
  grow<float>(W.x0, (size_t)B * T_max * 512, g);
  grow<float>(W.ca, (size_t)B * T_max * 512, g);
  grow<float>(W.cb, (size_t)B * T_max * 512, g);
  grow<float>(W.gin, (size_t)B * T_max * 2048, g);
  grow<float>(W.lh, (size_t)2 * 2 * 64 * 256, g);
  grow<float>(W.lc, (size_t)2 * 64 * 256, g);
  grow<float>(W.enc, (size_t)B * T_max * 512, g);
  grow<float>(W.penc, (size_t)B * T_max * 128, g);
  grow<float>(W.p1, (size_t)Bp * 256, g);
  grow<float>(W.pb, (size_t)2 * 64 * 256, g);  // persistent decoder: two K halves of prenet layer 2
  grow<float>(W.gatt, (size_t)Bp * 4096, g);
  grow<float>(W.hatt, (size_t)Bp * 1024, g);
  grow<float>(W.catt, (size_t)Bp * 1024, g);
  grow<float>(W.hdec0, (size_t)Bp * 1024, g);
  grow<float>(W.hdec1, (size_t)Bp * 1024, g);
  grow<float>(W.cdec, (size_t)Bp * 1024, g);
  grow<float>(W.ctx, (size_t)Bp * 512, g);
  grow<float>(W.y, (size_t)Bp * 80 * c->taco.r_init, g);
  grow<float>(W.pq, (size_t)128 * Bp * 128, g);
  grow<float>(W.spart, (size_t)Bp, g);
  grow<float>(W.alpha, (size_t)B * T_max, g);
  grow<float>(W.acum, (size_t)B * T_max, g);
  grow<float>(W.energy, (size_t)B * T_max, g);
  const int nch = (T_max + 15) / 16;
  grow<float>(W.aps, (size_t)B * nch, g);
  grow<float>(W.apf, (size_t)B * nch, g);
  grow<float>(W.apm, (size_t)B * nch, g);
  grow<float>(W.apu, (size_t)B * nch * 512, g);
  grow<unsigned>(W.acnt, BMAX, g);
  grow<DecCtlBlock>(W.ctl, 1, g);
  grow<float>(W.dec, (size_t)B * S_cap * r * 80, g);
  grow<float>(W.align, (size_t)B * S_cap * T_max, g);
  grow<float>(W.stop, (size_t)B * S_cap, g);
  grow<float>(W.pa, (size_t)B * 512 * S_cap * r, g);
  grow<float>(W.pbb, (size_t)B * 512 * S_cap * r, g);
  grow<float>(W.post, (size_t)B * S_cap * r * 80, g);
  grow<int>(W.map, 2 * BMAX, g);
  grow<int>(W.stat, 256, g);
  grow<float>(W.ypart, (size_t)2 * 64 * (1 + 5 * c->taco.r_init + 16) * 16, g);
  grow<unsigned>(W.pbar, PBAR_CAND * BAR_WORDS, g);  // candidate barrier blocks, one picked per launch (MT = 4 .. 1)
  if (W.pslot_base != W.pbar.p) {  // new candidate blocks: calibrated lazily by the first persistent decode
    for (int i = 0; i < PMAX_LAUNCH; ++i) W.pslot[i] = i;
    W.pslot_base = W.pbar.p;
    W.pslot_cal = false;
  }
  grow<float>(W.anorm, (size_t)2 * BMAX, g);
  grow<float>(W.spk, (size_t)64 * 1024, g);
  grow<int>(W.win_idx, 64, g);
  grow<float>(W.gh, 64 * 1024, g);
  grow<float>(W.gmu, 64 * 16, g);
  grow<float>(W.fwd_u, 64, g);
  grow<int64_t>(W.spkid, 64, g);
  W.B = B;
  W.T_max = T_max;
  W.S_cap = S_cap;
  W.r = r;
  W.MT = Bp / 16;
}

// projection job tiles of the persistent decoder for reduction factor r: the stop tile, the
// 5r tiles of the first r frames, and prenet layer 1 folded through the last frame's rows
// (relu(W1 y_last) = relu(W1 W_p,last [h|ctx] + W1 b_p,last); layer 1 has no bias), fold in double
void ttsh::build_pj(tts_ctx* c, int r) {
  auto& M = c->taco;
  if (M.pj_r == r) return;
  const int K = 1536, F = 80, P = 256;
  const int rows_p = 16 + F * r;
  std::vector<float> rows((size_t)(rows_p + P) * K), bias(rows_p + P);
  std::memcpy(rows.data(), M.proj_rows.data(), (size_t)rows_p * K * sizeof(float));
  std::memcpy(bias.data(), M.proj_bias.data(), (size_t)rows_p * sizeof(float));
  const float* wl = M.proj_rows.data() + (size_t)(16 + F * (r - 1)) * K;  // W_p rows of the last frame
  const float* bl = M.proj_bias.data() + 16 + F * (r - 1);
  std::vector<double> acc(K);
  for (int k = 0; k < P; ++k) {
    std::fill(acc.begin(), acc.end(), 0.0);
    double bs = 0.0;
    for (int i = 0; i < F; ++i) {
      const double w1 = M.pre1_host[(size_t)k * F + i];
      const float* row = wl + (size_t)i * K;
      for (int j = 0; j < K; ++j) acc[j] += w1 * row[j];
      bs += w1 * bl[i];
    }
    float* dst = rows.data() + (size_t)(rows_p + k) * K;
    for (int j = 0; j < K; ++j) dst[j] = (float)acc[j];
    bias[rows_p + k] = (float)(bs + (M.pre1_bias.empty() ? 0.0 : (double)M.pre1_bias[k]));
  }
  M.pj_w.upload(swz(rows, rows_p + P, K));
  upload_split_rows(M.pj_x3, rows, rows_p + P, K);
  M.pj_b.upload(bias);
  if (M.spk_dim) {
    // speaker columns, transposed [Es][att 4096 | dec 4096 | penc 128 | pj rows_p + P]
    const int S = M.spk_dim, N = 4096 + 4096 + 128 + rows_p + P;
    std::vector<float> wt((size_t)S * N);
    auto put = [&](const std::vector<float>& rm, int n0, int nrows) {
      for (int i = 0; i < nrows; ++i)
        for (int e = 0; e < S; ++e) wt[(size_t)e * N + n0 + i] = rm[(size_t)i * S + e];
    };
    put(M.spk_att_h, 0, 4096);
    put(M.spk_dec_h, 4096, 4096);
    put(M.spk_penc_h, 8192, 128);
    put(M.proj_spk, 8320, rows_p);
    const float* sl = M.proj_spk.data() + (size_t)(16 + F * (r - 1)) * S;  // last frame's rows
    for (int k = 0; k < P; ++k)
      for (int e = 0; e < S; ++e) {
        double acc = 0.0;
        for (int i = 0; i < F; ++i) acc += (double)M.pre1_host[(size_t)k * F + i] * sl[(size_t)i * S + e];
        wt[(size_t)e * N + 8320 + rows_p + k] = (float)acc;
      }
    M.spk_wT.upload(wt);
  }
  M.pj_r = r;
}

extern "C" {

int tts_taco_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::taco_host, name, h, shape, ndim);
}

int tts_taco_finalize(tts_ctx* c, int num_chars, int r_init, int attn_norm) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(attn_norm == 0 || attn_norm == 1, "attn_norm must be 0 (sigmoid) or 1 (softmax)");
    TTS_CHECK(r_init >= 1 && r_init <= 16, "r_init out of range");
    DeviceGuard g(c->device);
    HostMapConsumer consume{c->taco_host};  // staged tensors are consumed, even on failure
    taco_finalize(c, num_chars, r_init, attn_norm);
  });
}

int tts_taco_set_options(tts_ctx* c, int windowing, int forward_attn, int forward_attn_mask) {
  return guarded_ctx(c, [&] {
    c->taco.windowing = windowing != 0;
    c->taco.forward_attn = forward_attn != 0;
    c->taco.forward_attn_mask = forward_attn_mask != 0;
  });
}

int tts_taco_speaker_dim(tts_ctx* c, int* spk_dim, int* num_speakers) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && spk_dim && num_speakers, "null argument");
    TTS_CHECK(c->taco.ready, "tacotron2 weights not finalized");
    *spk_dim = c->taco.spk_dim;
    *num_speakers = c->taco.num_spk;
  });
}

}  // extern "C"
