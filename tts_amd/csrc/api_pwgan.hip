// ParallelWaveGAN: weight packing, the generator, and the tts_pwgan_* entry points.
#include "host.h"
#include "split16.h"
#include "switches.h"

#include <cmath>

using namespace ttsh;

namespace {

void pwgan_finalize(tts_ctx* c, int layers, int stacks, const int32_t* ups, int n_up) {
  auto& P = c->pw;
  const auto& h = c->pw_host;
  P.ready = false;
  TTS_CHECK(layers >= 1 && layers <= 64 && stacks >= 1 && layers % stacks == 0, "pwgan: layers / stacks");
  TTS_CHECK(n_up >= 1 && n_up <= 6, "pwgan: upsample factors");
  const int R = 64, G = 128, A = 80, S = 64, K1 = 3 * R + A;
  P.layers = layers;
  P.stacks = stacks;
  P.ups.assign(ups, ups + n_up);
  P.first_w.upload(wn_weight(h, "first_conv", {R, 1, 1}));
  P.first_b.upload(need(h, "first_conv.bias", {R}).d);
  int p0[8] = {0};
  pack_conv(P.conv_in, wn_weight(h, "upsample_net.conv_in", {A, A, 1}), std::vector<float>(A, 0.f), A, A, 1, 1, 1,
            p0);
  P.up_h.clear();
  P.up_h.resize(n_up);
  for (int i = 0; i < n_up; ++i) {
    TTS_CHECK(ups[i] == 2 || ups[i] == 4 || ups[i] == 8, "pwgan: upsample factors must be 2, 4 or 8");
    P.up_h[i].upload(
        wn_weight(h, "upsample_net.upsample.up_layers." + std::to_string(2 * i + 1), {1, 1, 1, 2 * ups[i] + 1}));
  }
  P.W1.clear();
  P.W1.resize(layers);
  P.b1.clear();
  P.b1.resize(layers);
  P.W2.clear();
  P.W2.resize(layers);
  P.b2.clear();
  P.b2.resize(layers);
  P.W1x.clear();
  P.W1x.resize(layers);
  P.W2x.clear();
  P.W2x.resize(layers);
  for (int l = 0; l < layers; ++l) {
    const std::string q = "conv_layers." + std::to_string(l) + ".";
    const auto wd = wn_weight(h, q + "conv", {G, R, 3});
    const auto& bd = need(h, q + "conv.bias", {G}).d;
    const auto wa = wn_weight(h, q + "conv1x1_aux", {G, A, 1});
    // GEMM1 matrix (128 x 272): row r = gate row (r even: r/2, odd: 64 + r/2); column k = tap*64 + ch
    // for the dilated taps, 192 + ch for the aux features
    std::vector<float> m1((size_t)G * K1), bb1(G);
    for (int r = 0; r < G; ++r) {
      const int src = (r & 1) ? G / 2 + r / 2 : r / 2;
      for (int tap = 0; tap < 3; ++tap)
        for (int ch = 0; ch < R; ++ch) m1[(size_t)r * K1 + tap * R + ch] = wd[((size_t)src * R + ch) * 3 + tap];
      for (int ch = 0; ch < A; ++ch) m1[(size_t)r * K1 + 3 * R + ch] = wa[(size_t)src * A + ch];
      bb1[r] = bd[src];
    }
    std::vector<float> sw1((size_t)G * K1);
    swizzle_rows16(m1.data(), G, G, K1, sw1.data());
    P.W1[l].upload(sw1);
    P.b1[l].upload(bb1);
    const auto wo = wn_weight(h, q + "conv1x1_out", {R, G / 2, 1});
    const auto ws = wn_weight(h, q + "conv1x1_skip", {S, G / 2, 1});
    std::vector<float> m2((size_t)(R + S) * (G / 2)), bb2(R + S);
    std::copy(wo.begin(), wo.end(), m2.begin());
    std::copy(ws.begin(), ws.end(), m2.begin() + (size_t)R * (G / 2));
    const auto& bo = need(h, q + "conv1x1_out.bias", {R}).d;
    const auto& bs = need(h, q + "conv1x1_skip.bias", {S}).d;
    std::copy(bo.begin(), bo.end(), bb2.begin());
    std::copy(bs.begin(), bs.end(), bb2.begin() + R);
    std::vector<float> sw2(m2.size());
    swizzle_rows16(m2.data(), R + S, R + S, G / 2, sw2.data());
    P.W2[l].upload(sw2);
    P.b2[l].upload(bb2);
    bool in_range = true;
    for (float v : m1) in_range &= std::fabs(v) < F16_RANGE;
    for (float v : m2) in_range &= std::fabs(v) < F16_RANGE;
    if (in_range) {
      std::vector<uint16_t> w1x, w2x;
      pack_pw_layer_x3(m1, m2, w1x, w2x);
      P.W1x[l].upload(w1x);
      P.W2x[l].upload(w2x);
    }
  }
  P.W3.upload(wn_weight(h, "last_conv_layers.1", {S, S, 1}));
  P.b3.upload(need(h, "last_conv_layers.1.bias", {S}).d);
  P.w4.upload(wn_weight(h, "last_conv_layers.3", {1, S, 1}));
  P.b4.upload(need(h, "last_conv_layers.3.bias", {1}).d);
  HIP_OK(hipDeviceSynchronize());
  P.ready = true;
}

// ParallelWaveganGenerator.inference (parallel_wavegan_generator.py:120-125) for B mels of
// h_lens[b] frames: replicate pad p, upsample, WaveNet, output (B, 1, hop * (M_max + 2p)),
// row b zero past hop * (h_lens[b] + 2p). d_noise (B, 1, hop * (M_max + 2p)) standard normal.
void pwgan_infer(tts_ctx* c, const float* mel, const int32_t* h_lens, int B, int M_max, int pad, const float* noise,
                 float* out) {
  auto& P = c->pw;
  auto& W = c->pws;
  TTS_CHECK(P.ready, "pwgan weights not finalized");
  TTS_CHECK(B >= 1 && M_max >= 1 && pad >= 0 && pad <= 64, "pwgan: bad sizes");
  check_rows(h_lens, B, 1, M_max, "pwgan: mel lens out of range");
  hipStream_t s = c->s;
  int hop = 1;
  for (int u : P.ups) hop *= u;
  const int Lf = M_max + 2 * pad, Tmax = Lf * hop;
  W.ca.ensure((size_t)B * 80 * Tmax * 4);
  W.cb.ensure((size_t)B * 80 * Tmax * 4);
  W.xa.ensure((size_t)B * 64 * Tmax * 4);
  W.xb.ensure((size_t)B * 64 * Tmax * 4);
  W.skip.ensure((size_t)B * 64 * Tmax * 4);
  const int* dl = put_rows(W.lens, h_lens, B, s);
  // replicate pad + ConvUpsample.conv_in (1x1, frame rate)
  float* cin = W.cb.f();
  float* cout = W.ca.f();
  ConvCall cc = conv_call(c, dl, B, Lf).in(mel, bct(80, M_max), 80).to(cin, bct(80, Lf));
  cc.len_add = 2 * pad;
  cc.pad_mode = 2;
  cc.rep_pad = pad;
  run_conv(P.conv_in, cc, s);
  int L = Lf, mul = 1;
  for (size_t i = 0; i < P.ups.size(); ++i) {
    const int u = P.ups[i];
    launch_pw_upsample(cin, (long)80 * L, L, dl, 2 * pad, mul, u, P.up_h[i].f(), cout, (long)80 * L * u, L * u, 80, B,
                       s);
    std::swap(cin, cout);
    L *= u;
    mul *= u;
  }
  const float* cfeat = cin;  // (B, 80, Tmax)
  float* x = W.xa.f();
  float* xn = W.xb.f();
  launch_pw_first(noise, Tmax, P.first_w.f(), P.first_b.f(), dl, 2 * pad, hop, x, Tmax, B, s);
  if (!W.zeros.p) {
    W.zeros.ensure(256 * 4);
    HIP_OK(hipMemsetAsync(W.zeros.p, 0, 256 * 4, s));
  }
  // residual-block kernel: LDS-DMA ring (default) or register staging (TTS_PWGAN_STAGING=regs)
  const int variant = sw::pwgan_staging();
  const int per_stack = P.layers / P.stacks;
  unsigned* flag = x3_flag(c);
  for (int l = 0; l < P.layers; ++l) {
    if (flag && P.W1x[l].p)
      launch_pw_layer_x3(x, cfeat, xn, W.skip.f(), P.W1x[l].p, P.b1[l].f(), P.W2x[l].p, P.b2[l].f(), dl, h_lens,
                         2 * pad, hop, Tmax, 1 << (l % per_stack), l == 0, B, flag, s);
    else
      launch_pw_layer(x, cfeat, xn, W.skip.f(), P.W1[l].f(), P.b1[l].f(), P.W2[l].f(), P.b2[l].f(), dl, W.zeros.f(),
                      2 * pad, hop, Tmax, 1 << (l % per_stack), l == 0, B, variant, s);
    std::swap(x, xn);
  }
  launch_pw_out(W.skip.f(), std::sqrt(1.0f / P.layers), P.W3.f(), P.b3.f(), P.w4.f(), P.b4.f(), dl, 2 * pad, hop,
                Tmax, out, B, s);
  HIP_OK(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int tts_pwgan_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::pw_host, name, h, shape, ndim);
}

int tts_pwgan_finalize(tts_ctx* c, int num_res_blocks, int stacks, const int32_t* upsample_factors, int n_up) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && upsample_factors, "null argument");
    DeviceGuard g(c->device);
    HostMapConsumer consume{c->pw_host};
    pwgan_finalize(c, num_res_blocks, stacks, upsample_factors, n_up);
  });
}

int tts_pwgan_infer(tts_ctx* c, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                    const float* d_noise, float* d_out, void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_mel && h_lens && d_noise && d_out, "null argument"); },
      [&] { pwgan_infer(c, d_mel, h_lens, B, M_max, pad, d_noise, d_out); });
}

}  // extern "C"
