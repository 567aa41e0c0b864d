// GE2E speaker encoder: weight packing, the LSTM stack, and the tts_ge2e_* entry points.
#include "host.h"
#include "gsync.h"
#include "split16.h"
#include "switches.h"

#include <cmath>

using namespace ttsh;

namespace {

// (B, T, D) -> (B, T, Dp) with zero channels D..Dp-1 (the conv staging reads 16-channel chunks)
__global__ void pad_channels_kernel(const float* __restrict__ x, int D, int Dp, long n_rows, float* __restrict__ y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows * Dp; i += (long)gridDim.x * blockDim.x) {
    const long r = i / Dp;
    const int c = (int)(i - r * Dp);
    y[i] = c < D ? x[r * D + c] : 0.f;
  }
}

// one workgroup per sequence: v = last frame (with_proj) or relu(W h_last + b), then
// F.normalize(v, p=2, dim=1) = v / max(||v||, 1e-12)  (model.py:58-63)
__global__ __launch_bounds__(256) void ge2e_final_kernel(const float* __restrict__ src, long sb, int width,
                                                         const int* lens, int T_max, const float* __restrict__ W,
                                                         const float* __restrict__ bias, int P,
                                                         float* __restrict__ out) {
  __shared__ float v[1024], red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* last = src + b * sb + (long)(lens[b] - 1) * width;
  for (int i = tid; i < P; i += blockDim.x) {
    float x;
    if (W) {
      float acc = bias[i];
      for (int k = 0; k < width; ++k) acc = fmaf(W[(long)i * width + k], last[k], acc);
      x = fmaxf(acc, 0.f);
    } else {
      x = last[i];
    }
    v[i] = x;
  }
  __syncthreads();
  float ss = 0.f;
  for (int i = tid; i < P; i += blockDim.x) ss = fmaf(v[i], v[i], ss);
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float nrm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
  for (int i = tid; i < P; i += blockDim.x) out[(long)b * P + i] = v[i] / nrm;
}

void ge2e_finalize(tts_ctx* c, int in_dim, int proj, int lstm, int nl, int with_proj) {
  auto& G = c->ge2e;
  const auto& h = c->ge2e_host;
  G.ready = false;
  TTS_CHECK(lstm == 768, "speaker encoder: lstm_dim must be 768 (the persistent LSTM kernel's width)");
  TTS_CHECK(nl >= 1 && nl <= 4 && in_dim >= 1 && in_dim <= 1024 && proj >= 1 && proj <= 1024, "speaker encoder sizes");
  G.in_dim = in_dim;
  G.in_pad = (in_dim + 15) / 16 * 16;
  G.proj = proj;
  G.H = lstm;
  G.nl = nl;
  G.with_proj = with_proj;
  const int H = lstm;
  int pl0[8] = {0};
  for (int l = 0; l < nl; ++l) {
    const std::string pfx = with_proj ? "layers." + std::to_string(l) + ".lstm." : "layers.lstm.";
    const std::string sfx = with_proj ? "_l0" : "_l" + std::to_string(l);
    const int din = l == 0 ? in_dim : (with_proj ? proj : H);
    const int dpad = l == 0 ? G.in_pad : din;
    TTS_CHECK(dpad % 16 == 0, "speaker encoder: layer input width must be a multiple of 16");
    const auto& wih = need(h, pfx + "weight_ih" + sfx, {4 * H, din}).d;
    const auto& whh = need(h, pfx + "weight_hh" + sfx, {4 * H, H}).d;
    const auto& bih = need(h, pfx + "bias_ih" + sfx, {4 * H}).d;
    const auto& bhh = need(h, pfx + "bias_hh" + sfx, {4 * H}).d;
    std::vector<float> wt = lstm_tile_rows(wih, H, din), w2((size_t)4 * H * dpad, 0.f);
    for (int r = 0; r < 4 * H; ++r)
      for (int k = 0; k < din; ++k) w2[(size_t)r * dpad + k] = wt[(size_t)r * din + k];
    std::vector<float> bs(4 * H);
    for (int i = 0; i < 4 * H; ++i) bs[i] = bih[i] + bhh[i];
    pack_conv(G.gin[l], w2, lstm_tile_rows(bs, H, 1), dpad, 4 * H, 1, 1, 1, pl0);
    G.whh[l].upload(swz(lstm_tile_rows(whh, H, H), 4 * H, H));
    upload_split_rows(G.whh16[l], lstm_tile_rows(whh, H, H), 4 * H, H);
    if (with_proj) {
      const auto& wl = need(h, "layers." + std::to_string(l) + ".linear.weight", {proj, H}).d;
      pack_conv(G.proj_l[l], wl, std::vector<float>(proj, 0.f), H, proj, 1, 1, 1, pl0);
    }
  }
  if (!with_proj) {
    G.lin_w.upload(need(h, "layers.linear.weight", {proj, H}).d);
    G.lin_b.upload(need(h, "layers.linear.bias", {proj}).d);
  }
  G.pipe_ok = G.whh16[0].p != nullptr;
  for (int l = 1; l < nl && G.pipe_ok; ++l) {
    const std::string pfx = with_proj ? "layers." + std::to_string(l) + ".lstm." : "layers.lstm.";
    const std::string sfx = with_proj ? "_l0" : "_l" + std::to_string(l);
    const int din = with_proj ? proj : H;
    const auto& wih = need(h, pfx + "weight_ih" + sfx, {4 * H, din}).d;
    const auto& whh = need(h, pfx + "weight_hh" + sfx, {4 * H, H}).d;
    const auto& bih = need(h, pfx + "bias_ih" + sfx, {4 * H}).d;
    const auto& bhh = need(h, pfx + "bias_hh" + sfx, {4 * H}).d;
    std::vector<float> win;
    if (with_proj) {  // the previous layer's Linear (no bias, model.py:22) folded into W_ih
      const auto& wl = need(h, "layers." + std::to_string(l - 1) + ".linear.weight", {proj, H}).d;
      win.assign((size_t)4 * H * H, 0.f);
      std::vector<double> acc(H);
      for (int r = 0; r < 4 * H; ++r) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int j = 0; j < proj; ++j) {
          const double a = wih[(size_t)r * proj + j];
          const float* wr = &wl[(size_t)j * H];
          for (int k = 0; k < H; ++k) acc[k] += a * wr[k];
        }
        for (int k = 0; k < H; ++k) win[(size_t)r * H + k] = (float)acc[k];
      }
    } else {
      win = wih;
    }
    const auto t1 = lstm_tile_rows(whh, H, H), t2 = lstm_tile_rows(win, H, H);
    std::vector<float> wc((size_t)4 * H * 2 * H);
    for (int r = 0; r < 4 * H; ++r) {
      std::memcpy(&wc[(size_t)r * 2 * H], &t1[(size_t)r * H], H * 4);
      std::memcpy(&wc[(size_t)r * 2 * H + H], &t2[(size_t)r * H], H * 4);
    }
    upload_split_rows(G.wpipe[l], wc, 4 * H, 2 * H);
    std::vector<float> bs(4 * H);
    for (int i = 0; i < 4 * H; ++i) bs[i] = bih[i] + bhh[i];
    G.bpipe[l].upload(lstm_tile_rows(bs, H, 1));
    G.pipe_ok = G.wpipe[l].p != nullptr;
  }
  HIP_OK(hipDeviceSynchronize());
  G.ready = true;
}

void ge2e_infer(tts_ctx* c, const float* d_x, const int32_t* h_lens, int B, int T_max, float* d_out) {
  auto& G = c->ge2e;
  auto& W = c->gws;
  TTS_CHECK(G.ready, "speaker encoder weights not finalized");
  TTS_CHECK(B >= 1 && B <= 64, "speaker encoder: B must be in [1, 64]");
  TTS_CHECK(T_max >= 1 && T_max <= 100000, "speaker encoder: bad T_max");
  check_rows(h_lens, B, 1, T_max, "speaker encoder: lens out of range");
  hipStream_t s = c->s;
  const int H = G.H;
  ensure<float>(W.x, (size_t)B * T_max * G.in_pad);
  ensure<int>(W.lens, 64);
  ensure<float>(W.g, (size_t)B * T_max * 4 * H);
  ensure<float>(W.o, (size_t)B * T_max * H);
  ensure<float>(W.p, (size_t)B * T_max * G.proj);
  ensure<unsigned>(W.bar, BAR_WORDS);
  ensure<float>(W.hbuf, (size_t)2 * 64 * H);
  const int* dl = put_rows(W.lens, h_lens, B, s);
  pad_channels_kernel<<<1024, 256, 0, s>>>(d_x, G.in_dim, G.in_pad, (long)B * T_max, W.x.f());
  HIP_OK(hipGetLastError());
  const float* in = W.x.f();
  int din = G.in_pad;
  // gates_in = x W_ih^T + b of layer l (time-major rows, K = 1), and the layer's Linear
  auto gates = [&](int l) {
    run_conv(G.gin[l], conv_call(c, dl, B, T_max).in(in, btc(T_max, din), din).to(W.g.f(), btc(T_max, 4 * H)), s);
  };
  auto project = [&](int l) {
    run_conv(G.proj_l[l], conv_call(c, dl, B, T_max).in(W.o.f(), btc(T_max, H), H).to(W.p.f(), btc(T_max, G.proj)), s);
  };
  // all layers in one persistent launch (encoder.hip ge2e_pipe_kernel); TTS_GE2E_PIPE=0 keeps
  // one launch per layer with the input projections as convs
  const bool pipe_env = sw::ge2e_pipe();
  bool piped = false;
  if (pipe_env && c->gemm_x3 && G.pipe_ok && B <= 16) {
    gates(0);
    const uint16_t* w16[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* bias[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < G.nl; ++l) {
      w16[l] = l == 0 ? G.whh16[0].h() : G.wpipe[l].h();
      bias[l] = l == 0 ? nullptr : G.bpipe[l].f();
    }
    piped = launch_ge2e_pipe(w16, bias, G.nl, W.g.f(), dl, T_max, B, W.hbuf.f(), reinterpret_cast<unsigned*>(W.bar.p),
                             W.o.f(), s);
    if (piped && G.with_proj) project(G.nl - 1);  // the last layer's Linear
  }
  for (int l = 0; l < G.nl && !piped; ++l) {
    gates(l);
    const bool ok = launch_lstm768_persist(W.g.f(), G.whh[l].f(), c->gemm_x3 ? G.whh16[l].h() : nullptr, dl, T_max, B,
                                           W.hbuf.f(), reinterpret_cast<unsigned*>(W.bar.p), W.o.f(), s);
    TTS_CHECK(ok, "speaker encoder: cooperative launch unavailable");
    if (G.with_proj) {
      project(l);
      in = W.p.f();
      din = G.proj;
    } else {
      in = W.o.f();
      din = H;
    }
  }
  if (G.with_proj)
    ge2e_final_kernel<<<B, 256, 0, s>>>(W.p.f(), (long)T_max * G.proj, G.proj, dl, T_max, nullptr, nullptr,
                                        G.proj, d_out);
  else
    ge2e_final_kernel<<<B, 256, 0, s>>>(W.o.f(), (long)T_max * H, H, dl, T_max, G.lin_w.f(), G.lin_b.f(),
                                        G.proj, d_out);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  unsigned err = 0;
  HIP_OK(hipMemcpy(&err, reinterpret_cast<unsigned*>(W.bar.p) + 16, 4, hipMemcpyDeviceToHost));
  TTS_CHECK(err == 0, "speaker encoder: grid barrier timed out (workgroups not co-resident) or preempted past TTS_BARRIER_TIMEOUT_MS; retrying the call is safe)");
}

}  // namespace

extern "C" {

int tts_ge2e_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::ge2e_host, name, h, shape, ndim);
}

int tts_ge2e_finalize(tts_ctx* c, int input_dim, int proj_dim, int lstm_dim, int num_lstm_layers,
                      int use_lstm_with_projection) {
  return guarded_ctx(c, [&] {
    DeviceGuard g(c->device);
    HostMapConsumer consume{c->ge2e_host};
    ge2e_finalize(c, input_dim, proj_dim, lstm_dim, num_lstm_layers, use_lstm_with_projection);
  });
}

int tts_ge2e_infer(tts_ctx* c, const float* d_x, const int32_t* h_lens, int B, int T_max, float* d_out,
                   void* stream) {
  return ctx_call(
      c, stream, [&] { TTS_CHECK(c && d_x && h_lens && d_out, "null argument"); },
      [&] { ge2e_infer(c, d_x, h_lens, B, T_max, d_out); });
}

}  // extern "C"
