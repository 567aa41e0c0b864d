// Context life cycle, error text, GEMM mode, and the host helpers every model's file shares
// (host.h): tensor staging, weight layout, conv layer packing and launching, stream ordering.
#include "host.h"
#include "split16.h"
#include "switches.h"

#include <cmath>
#include <cstring>
#include <memory>

static thread_local std::string g_err;
void tts_set_error(const std::string& m) { g_err = m; }

namespace ttsh {

__global__ void put_rows_kernel(int* dst, RowInts r, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = r.v[threadIdx.x];
}

const int* put_rows(int* dst, const int32_t* h, int n, hipStream_t s) {
  for (int o = 0; o < n; o += BMAX) {
    const int m = std::min(BMAX, n - o);
    put_rows_kernel<<<1, BMAX, 0, s>>>(dst + o, row_ints(h + o, m), m);
    HIP_OK(hipGetLastError());
  }
  return dst;
}
const int* put_rows(DevBuf& dst, const int32_t* h, int n, hipStream_t s) {
  ensure<int>(dst, n);
  return put_rows(dst.i(), h, n, s);
}
const int* fill_rows(DevBuf& dst, int value, int n, hipStream_t s) {
  const std::vector<int32_t> h(n, value);
  return put_rows(dst, h.data(), n, s);
}

void check_rows(const int32_t* h, int n, long lo, long hi, const std::string& msg) {
  for (int b = 0; b < n; ++b) TTS_CHECK(h[b] >= lo && h[b] <= hi, msg);
}

void upload_split_rows(DevBuf& d, const std::vector<float>& w, int rows, int K) {
  bool ok = rows % 16 == 0 && K % 32 == 0 && w.size() == (size_t)rows * K;
  for (float v : w) ok &= std::fabs(v) < F16_RANGE;
  if (!ok) {
    d.reset();
    return;
  }
  d.upload(pack_split_a(rows / 16, K / 32, [&](int m, int k) { return w[(size_t)m * K + k]; }));
}

const HostT& need(const HostMap& m, const std::string& k, std::vector<int64_t> shape) {
  auto it = m.find(k);
  TTS_CHECK(it != m.end(), "missing tensor: " + k);
  if (!shape.empty()) {
    bool ok = it->second.shape == shape;
    if (!ok) {
      std::string s = "shape mismatch for " + k + ": got (";
      for (auto x : it->second.shape) s += std::to_string(x) + ",";
      s += ") expected (";
      for (auto x : shape) s += std::to_string(x) + ",";
      throw std::runtime_error(s + ")");
    }
  }
  return it->second;
}

std::vector<float> wn_weight(const HostMap& m, const std::string& name, std::vector<int64_t> shape) {
  auto itw = m.find(name + ".weight");
  if (itw != m.end()) return need(m, name + ".weight", shape).d;
  const auto& v = need(m, name + ".weight_v", shape).d;
  std::vector<int64_t> gshape(shape.size(), 1);
  gshape[0] = shape[0];
  const auto& g = need(m, name + ".weight_g", gshape).d;
  const size_t per = v.size() / shape[0];
  std::vector<float> w(v.size());
  for (int64_t o = 0; o < shape[0]; ++o) {
    double n = 0;
    for (size_t i = 0; i < per; ++i) n += (double)v[o * per + i] * v[o * per + i];
    n = std::sqrt(n);
    const double sc = g[o] / n;
    for (size_t i = 0; i < per; ++i) w[o * per + i] = (float)(v[o * per + i] * sc);
  }
  return w;
}

int stage_tensor(tts_ctx* c, HostMap tts_ctx::*staged, const char* name, const float* h, const int64_t* shape,
                 int ndim) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(name && (h || ndim == 0), "set_tensor: null argument");
    HostT t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      TTS_CHECK(shape[i] >= 0, "negative dim");
      t.shape.push_back(shape[i]);
      n *= (size_t)shape[i];
    }
    t.d.assign(h, h + n);
    (c->*staged)[name] = std::move(t);
  });
}

void pack_conv(ConvLayer& L, const std::vector<float>& Wm, const std::vector<float>& bias, int Cin, int Cout,
               int K, int dil, int nphase, const int* pad_left) {
  TTS_CHECK(Cin % 16 == 0, "conv Cin must be a multiple of 16");
  L.Cin = Cin;
  L.Cout = Cout;
  L.K = K;
  L.dil = dil;
  L.nphase = nphase;
  L.tile = conv_tile_for_cout(Cout);
  if (K == 1 && Cout % 64 == 0 && Cout <= 384) L.tile = TILE_64x64;  // short 1x1 convs: more workgroups
  const int TC = conv_tile_tc(L.tile);
  L.Cout_pad = (Cout + TC - 1) / TC * TC;
  const int Kdim = Cin * K;
  const size_t per = (size_t)L.Cout_pad * Kdim;
  // k order inside each 16-input-channel chunk: tap-major (k' = tap * 16 + ci % 16), so k-chunk
  // `tap` of a staging chunk reads LDS rows ci at column offset tap * dil (no offset table)
  std::vector<float> Wt(Wm.size());
  for (size_t r = 0; r < (size_t)nphase * Cout; ++r)
    for (int ci = 0; ci < Cin; ++ci)
      for (int k = 0; k < K; ++k)
        Wt[r * Kdim + (size_t)(ci / 16) * 16 * K + k * 16 + ci % 16] = Wm[r * Kdim + (size_t)ci * K + k];
  std::vector<float> sw(per * nphase);
  for (int ph = 0; ph < nphase; ++ph)
    swizzle_rows16(Wt.data() + (size_t)ph * Cout * Kdim, Cout, L.Cout_pad, Kdim, sw.data() + ph * per);
  L.phase_stride = (long)per;
  L.W.upload(sw);
  L.bias.upload(bias);
  for (int ph = 0; ph < nphase; ++ph) L.pad_left[ph] = pad_left[ph];
  // split-f16 weights when the shape is covered and every weight is inside the f16 range
  bool in_range = true;
  for (float v : Wm) in_range &= std::fabs(v) < F16_RANGE;
  if (conv_x3_supported(Cin, Cout, K, dil) && in_range) {
    const std::vector<uint16_t> w16 = pack_conv_x3(Wm, Cin, Cout, K, nphase, &L.w16_stride);
    L.W16.ensure(w16.size() * 2);
    HIP_OK(hipMemcpy(L.W16.p, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));
  } else {
    L.W16.reset();
  }
}

void pack_conv_x3_only(ConvLayer& L, const std::vector<float>& Wm, const std::vector<float>& bias, int Cin, int Cout,
                       int K) {
  TTS_CHECK(conv_x3_supported(Cin, Cout, K, 1), "conv_x3: shape not covered");
  L.Cin = Cin;
  L.Cout = L.Cout_pad = Cout;
  L.K = K;
  L.dil = 1;
  L.nphase = 1;
  L.pad_left[0] = (K - 1) / 2 + (K == 2 ? 1 : 0);
  for (float v : Wm) TTS_CHECK(std::fabs(v) < F16_RANGE, "conv_x3: weight outside the f16 range");
  const std::vector<uint16_t> w16 = pack_conv_x3(Wm, Cin, Cout, K, 1, &L.w16_stride);
  L.W16.ensure(w16.size() * 2);
  HIP_OK(hipMemcpy(L.W16.p, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));
  L.bias.upload(bias);
}

void pack_convT(ConvLayer& L, ConvLayer& Lm, const std::vector<float>& wt, const std::vector<float>& bias, int u,
                int Cin, int Cout) {
  TTS_CHECK(u % 2 == 0 && u >= 2 && u <= 8, "upsample factors must be even and <= 8");
  TTS_CHECK(wt.size() == (size_t)Cin * Cout * 2 * u && bias.size() == (size_t)Cout, "ConvTranspose weight / bias size");
  const int p = u / 2;
  std::vector<float> Wm((size_t)u * Cout * Cin * 2);
  int pls[8] = {0};
  for (int ph = 0; ph < u; ++ph) {
    const int dmax = (ph + p) / u, dmin = dmax - 1;
    pls[ph] = -dmin;
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci)
        for (int jj = 0; jj < 2; ++jj) {
          const int delta = dmin + jj;
          const int k = ph + p - delta * u;
          Wm[(((size_t)ph * Cout + co) * Cin + ci) * 2 + jj] = wt[((size_t)ci * Cout + co) * (2 * u) + k];
        }
  }
  pack_conv(L, Wm, bias, Cin, Cout, 2, 1, u, pls);
  bool wm_in_range = true;
  for (float v : Wm) wm_in_range &= std::fabs(v) < F16_RANGE;
  // the merged GEMM has u * Cout rows, so it is covered even where Cout alone is not (full-band 64 -> 32)
  if (wm_in_range && conv_x3_supported(Cin, u * Cout, 2, 1)) {
    std::vector<float> bm((size_t)u * Cout);
    for (size_t r = 0; r < bm.size(); ++r) bm[r] = bias[r / u];
    pack_conv_x3_only(Lm, merge_convT_phases(Wm, u, Cin, Cout), bm, Cin, u * Cout, 2);
  } else {
    Lm.W16.reset();
  }
}

ConvRan run_conv(const ConvLayer& L, const ConvCall& c, hipStream_t st) {
  ConvArgs a{};
  a.src[0] = c.s[0];
  a.src[1] = c.nsrc > 1 ? c.s[1] : c.s[0];
  if (c.nsrc == 1) a.src[0].C = L.Cin;
  a.nsrc = c.nsrc;
  a.Cin = L.Cin;
  a.K = L.K;
  a.dil = L.dil;
  a.pad_mode = c.pad_mode;
  a.lens = c.lens;
  a.len_add = c.len_add;
  a.in_mul = c.in_mul;
  a.q_mul = c.q_mul;
  a.rep_pad = c.rep_pad;
  a.nphase = L.nphase;
  for (int i = 0; i < 8; ++i) a.pad_left[i] = L.pad_left[i];
  a.w_phase_stride = L.phase_stride;
  a.W = L.W.f();
  a.bias = L.bias.f();
  a.Cout = L.Cout;
  a.Cout_pad = L.Cout_pad;
  a.out = c.out;
  a.ob = c.ob;
  a.oc = c.oc;
  a.ot = c.ot;
  a.out_mul = c.out_mul;
  a.epi_act = c.epi;
  a.resid = c.resid;
  a.rb = c.rb;
  a.rc = c.rc;
  a.rt = c.rt;
  a.resid_rows = c.resid_rows;
  a.aux = c.aux;
  a.auxb = c.auxb;
  a.max_q = c.max_q;
  a.B = c.B;
  a.merged_u = c.merged_u;
  TTS_CHECK(!c.merged_u || (c.oflow && L.W16.p), "phase-merged ConvTranspose runs on split-f16 weights only");
  if (c.oflow && L.W16.p && c.nsrc == 1 && (c.s[0].sc != 1 || c.s[0].st % 4 == 0)) {
    a.W16 = L.W16.p;
    a.w16_phase_stride = L.w16_stride;
    a.oflow = c.oflow;
    return {true, launch_conv_x3(a, st)};
  }
  return {false, launch_conv(a, L.tile, st)};
}

void enter(tts_ctx* c, void* stream, bool join_voc) {
  if (c->sv_live && join_voc) {  // a fused submission's vocoder may still use the vocoder workspace
    HIP_OK(hipStreamWaitEvent(c->s, c->ev_sv, 0));
    c->sv_live = false;
  }
  if (hipStreamQuery((hipStream_t)stream) == hipSuccess) return;
  (void)hipGetLastError();  // hipErrorNotReady is not an error here; clear it for later launch checks
  HIP_OK(hipEventRecord(c->ev_in, (hipStream_t)stream));
  HIP_OK(hipStreamWaitEvent(c->s, c->ev_in, 0));
}
void leave(tts_ctx* c, void* stream) {
  HIP_OK(hipEventRecord(c->ev_out, c->s));
  HIP_OK(hipStreamWaitEvent((hipStream_t)stream, c->ev_out, 0));
}

std::vector<float> lstm_tile_rows(const std::vector<float>& W, int H, int K) {
  std::vector<float> out((size_t)4 * H * K);
  for (int t = 0; t < H / 4; ++t)
    for (int g = 0; g < 4; ++g)
      for (int u = 0; u < 4; ++u) {
        const size_t src = (size_t)(g * H + 4 * t + u) * K, dst = (size_t)(t * 16 + g * 4 + u) * K;
        std::memcpy(&out[dst], &W[src], K * sizeof(float));
      }
  return out;
}

std::vector<float> hcat(const std::vector<std::pair<const float*, int>>& parts, int rows) {
  int K = 0;
  for (auto& p : parts) K += p.second;
  std::vector<float> out((size_t)rows * K);
  for (int r = 0; r < rows; ++r) {
    int off = 0;
    for (auto& p : parts) {
      std::memcpy(&out[(size_t)r * K + off], p.first + (size_t)r * p.second, p.second * sizeof(float));
      off += p.second;
    }
  }
  return out;
}

std::vector<float> slice_cols(const std::vector<float>& W, int rows, int K, int c0, int c1) {
  std::vector<float> out((size_t)rows * (c1 - c0));
  for (int r = 0; r < rows; ++r)
    std::memcpy(&out[(size_t)r * (c1 - c0)], &W[(size_t)r * K + c0], (c1 - c0) * sizeof(float));
  return out;
}

std::vector<float> swz(const std::vector<float>& Wm, int rows, int K) {
  const int rp = (rows + 15) / 16 * 16;
  std::vector<float> out((size_t)rp * K);
  swizzle_rows16(Wm.data(), rows, rp, K, out.data());
  return out;
}

void fold_convbn(const HostMap& m, const std::string& pfx, int Cin, int Cout, int K, std::vector<float>& Wm,
                 std::vector<float>& bias) {
  const auto& W = need(m, pfx + ".convolution1d.weight", {Cout, Cin, K}).d;
  const auto& b = need(m, pfx + ".convolution1d.bias", {Cout}).d;
  const auto& g = need(m, pfx + ".batch_normalization.weight", {Cout}).d;
  const auto& be = need(m, pfx + ".batch_normalization.bias", {Cout}).d;
  const auto& mu = need(m, pfx + ".batch_normalization.running_mean", {Cout}).d;
  const auto& var = need(m, pfx + ".batch_normalization.running_var", {Cout}).d;
  Wm.resize((size_t)Cout * Cin * K);
  bias.resize(Cout);
  for (int co = 0; co < Cout; ++co) {
    const double sc = (double)g[co] / std::sqrt((double)var[co] + 1e-5);
    for (int i = 0; i < Cin * K; ++i) Wm[(size_t)co * Cin * K + i] = (float)(W[(size_t)co * Cin * K + i] * sc);
    bias[co] = (float)(((double)b[co] - mu[co]) * sc + be[co]);
  }
}

}  // namespace ttsh

using namespace ttsh;

extern "C" {

int tts_version(void) { return 1; }
const char* tts_last_error(void) { return g_err.c_str(); }

int tts_ctx_create(int device, tts_ctx** out) {
  return guarded([&] {
    TTS_CHECK(out, "null out");
    int n = 0;
    HIP_OK(hipGetDeviceCount(&n));
    TTS_CHECK(device >= 0 && device < n, "invalid device");
    auto c = std::make_unique<tts_ctx>();
    c->device = device;
    c->gemm_x3 = !sw::gemm_f32();
    DeviceGuard g(device);
    HIP_OK(hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking));
    if (!sw::voc_stream()) c->sv = c->s;
    else HIP_OK(hipStreamCreateWithFlags(&c->sv, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&c->ev_sv, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->ev_chunk[0], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->ev_chunk[1], hipEventDisableTiming));
    for (auto& e : c->ev_dec) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventCreateWithFlags(&c->ev_status, hipEventDisableTiming));
    for (auto& t : c->vt) HIP_OK(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&c->pinned), PIN_N * 4, hipHostMallocDefault));
    std::memset(c->pinned, 0, PIN_N * 4);
    *out = c.release();
  });
}

int tts_ctx_destroy(tts_ctx* c) {
  return guarded([&] {
    if (!c) return;
    { std::lock_guard<std::recursive_mutex> lk(c->mu); }  // a call still inside the context ends first
    {
      DeviceGuard g(c->device);
      (void)hipStreamSynchronize(c->sv);
      (void)hipStreamSynchronize(c->s);
      for (auto& ge : c->tws.graphs)
        if (ge) {
          (void)hipGraphExecDestroy(ge);
          ge = nullptr;
        }
    }
    int dev = c->device;
    {
      DeviceGuard g(dev);
      hipStream_t s = c->s, sv = c->sv;
      std::vector<hipEvent_t> e = {c->ev_in, c->ev_out, c->ev_chunk[0], c->ev_chunk[1], c->ev_sv};
      for (auto ev : c->ev_dec) e.push_back(ev);
      e.push_back(c->ev_status);
      for (auto& t : c->vt) e.push_back(t.ev);
      int* pin = c->pinned;
      delete c;
      for (auto ev : e) (void)hipEventDestroy(ev);
      if (sv && sv != s) (void)hipStreamDestroy(sv);
      (void)hipStreamDestroy(s);
      (void)hipHostFree(pin);
    }
  });
}

int tts_set_gemm_mode(tts_ctx* c, int mode) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(mode == 0 || mode == 1, "gemm mode must be 0 (fp32) or 1 (split-f16)");
    c->gemm_x3 = mode == 1;
  });
}

int tts_test_stall_lstm(int recurrence) {
  g_test_stall_lstm.store(recurrence < 0 ? -1 : recurrence);
  return 0;
}

int tts_test_conv(tts_ctx* c, tts_conv_test* d, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(d && d->h_weight && d->h_bias && d->h_lens && d->d_src[0] && d->d_out, "test_conv: null argument");
    TTS_CHECK(d->Cin >= 1 && d->Cout >= 1 && d->B >= 1 && d->max_q >= 0, "test_conv: sizes");
    TTS_CHECK(d->nsrc == 1 || (d->nsrc == 2 && d->d_src[1] && d->src_C[0] + d->src_C[1] == d->Cin), "test_conv: sources");
    TTS_CHECK(d->nphase >= 1 && d->nphase <= 8, "conv: nphase");
    auto lay = [](const int64_t* s) {
      TTS_CHECK(s[1] >= 0 && s[2] >= 0 && s[1] < (1L << 31) && s[2] < (1L << 31), "test_conv: strides");
      return Layout{(long)s[0], (int)s[1], (int)s[2]};
    };
    d->ran_x3 = d->tq = 0;
    d->range_flag = 0;
    DeviceGuard g(c->device);
    enter(c, stream);
    ConvLayer L, Lm;
    const std::vector<float> bias(d->h_bias, d->h_bias + d->Cout);
    if (d->transposed) {
      const int u = d->nphase;
      TTS_CHECK(d->merged_u == 0 || d->merged_u == u, "test_conv: merged_u is 0 or the stride");
      pack_convT(L, Lm, std::vector<float>(d->h_weight, d->h_weight + (size_t)d->Cin * d->Cout * 2 * u), bias, u,
                 d->Cin, d->Cout);
    } else {
      TTS_CHECK(d->K >= 1 && d->dil >= 1 && d->merged_u == 0, "test_conv: taps");
      const size_t n = (size_t)d->nphase * d->Cout * d->Cin * d->K;
      pack_conv(L, std::vector<float>(d->h_weight, d->h_weight + n), bias, d->Cin, d->Cout, d->K, d->dil, d->nphase,
                d->pad_left);
    }
    DevBuf lens;
    ConvCall cc = conv_call(c, put_rows(lens, d->h_lens, d->B, c->s), d->B, d->max_q);
    cc.in(d->d_src[0], lay(d->src_strides[0]), d->nsrc == 2 ? d->src_C[0] : d->Cin, d->src_act[0]);
    if (d->nsrc == 2) {
      cc.in2(d->d_src[1], lay(d->src_strides[1]), d->src_C[1]);
      cc.s[1].act = d->src_act[1];
    }
    cc.to(d->d_out, lay(d->out_strides));
    if (d->d_resid) cc.add(d->d_resid, lay(d->resid_strides));
    cc.resid_rows = d->resid_rows;
    cc.aux = d->d_aux;
    cc.auxb = (long)d->auxb;
    cc.pad_mode = d->pad_mode;
    cc.len_add = d->len_add;
    cc.in_mul = d->in_mul;
    cc.q_mul = d->q_mul;
    cc.out_mul = d->out_mul;
    cc.rep_pad = d->rep_pad;
    cc.epi = d->epi;
    cc.merged_u = d->merged_u;
    if (cc.oflow) HIP_OK(hipMemsetAsync(cc.oflow, 0, 4, c->s));
    // the layers' buffers are freed when this scope ends: wait for the launch first, also on an error
    struct Sync {
      hipStream_t s;
      ~Sync() { (void)hipStreamSynchronize(s); }
    } sync{c->s};
    const ConvRan ran = run_conv(d->merged_u ? Lm : L, cc, c->s);
    d->ran_x3 = ran.x3 ? 1 : 0;
    d->tq = ran.tq;
    if (cc.oflow) HIP_OK(hipMemcpyAsync(&c->pinned[PIN_FLAG], cc.oflow, 4, hipMemcpyDeviceToHost, c->s));
    HIP_OK(hipStreamSynchronize(c->s));
    if (cc.oflow) d->range_flag = (uint32_t)c->pinned[PIN_FLAG];
    leave(c, stream);
  });
}

int tts_gemm_mode(tts_ctx* c, int* mode, int64_t* fallbacks) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(mode && fallbacks, "null argument");
    *mode = c->gemm_x3 ? 1 : 0;
    *fallbacks = c->x3_fallbacks;
  });
}

}  // extern "C"
