// MelGAN / MB-MelGAN: weight packing, the generator, output conv + PQMF synthesis, and the
// tts_melgan_* entry points.
#include "host.h"
#include "split16.h"
#include "switches.h"

#include <cmath>
#include <cstring>

using namespace ttsh;

namespace {

// One ResidualStack block's device weights from its three convs (shared by melgan_finalize and
// tts_test_voc): the dilated conv, [W_1x1 | W_sc] with b_1x1 + b_sc as one 1x1 conv over [lrelu(h); x],
// and where the channel count is covered the split-f16 fragments of both (resblock_x3.hip; phase 1
// also in resstack_x3's packed order when C % 32 == 16)
struct ResBlockPack {
  ConvLayer &dconv, &fused;
  DevBuf &wd16, &wf16, &wd16p;
};
void pack_res_block(const ResBlockPack& P, const std::vector<float>& wd, const std::vector<float>& bd,
                    const std::vector<float>& w1, const std::vector<float>& b1, const std::vector<float>& ws,
                    const std::vector<float>& bs, int C, int dil) {
  int pld[8] = {dil}, pl0[8] = {0};
  pack_conv(P.dconv, wd, bd, C, C, 3, dil, 1, pld);
  std::vector<float> Wf((size_t)C * 2 * C), bf(C);
  for (int co = 0; co < C; ++co) {
    std::memcpy(&Wf[(size_t)co * 2 * C], &w1[(size_t)co * C], C * 4);
    std::memcpy(&Wf[(size_t)co * 2 * C + C], &ws[(size_t)co * C], C * 4);
    bf[co] = b1[co] + bs[co];
  }
  pack_conv(P.fused, Wf, bf, 2 * C, C, 1, 1, 1, pl0);
  if (resblock_x3_supported(C)) {
    std::vector<uint16_t> wd16, wf16;
    pack_resblock_x3(wd, Wf, C, wd16, wf16);
    P.wd16.upload(wd16);
    P.wf16.upload(wf16);
    if (C % 32 == 16) {
      pack_resblock_x3p(wd, C, wd16);
      P.wd16p.upload(wd16);
    }
  }
}

// The output conv's weight (out_ch, C, 7) for the VALU output kernels (melgan_out.hip): [c][k][o]
// for the fused output + PQMF kernel (out_ch = 4), [c][k] as it is for the full-band one (out_ch = 1)
void pack_out_conv(DevBuf& out_w, DevBuf& out_b, const std::vector<float>& w, const std::vector<float>& bo, int C,
                   int out_ch) {
  if (out_ch == 4) {
    std::vector<float> wo((size_t)C * 7 * 4);
    for (int o = 0; o < 4; ++o)
      for (int ci = 0; ci < C; ++ci)
        for (int k = 0; k < 7; ++k) wo[((size_t)ci * 7 + k) * 4 + o] = w[((size_t)o * C + ci) * 7 + k];
    out_w.upload(wo);
    out_b.upload(bo);
  } else if (out_ch == 1) {
    out_w.upload(w);
    out_b.upload(bo);
  }
}

}  // namespace

static void melgan_finalize(tts_ctx* c, int in_ch, int out_ch, int base, const int32_t* ups, int n_up, int nres,
                     int use_pqmf) {
  auto& G = c->mg;
  const auto& m = c->mg_host;
  G.ready = false;
  TTS_CHECK(nres >= 1 && nres <= 4, "num_res_blocks must be in [1, 4] (dilation <= 27)");
  G.in_ch = in_ch;
  G.out_ch = out_ch;
  G.base = base;
  G.nres = nres;
  G.pqmf = use_pqmf;
  G.ups.assign(ups, ups + n_up);
  G.convT.clear();
  G.dconv.clear();
  G.fused.clear();
  G.convT.resize(n_up);
  G.convTm.clear();
  G.convTm.resize(n_up);
  G.dconv.resize((size_t)n_up * nres);
  G.fused.resize((size_t)n_up * nres);
  G.rb_wd16.clear();
  G.rb_wf16.clear();
  G.rb_wd16.resize((size_t)n_up * nres);
  G.rb_wf16.resize((size_t)n_up * nres);
  G.rb_wd16p.clear();
  G.rb_wd16p.resize((size_t)n_up * nres);
  int pl3[8] = {3};
  {
    auto w = wn_weight(m, "layers.1", {base, in_ch, 7});
    pack_conv(G.conv_in, w, need(m, "layers.1.bias", {base}).d, in_ch, base, 7, 1, 1, pl3);
  }
  int idx = 2, C = base;
  for (int i = 0; i < n_up; ++i) {
    const int u = ups[i];
    TTS_CHECK(u % 2 == 0 && u <= 8, "upsample factors must be even and <= 8");
    const int cin = base >> i, cout = base >> (i + 1);
    const std::string nm = "layers." + std::to_string(idx + 1);
    auto wt = wn_weight(m, nm, {cin, cout, 2 * u});  // ConvTranspose1d weight (Cin, Cout, K)
    pack_convT(G.convT[i], G.convTm[i], wt, need(m, nm + ".bias", {cout}).d, u, cin, cout);
    C = cout;
    for (int bk = 0; bk < nres; ++bk) {
      int dil = 1;
      for (int q = 0; q < bk; ++q) dil *= 3;
      const std::string bn = "layers." + std::to_string(idx + 2) + ".blocks." + std::to_string(bk);
      const std::string sn = "layers." + std::to_string(idx + 2) + ".shortcuts." + std::to_string(bk);
      const size_t j = (size_t)i * nres + bk;
      pack_res_block({G.dconv[j], G.fused[j], G.rb_wd16[j], G.rb_wf16[j], G.rb_wd16p[j]}, wn_weight(m, bn + ".2", {C, C, 3}),
                     need(m, bn + ".2.bias", {C}).d, wn_weight(m, bn + ".4", {C, C, 1}), need(m, bn + ".4.bias", {C}).d,
                     wn_weight(m, sn, {C, C, 1}), need(m, sn + ".bias", {C}).d, C, dil);
    }
    idx += 3;
  }
  {
    const std::string nm = "layers." + std::to_string(idx + 2);
    auto w = wn_weight(m, nm, {out_ch, C, 7});
    const auto& bo = need(m, nm + ".bias", {out_ch}).d;
    pack_conv(G.conv_out, w, bo, C, out_ch, 7, 1, 1, pl3);
    G.C_last = C;
    pack_out_conv(G.out_w, G.out_b, w, bo, C, out_ch);
  }
  if (use_pqmf) {
    const auto& g = need(m, "pqmf_layer.G", {}).d;
    auto it = m.find("pqmf_layer.G");
    TTS_CHECK(it->second.shape.size() == 3 && it->second.shape[1] == out_ch, "pqmf_layer.G shape");
    G.taps = (int)it->second.shape[2] - 1;
    G.G.upload(g);
  }
  HIP_OK(hipDeviceSynchronize());
  G.ready = true;
}

namespace {

// One generator run: the call, where its lengths and range flag are, and the running activation
// x (B, C, Ls) at mul positions per mel frame (xo: the other ping-pong buffer)
struct GenRun {
  tts_ctx* c;
  const VocCall& v;
  hipStream_t s;
  const int* lens;  // device lengths (mel frames); v.h_lens: the same on the host, or per-row upper bounds
  unsigned* oflow;  // range flag: the split-f16 kernels run; null: fp32
  int Lb, pad;      // the longest row's padded mel frames, inference padding
  float *x, *xo;
  int C, mul;
  long Ls;
  // a conv of this run over max_q positions, on the run's own range flag
  ConvCall conv(int max_q) const {
    ConvCall cc;
    cc.lens = lens;
    cc.B = v.B;
    cc.max_q = max_q;
    cc.oflow = oflow;
    cc.len_add = 2 * pad;
    return cc;
  }
  void wrote(int C_, long Ls_, int mul_) {  // a step wrote the next activation into xo
    std::swap(x, xo);
    C = C_;
    Ls = Ls_;
    mul = mul_;
  }
};

// argument checks, workspace, lengths on the device
GenRun gen_begin(tts_ctx* c, const VocCall& v) {
  auto& G = c->mg;
  auto& W = c->mws;
  const int32_t* h_lens = v.h_lens;
  const int B = v.B, M_max = v.M_max, pad = v.pad;
  hipStream_t s = v.s ? v.s : c->s;
  TTS_CHECK(G.ready, "melgan weights not finalized");
  TTS_CHECK(B >= 1, "B >= 1");
  for (int b = 0; b < B && !v.dev_lens; ++b) {
    TTS_CHECK(h_lens[b] >= 1 && h_lens[b] <= M_max, "mel lens out of range");
    TTS_CHECK(h_lens[b] + 2 * pad >= 4, "ReflectionPad1d(3): mel frames + 2*padding must be >= 4");
    for (int k = 0; k < G.nres && !G.ups.empty(); ++k)  // ResidualStack ReflectionPad1d(dilation), stage 0
      TTS_CHECK((long)(h_lens[b] + 2 * pad) * G.ups[0] > G.dconv[k].dil,
                "ReflectionPad1d: a residual stack's dilation must be < the first stage's length");
  }
  const int Lb = M_max + 2 * pad;
  size_t maxelems = (size_t)G.base * Lb;
  {
    int mul = 1, Cc = G.base;
    for (int u : G.ups) {
      mul *= u;
      Cc /= 2;
      maxelems = std::max(maxelems, (size_t)Cc * Lb * mul);
    }
  }
  // device lengths: the ticket slot's (a fused submission's vocoder) or the workspace's
  int* vld = v.d_lens;
  if (!vld) {
    W.lens.ensure(B * 4);
    vld = W.lens.i();
  }
  W.xa.ensure((size_t)B * maxelems * 4);
  W.xb.ensure((size_t)B * maxelems * 4);
  if (!v.dev_lens) put_rows(vld, h_lens, B, s);
  else TTS_CHECK(v.d_lens || W.lens.bytes >= (size_t)B * 4, "vocoder lengths buffer");
  unsigned* oflow = c->gemm_x3 && v.flag ? v.flag : x3_flag(c);
  // no activation yet: the input conv writes xo = W.xa
  return GenRun{c, v, s, vld, oflow, Lb, pad, W.xb.f(), W.xa.f(), 0, 1, 0};
}

// layers[0..1]: replicate pad (inference_padding) + ReflectionPad1d(3) + Conv1d(k7) on the mel
void gen_input_conv(GenRun& r) {
  const auto& G = r.c->mg;
  const VocCall& v = r.v;
  ConvCall cc = r.conv(r.Lb);
  if (const int64_t* st = v.mel_strides) {
    TTS_CHECK(st[1] >= 1 && st[2] >= 1 && st[1] < (1L << 31) && st[2] < (1L << 31) && (st[0] >= 1 || v.B == 1) &&
                  st[0] >= 0,
              "mel strides must be positive");
    TTS_CHECK(st[1] != 1 || (st[2] % 4 == 0 && (reinterpret_cast<uintptr_t>(v.mel) & 15) == 0),
              "channel stride 1 needs a frame stride divisible by 4 and a 16-byte aligned mel");
    cc.in(v.mel, Layout{(long)st[0], (int)st[1], (int)st[2]}, G.in_ch);
  } else {
    cc.in(v.mel, bct(G.in_ch, v.M_max), G.in_ch);
  }
  cc.pad_mode = 1;
  cc.rep_pad = r.pad;
  cc.to(r.xo, bct(G.base, r.Lb));
  run_conv(G.conv_in, cc, r.s);
  r.wrote(G.base, r.Lb, 1);
}

// LeakyReLU + ConvTranspose1d of stage i: all u phases as one GEMM over input positions 0 .. L
// (split-f16, phase-merged weights), or u polyphase 2-tap convs
void gen_conv_transpose(GenRun& r, size_t i) {
  const auto& G = r.c->mg;
  const int u = G.ups[i], Cn = r.C / 2;
  const long Ln = r.Ls * u;
  const bool merged = r.oflow && G.convTm[i].W16.p;
  ConvCall t = r.conv(merged ? r.Lb * r.mul + 1 : r.Lb * r.mul);
  t.in(r.x, bct(r.C, r.Ls), r.C, 1).to(r.xo, bct(Cn, Ln));
  t.in_mul = t.q_mul = r.mul;
  t.out_mul = merged ? 1 : u;
  t.merged_u = merged ? u : 0;
  run_conv(merged ? G.convTm[i] : G.convT[i], t, r.s);
  r.wrote(Cn, Ln, r.mul * u);
}

// Blocks 0-2 of stage i as one resstack_x3 launch, over the stage's input x; with_ct: x is the
// ConvTranspose's input and the kernel computes the stage's input per tile (LeakyReLU +
// ConvTranspose1d + blocks 0-2, resstack_x3.hip CTU = 2). False, and nothing launched, if not covered.
bool gen_stack(GenRun& r, size_t i, bool with_ct) {
  const auto& G = r.c->mg;
  const int u = G.ups[i];
  if (with_ct && !(u == 2 && r.C == 96 && sw::ct_fuse() && r.oflow && G.convTm[i].W16.p)) return false;
  const int Cs = with_ct ? r.C / 2 : r.C, muls = with_ct ? r.mul * u : r.mul;
  const long Lss = with_ct ? r.Ls * u : r.Ls;
  if (!(r.oflow && G.nres >= 3 && sw::stack_fuse() && G.rb_wd16[i * G.nres].p)) return false;
  if (Cs == 96 && !sw::stack_fuse96()) return false;
  int dil[3];
  for (int k = 0; k < 3; ++k) dil[k] = G.dconv[i * G.nres + k].dil;
  if (!resstack_x3_supported(Cs, dil, 3)) return false;
  StackArgs sa{};
  sa.B = r.v.B;
  sa.x = with_ct ? nullptr : r.x;
  sa.y = r.xo;
  sa.sb = (long)Cs * Lss;
  sa.Ls = (int)Lss;
  sa.lens = r.lens;
  sa.len_add = 2 * r.pad;
  sa.mul = muls;
  for (int k = 0; k < 3; ++k) {
    sa.dil[k] = dil[k];
    sa.wd16[k] = Cs % 32 == 16 ? G.rb_wd16p[i * G.nres + k].p : G.rb_wd16[i * G.nres + k].p;
    sa.wf16[k] = G.rb_wf16[i * G.nres + k].p;
    sa.bd[k] = G.dconv[i * G.nres + k].bias.f();
    sa.bf[k] = G.fused[i * G.nres + k].bias.f();
  }
  sa.oflow = r.oflow;
  if (with_ct) {
    sa.xin = r.x;
    sa.sb_in = (long)r.C * r.Ls;
    sa.Ls_in = (int)r.Ls;
    sa.ct16 = G.convTm[i].W16.p;
    sa.ct_bias = G.convTm[i].bias.f();
  }
  if (!resstack_x3_fits(sa, r.v.h_lens)) return false;
  launch_resstack_x3(sa, r.v.h_lens, Cs, r.s);
  r.wrote(Cs, Lss, muls);
  return true;
}

// one fused ResidualStack block (resblock_x3.hip split-f16, or resblock.hip fp32)
void gen_block(GenRun& r, size_t i, int bk) {
  const auto& G = r.c->mg;
  const ConvLayer& dl = G.dconv[i * G.nres + bk];
  const ConvLayer& fl = G.fused[i * G.nres + bk];
  ResArgs ra{};
  ra.x = r.x;
  ra.y = r.xo;
  ra.sb = (long)r.C * r.Ls;
  ra.Ls = (int)r.Ls;
  ra.lens = r.lens;
  ra.len_add = 2 * r.pad;
  ra.mul = r.mul;
  ra.dil = dl.dil;
  ra.Wd = dl.W.f();
  ra.bd = dl.bias.f();
  ra.Wf = fl.W.f();
  ra.bf = fl.bias.f();
  ra.max_q = r.Lb * r.mul;
  ra.B = r.v.B;
  const DevBuf& w16 = G.rb_wd16[i * G.nres + bk];
  if (r.oflow && w16.p) {
    ra.Wd16 = w16.p;
    ra.Wf16 = G.rb_wf16[i * G.nres + bk].p;
    ra.oflow = r.oflow;
    launch_resblock_x3(ra, r.v.h_lens, r.C, r.s);
  } else {
    launch_resblock(ra, r.C, r.s);
  }
  r.wrote(r.C, r.Ls, r.mul);
}

// LeakyReLU + ReflectionPad1d(3) + Conv1d(k7) + tanh into out (B, out_ch, Ls), rows zero past their length
void gen_output_conv(GenRun& r, float* out) {
  const auto& G = r.c->mg;
  const int B = r.v.B;
  if (G.out_ch == 1) {  // full-band output stage on the VALU (melgan_out.hip)
    HIP_OK(hipMemsetAsync(out, 0, (size_t)B * r.Ls * 4, r.s));
    launch_out_conv1(r.x, (long)r.C * r.Ls, r.Ls, r.C, G.out_w.f(), G.out_b.f(), r.lens, 2 * r.pad, r.mul,
                     (int)(r.Lb * r.mul), B, out, r.Ls, r.s);
    return;
  }
  ConvCall o = r.conv(r.Lb * r.mul);
  o.in(r.x, bct(r.C, r.Ls), r.C, 1).to(out, bct(G.out_ch, r.Ls));
  o.pad_mode = 1;
  o.in_mul = o.q_mul = r.mul;
  o.epi = 2;
  HIP_OK(hipMemsetAsync(out, 0, (size_t)B * G.out_ch * r.Ls * 4, r.s));
  run_conv(G.conv_out, o, r.s);
}

}  // namespace

int ttsh::run_generator(tts_ctx* c, const VocCall& v, float* out, GenTail* tail) {
  GenRun r = gen_begin(c, v);
  const auto& G = c->mg;
  gen_input_conv(r);
  int up = 1;
  for (size_t i = 0; i < G.ups.size(); ++i) {
    up *= G.ups[i];
    // ConvTranspose and blocks 0-2 in one launch; else the ConvTranspose, then blocks 0-2 in one
    // launch; the blocks neither covers run one by one
    int bk = 0;
    if (gen_stack(r, i, /*with_ct=*/true)) {
      bk = 3;
    } else {
      gen_conv_transpose(r, i);
      if (gen_stack(r, i, /*with_ct=*/false)) bk = 3;
    }
    for (; bk < G.nres; ++bk) gen_block(r, i, bk);
  }
  if (tail) *tail = GenTail{r.x, r.C, r.Ls, r.mul};  // the fused output conv + PQMF kernel takes it from here
  else gen_output_conv(r, out);
  return up;
}

void ttsh::mbmelgan_body(tts_ctx* c, const VocCall& v, float* d_wav) {
  hipStream_t s = v.s ? v.s : c->s;
  const int B = v.B, pad = v.pad;
  auto& G = c->mg;
  int up = 1;
  for (int u : G.ups) up *= u;
  const long Ls = (long)(v.M_max + 2 * pad) * up;
  const bool fused = G.out_ch == 4 && G.taps == 62 && (G.C_last == 32 || G.C_last == 48);
  if (fused) {  // launch_out_pqmf writes the rows' zero padding itself
    GenTail t;
    run_generator(c, v, nullptr, &t);
    TTS_CHECK(t.Ls == Ls, "generator length bookkeeping");
    const int* dl = v.d_lens ? v.d_lens : c->mws.lens.i();
    TTS_CHECK(launch_out_pqmf(t.x, (long)t.C * t.Ls, t.Ls, t.C, G.out_w.f(), G.out_b.f(), G.G.f(), G.out_ch,
                              G.taps, dl, 2 * pad, up, (int)Ls, B, d_wav, (long)G.out_ch * Ls, s),
              "fused output/PQMF shape not covered");
  } else {
    HIP_OK(hipMemsetAsync(d_wav, 0, (size_t)B * G.out_ch * Ls * 4, s));
    c->mws.bands.ensure((size_t)B * G.out_ch * Ls * 4);
    run_generator(c, v, c->mws.bands.f());
    const int* dl = v.d_lens ? v.d_lens : c->mws.lens.i();
    launch_pqmf_synthesis(c->mws.bands.f(), (long)G.out_ch * Ls, Ls, G.G.f(), G.out_ch, G.taps, dl,
                          2 * pad, up, (int)Ls, B, d_wav, (long)G.out_ch * Ls, s);
  }
}

int ttsh::vocoder_min_len(const MelganModel& G, int pad) {
  int L = std::max(1, 4 - 2 * pad);
  for (int k = 0; k < G.nres && !G.ups.empty(); ++k)
    while ((long)(L + 2 * pad) * G.ups[0] <= G.dconv[k].dil) ++L;
  return L;
}

static int melgan_infer_impl(tts_ctx* c, const float* d_mel, const int64_t* mel_strides, const int32_t* h_lens, int B,
                             int M_max, int pad, float* d_wav, void* stream) {
  return ctx_call(
      c, stream,
      [&] {
        TTS_CHECK(c && d_mel && h_lens && d_wav, "null argument");
        TTS_CHECK(pad >= 0, "pad >= 0");
        TTS_CHECK(c->mg.ready && c->mg.pqmf, "melgan (with PQMF) not finalized");
      },
      [&] { mbmelgan_body(c, VocCall{d_mel, mel_strides, h_lens, B, M_max, pad}, d_wav); });
}

extern "C" {

int tts_melgan_set_tensor(tts_ctx* c, const char* name, const float* h, const int64_t* shape, int ndim) {
  return stage_tensor(c, &tts_ctx::mg_host, name, h, shape, ndim);
}

int tts_melgan_finalize(tts_ctx* c, int in_ch, int out_ch, int base, const int32_t* ups, int n_up, int nres,
                        int use_pqmf) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && ups && n_up >= 1 && n_up <= 6, "bad arguments");
    DeviceGuard g(c->device);
    HIP_OK(hipStreamSynchronize(c->sv));  // no submitted vocoder still reads the weights replaced here
    c->sv_live = false;
    HostMapConsumer consume{c->mg_host};
    melgan_finalize(c, in_ch, out_ch, base, ups, n_up, nres, use_pqmf);
  });
}

int tts_melgan_generator(tts_ctx* c, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                         float* d_out, void* stream) {
  return ctx_call(
      c, stream,
      [&] {
        TTS_CHECK(c && d_mel && h_lens && d_out, "null argument");
        TTS_CHECK(pad >= 0, "pad >= 0");
      },
      [&] { run_generator(c, VocCall{d_mel, nullptr, h_lens, B, M_max, pad}, d_out); });
}

int tts_melgan_infer(tts_ctx* c, const float* d_mel, const int32_t* h_lens, int B, int M_max, int pad,
                     float* d_wav, void* stream) {
  return melgan_infer_impl(c, d_mel, nullptr, h_lens, B, M_max, pad, d_wav, stream);
}

int tts_melgan_infer_strided(tts_ctx* c, const float* d_mel, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                             const int32_t* h_lens, int B, int M_max, int pad, float* d_wav, void* stream) {
  const int64_t st[3] = {stride_b, stride_c, stride_t};
  return melgan_infer_impl(c, d_mel, st, h_lens, B, M_max, pad, d_wav, stream);
}

int tts_test_voc(tts_ctx* c, tts_voc_test* d, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(d && d->d_x && d->d_y && d->h_lens, "test_voc: null argument");
    TTS_CHECK(d->kind >= 0 && d->kind <= 5, "test_voc: kind must be in [0, 5]");
    TTS_CHECK(d->C >= 16 && d->C % 16 == 0 && d->C <= 1024 && d->B >= 1 && d->B <= 4096 && d->max_q >= 0 && d->mul >= 1,
              "test_voc: sizes");
    const int kind = d->kind, C = d->C, B = d->B;
    const int nblk = kind <= 1 ? 1 : (kind <= 3 ? 3 : 0);
    for (int k = 0; k < nblk; ++k)
      TTS_CHECK(d->wd[k] && d->bd[k] && d->w1[k] && d->b1[k] && d->ws[k] && d->bs[k], "test_voc: null block weights");
    TTS_CHECK(kind != 3 || (d->ct_w && d->ct_b), "test_voc: null ConvTranspose weights");
    TTS_CHECK(kind < 4 || (d->wo && d->bo && (kind == 5 || d->G)), "test_voc: null output weights");
    TTS_CHECK(kind != 4 || (d->N >= 1 && d->N <= 8 && d->taps >= 0), "test_voc: bands / taps");
    for (int i = 0; i < 2; ++i)
      TTS_CHECK(d->x_strides[i] >= 0 && d->y_strides[i] >= 0 && d->x_strides[1] < (1L << 31) && d->y_strides[1] < (1L << 31),
                "test_voc: strides");
    TTS_CHECK(kind >= 3 || (d->x_strides[0] == d->y_strides[0] && d->x_strides[1] == d->y_strides[1]),
              "test_voc: the block and stack kernels take one pair of strides for x and y");
    d->tq = 0;
    d->range_flag = 0;
    DeviceGuard g(c->device);
    enter(c, stream);
    const int32_t* bounds = d->h_bounds ? d->h_bounds : d->h_lens;
    // everything packed here is freed when this scope ends: wait for the launch first, also on an error
    ConvLayer dconv[3], fused[3], ctL, ctM;
    DevBuf wd16[3], wf16[3], wd16p[3], out_w, out_b, Gd, lens;
    struct Sync {
      hipStream_t s;
      ~Sync() { (void)hipStreamSynchronize(s); }
    } sync{c->s};
    auto vec = [](const float* p, size_t n) { return std::vector<float>(p, p + n); };
    for (int k = 0; k < nblk; ++k)
      pack_res_block({dconv[k], fused[k], wd16[k], wf16[k], wd16p[k]}, vec(d->wd[k], (size_t)C * C * 3), vec(d->bd[k], C),
                     vec(d->w1[k], (size_t)C * C), vec(d->b1[k], C), vec(d->ws[k], (size_t)C * C), vec(d->bs[k], C), C,
                     d->dil[k]);
    c->x3flag.ensure(4);
    unsigned* flag = reinterpret_cast<unsigned*>(c->x3flag.p);
    HIP_OK(hipMemsetAsync(flag, 0, 4, c->s));
    const int* dl = put_rows(lens, d->h_lens, B, c->s);
    if (kind <= 1) {
      ResArgs ra{};
      ra.x = d->d_x;
      ra.y = d->d_y;
      ra.sb = (long)d->y_strides[0];
      ra.Ls = (int)d->y_strides[1];
      ra.lens = dl;
      ra.len_add = d->len_add;
      ra.mul = d->mul;
      ra.dil = dconv[0].dil;
      ra.Wd = dconv[0].W.f();
      ra.bd = dconv[0].bias.f();
      ra.Wf = fused[0].W.f();
      ra.bf = fused[0].bias.f();
      ra.max_q = d->max_q;
      ra.B = B;
      if (kind == 1) {
        ra.Wd16 = wd16[0].p;
        ra.Wf16 = wf16[0].p;
        ra.oflow = flag;
        d->tq = launch_resblock_x3(ra, bounds, C, c->s);
      } else {
        d->tq = launch_resblock(ra, C, c->s);
      }
    } else if (kind <= 3) {
      StackArgs sa{};
      sa.B = B;
      sa.x = kind == 2 ? d->d_x : nullptr;
      sa.y = d->d_y;
      sa.sb = (long)d->y_strides[0];
      sa.Ls = (int)d->y_strides[1];
      sa.lens = dl;
      sa.len_add = d->len_add;
      sa.mul = d->mul;
      for (int k = 0; k < 3; ++k) {
        sa.dil[k] = dconv[k].dil;
        sa.wd16[k] = C % 32 == 16 ? wd16p[k].p : wd16[k].p;
        sa.wf16[k] = wf16[k].p;
        sa.bd[k] = dconv[k].bias.f();
        sa.bf[k] = fused[k].bias.f();
      }
      sa.oflow = flag;
      if (kind == 3) {
        pack_convT(ctL, ctM, vec(d->ct_w, (size_t)2 * C * C * 4), vec(d->ct_b, C), 2, 2 * C, C);
        TTS_CHECK(ctM.W16.p, "test_voc: the merged ConvTranspose has no split-f16 weights");
        sa.xin = d->d_x;
        sa.sb_in = (long)d->x_strides[0];
        sa.Ls_in = (int)d->x_strides[1];
        sa.ct16 = ctM.W16.p;
        sa.ct_bias = ctM.bias.f();
      }
      d->tq = launch_resstack_x3(sa, bounds, C, c->s);
    } else if (kind == 4) {
      pack_out_conv(out_w, out_b, vec(d->wo, (size_t)d->N * C * 7), vec(d->bo, d->N), C, d->N);
      TTS_CHECK(out_w.p, "fused output/PQMF shape not covered");
      Gd.upload(vec(d->G, (size_t)d->N * (d->taps + 1)));
      int tq = 0;
      TTS_CHECK(launch_out_pqmf(d->d_x, (long)d->x_strides[0], (long)d->x_strides[1], C, out_w.f(), out_b.f(), Gd.f(), d->N,
                                d->taps, dl, d->len_add, d->mul, d->max_q, B, d->d_y, (long)d->y_strides[0], c->s, &tq),
                "fused output/PQMF shape not covered");
      d->tq = tq;
    } else {
      pack_out_conv(out_w, out_b, vec(d->wo, (size_t)C * 7), vec(d->bo, 1), C, 1);
      d->tq = launch_out_conv1(d->d_x, (long)d->x_strides[0], (long)d->x_strides[1], C, out_w.f(), out_b.f(), dl, d->len_add,
                               d->mul, d->max_q, B, d->d_y, (long)d->y_strides[0], c->s);
    }
    HIP_OK(hipMemcpyAsync(&c->pinned[PIN_FLAG], flag, 4, hipMemcpyDeviceToHost, c->s));
    HIP_OK(hipStreamSynchronize(c->s));
    d->range_flag = (uint32_t)c->pinned[PIN_FLAG];
    leave(c, stream);
  });
}

int tts_pqmf_synthesis(tts_ctx* c, const float* d_x, int B, int N, int L, const float* d_G, int taps, float* d_y,
                       void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && d_x && d_G && d_y, "null argument");
    TTS_CHECK(B >= 1 && N >= 1 && N <= 8 && L >= 1 && taps >= 0, "bad sizes");
    DeviceGuard g(c->device);
    enter(c, stream);
    const int* dl = fill_rows(c->mws.lens, L, B, c->s);
    launch_pqmf_synthesis(d_x, (long)N * L, L, d_G, N, taps, dl, 0, 1, L, B, d_y, (long)N * L, c->s);
    HIP_OK(hipStreamSynchronize(c->s));
    leave(c, stream);
  });
}

}  // extern "C"
