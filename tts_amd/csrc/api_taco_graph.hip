// Tacotron2, the captured-graph decoder: the five launches of a decoder step (decoder.hip's per-step
// kernels), their CHUNK-step graphs polled by the host, and tts_time_decoder_kernel. The fallback of
// the persistent decoder (TTS_DECODER=graph, or a device it does not fit).
#include "host.h"
#include "decoder.h"

using namespace ttsh;

namespace {

// columns [k0, k0 + K) of a fragment-order activation with Ktot columns
SkSeg seg(const float* base, int Ktot, int k0, int K) {
  SkSeg s;
  s.ptr = base + (long)(k0 / 16) * 256;
  s.ms = 16 * Ktot;
  s.K = K;
  return s;
}

// the 5 launches of decoder step j of a chunk (parity j & 1 selects the h_dec buffer) over the
// first MT batch tiles (rows >= 16*MT must all be finished)
void enqueue_step(tts_ctx* c, int j, int which_only, hipStream_t s, int MT) {
  auto& M = c->taco;
  auto& W = c->tws;
  const DecDev d = make_dev(c, std::min(W.B, 16 * MT));
  const int r = W.r, YLD = 80 * M.r_init;
  float* hd_cur = (j & 1) ? W.hdec1.f() : W.hdec0.f();
  float* hd_nxt = (j & 1) ? W.hdec0.f() : W.hdec1.f();
  if (which_only < 0 || which_only == 1) {  // K1: prenet layers 1+2 || stop(t-1)
    SkArgs a{};
    a.njobs = 2;
    a.MT = MT;
    SkJob& J = a.job[0];  // layer 1 (result kept in LDS)
    J.seg[0] = seg(W.y.f(), YLD, 80 * (r - 1), 80);
    J.nseg = 1;
    J.K = 80;
    J.W = M.pre1.f();
    J.ntiles = 16;
    SkJob& J2 = a.job[1];  // layer 2
    J2.K = 256;
    J2.W = M.pre2.f();
    J2.ntiles = 16;
    J2.out = W.pb.f();
    J2.out_ld = 256;
    J2.out_frag = 1;
    StopArgs st{};
    st.part = W.spart.f();
    st.threshold = W.thr;
    launch_prenet_stop(a, d, st, j, s);
  }
  if (which_only < 0 || which_only == 3) {  // K2: attention_rnn + partial query projection
    SkArgs a{};
    a.njobs = 1;
    a.MT = MT;
    SkJob& J = a.job[0];
    J.seg[0] = seg(W.pb.f(), 256, 0, 256);
    J.nseg = 1;
    J.K = 256;
    J.W = M.att_p.f();
    J.ntiles = 256;
    J.epi = EPI_LSTM;
    J.addin = W.gatt.f();
    J.addin_ld = 4096;
    J.h_out = W.hatt.f();
    J.c_state = W.catt.f();
    J.hc_ld = 1024;
    J.WqT = M.WqT.f();
    J.pq_part = W.pq.f();
    J.pq_cap = 128;
    launch_skinny(a, d, j, 2, 4, s);  // 128 workgroups of 8 units: 128 query partials
  }
  if (which_only < 0 || which_only == 4) {  // K3: attention
    AttnArgs p{};
    p.pq_part = W.pq.f();
    p.npq = 128;
    p.Bp = MT * 16;
    p.alpha = W.alpha.f();
    p.alpha_cum = W.acum.f();
    p.Wloc = M.Wloc.f();
    p.WdT = M.Wdense.f();
    p.v = M.v.f();
    p.bv = M.bv;
    p.penc = W.penc.f();
    p.energy = W.energy.f();
    p.enc = W.enc.f();
    p.ctx = W.ctx.f();
    p.part_s = W.aps.f();
    p.part_m = W.apm.f();
    p.part_u = W.apu.f();
    p.counter = reinterpret_cast<unsigned*>(W.acnt.p);
    p.nchmax = (W.T_max + 15) / 16;
    p.softmax = M.softmax;
    launch_attention(p, d, j, s);
  }
  if (which_only < 0 || which_only == 0) {  // K4: decoder_rnn LSTMCell
    SkArgs a{};
    a.njobs = 1;
    a.MT = MT;
    SkJob& J = a.job[0];
    J.seg[0] = seg(W.hatt.f(), 1024, 0, 1024);
    J.seg[1] = seg(W.ctx.f(), 512, 0, 512);
    J.seg[2] = seg(hd_cur, 1024, 0, 1024);
    J.nseg = 3;
    J.K = 2560;
    J.W = M.dec_w.f();
    J.ntiles = 256;
    J.epi = EPI_LSTM;
    J.bias = M.dec_bias.f();
    J.h_out = hd_nxt;
    J.c_state = W.cdec.f();
    J.hc_ld = 1024;
    launch_skinny(a, d, j, 1, 4, s);
  }
  if (which_only < 0 || which_only == 5) {  // K5: projection + stop logit || next attention_rnn ctx/h part
    SkArgs a{};
    a.njobs = 2;
    a.MT = MT;
    SkJob& J = a.job[0];
    J.seg[0] = seg(hd_nxt, 1024, 0, 1024);
    J.seg[1] = seg(W.ctx.f(), 512, 0, 512);
    J.nseg = 2;
    J.K = 1536;
    J.W = M.proj_w.f();
    J.ntiles = 1 + 5 * r;  // stopnet tile + the first r frames (tacotron2.py:297)
    J.epi = EPI_STORE;
    J.bias = M.proj_b.f();
    J.out = W.y.f();
    J.out_ld = YLD;
    J.out_frag = 1;
    J.frames_r = r;
    J.lead_stop = 1;
    J.stop_part = W.spart.f();
    SkJob& J2 = a.job[1];  // (+ biases)
    J2.seg[0] = seg(W.ctx.f(), 512, 0, 512);
    J2.seg[1] = seg(W.hatt.f(), 1024, 0, 1024);
    J2.nseg = 2;
    J2.K = 1536;
    J2.W = M.att_pre.f();
    J2.ntiles = 256;
    J2.epi = EPI_STORE;
    J2.bias = M.att_bias.f();
    J2.out = W.gatt.f();
    J2.out_ld = 4096;
    launch_skinny(a, d, j, 1, 4, s);
  }
}

// CHUNK-step graph for batch tile count MT (captured once per configuration)
hipGraphExec_t step_graph(tts_ctx* c, int MT, hipStream_t s) {
  auto& W = c->tws;
  if (W.graphs[MT]) return W.graphs[MT];
  hipGraph_t g;
  HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  try {
    for (int j = 0; j < CHUNK; ++j) enqueue_step(c, j, -1, s, MT);
    launch_dec_advance(&ctl_block(W)->ctl, CHUNK, s);
  } catch (...) {
    hipGraph_t tmp;
    (void)hipStreamEndCapture(s, &tmp);
    throw;
  }
  HIP_OK(hipStreamEndCapture(s, &g));
  HIP_OK(hipGraphInstantiate(&W.graphs[MT], g, nullptr, nullptr, 0));
  HIP_OK(hipGraphDestroy(g));
  return W.graphs[MT];
}

}  // namespace

// the decode as captured CHUNK-step graphs (decoder.hip's per-step kernels), polled by the host
void ttsh::run_graph_decoder(tts_ctx* c, int B, int T_max, int S_cap, int r, float thr, int max_ms, hipStream_t s) {
  auto& W = c->tws;
  // step graphs, cached per configuration / buffer generation
  if (W.graph_gen != W.gen || W.gB != B || W.gT != T_max || W.gS != S_cap || W.gr != r || W.gthr != thr) {
    for (auto& ge : W.graphs)
      if (ge) {
        HIP_OK(hipGraphExecDestroy(ge));
        ge = nullptr;
      }
    W.graph_gen = W.gen;
    W.gB = B;
    W.gT = T_max;
    W.gS = S_cap;
    W.gr = r;
    W.gthr = thr;
  }
  for (int mt = 1; mt <= W.MT; ++mt) step_graph(c, mt, s);
  // run chunks until every utterance is done (checked one chunk behind) or t > max steps; drop
  // to fewer batch tiles once the trailing rows have all finished
  const int chunks_max = max_ms / CHUNK + 1;  // covers t = max_ms (stop of the last step)
  bool done = false;
  int mt = W.MT;
  for (int ch = 0; ch < chunks_max && !done; ++ch) {
    HIP_OK(hipGraphLaunch(W.graphs[mt], s));
    // {all_done, active_tiles} into the polling pair of this chunk's parity
    HIP_OK(hipMemcpyAsync(&c->pinned[PIN_CHUNK + 2 * (ch & 1)], &ctl_block(W)->ctl.all_done, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipEventRecord(c->ev_chunk[ch & 1], s));
    if (ch >= 1) {
      HIP_OK(hipEventSynchronize(c->ev_chunk[(ch - 1) & 1]));
      const int* pv = &c->pinned[PIN_CHUNK + 2 * ((ch - 1) & 1)];
      if (pv[0]) done = true;
      else if (pv[1] >= 1 && pv[1] < mt) mt = pv[1];
    }
  }
}

extern "C" {

int tts_time_decoder_kernel(tts_ctx* c, int which, int iters, float* ms_out) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && ms_out && iters >= 1, "bad arguments");
    TTS_CHECK(c->last_B > 0 && c->tws.graphs[c->tws.MT], "run tts_taco_infer first");
    TTS_CHECK(c->tws.S_cap >= CHUNK + 2, "S_cap too small for timing");
    DeviceGuard g(c->device);
    auto& W = c->tws;
    hipStream_t s = c->s;
    // live state of the last decode, re-armed: base = 1, nothing done, unbounded max steps
    DecCtlBlock ctl{};
    ctl.ctl.base = 1;
    std::fill(ctl.max_steps, ctl.max_steps + BMAX, 1 << 30);
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipMemcpyAsync(W.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    if (which == 0) enqueue_step(c, 0, 0, s, W.MT);  // warm-up
    else HIP_OK(hipGraphLaunch(W.graphs[W.MT], s));
    HIP_OK(hipMemcpyAsync(W.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) {
      if (which == 0) enqueue_step(c, 0, 0, s, W.MT);
      else {
        HIP_OK(hipGraphLaunch(W.graphs[W.MT], s));
      }
    }
    HIP_OK(hipEventRecord(e1, s));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = which == 0 ? ms / iters : ms / (iters * CHUNK);
    // leave the control block in a finished state
    ctl.ctl.all_done = 1;
    HIP_OK(hipMemcpy(W.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice));
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
  });
}

}  // extern "C"
