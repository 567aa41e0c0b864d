// Fused Tacotron2 + MB-MelGAN: a submission launches the vocoder on the decode's device-side
// lengths and returns a ticket; finishing the ticket orders the caller's stream after it.
#include "host.h"

using namespace ttsh;

namespace {

// the vocoder work just enqueued on sv: later entries join it (enter)
void sv_mark(tts_ctx* c) {
  HIP_OK(hipEventRecord(c->ev_sv, c->sv));
  c->sv_live = c->sv != c->s;
}
void sv_join(tts_ctx* c) {
  if (!c->sv_live) return;
  HIP_OK(hipStreamWaitEvent(c->s, c->ev_sv, 0));
  c->sv_live = false;
}

// completes a submitted fused call: if its split-f16 vocoder raised the range flag, the vocoder
// runs again on the fp32 kernels from the postnet output (the two-call path's fallback); then the
// caller's stream is ordered after it
void finish_ticket(tts_ctx* c, VocTicket& tk, void* stream) {
  if (!tk.pending) return;
  tk.pending = false;
  if (tk.x3) {
    HIP_OK(hipEventSynchronize(tk.ev));
    const int k = (int)(tk.id % NVT);
    if (c->pinned[TK_PIN + k]) {
      {  // on sv, behind any later submission's vocoder; the slot's lengths from the host
        Fp32Rerun f32(c);
        VocCall v{tk.d_post, tk.st, tk.lens.data(), tk.B, tk.M, tk.pad};
        v.s = c->sv;
        v.d_lens = vslot_lens(c, k);
        mbmelgan_body(c, v, tk.d_wav);
      }
      HIP_OK(hipEventRecord(tk.ev, c->sv));
      sv_mark(c);
    }
  }
  HIP_OK(hipStreamWaitEvent((hipStream_t)stream, tk.ev, 0));
}

// Tacotron2 decode + MB-MelGAN, submitted: the vocoder is launched on the device-side decoded
// lengths before the host waits for the decode's status words, and the call returns with the
// vocoder still running (ticket); finish_ticket completes it.
int64_t taco_mbmelgan_submit(tts_ctx* c, TacoCall call, int pad, float* d_wav) {
  const int64_t* d_ids = call.ids;
  const int32_t *h_lens = call.h_lens, *h_max_steps = call.run.h_max_steps;
  const int B = call.B, r = call.r, S_cap = call.run.S_cap;
  float *d_dec = call.d_dec, *d_post = call.d_post, *d_align = call.d_align, *d_stop = call.d_stop;
  int32_t *h_steps = call.run.h_steps, *h_status = call.run.h_status;
  void* stream = call.stream;
  TTS_CHECK(d_ids && h_lens && h_max_steps && d_dec && d_post && d_align && d_stop && d_wav && h_steps && h_status,
            "null argument");
  TTS_CHECK(pad >= 0, "pad >= 0");
  auto& G = c->mg;
  TTS_CHECK(G.ready && G.pqmf, "melgan (with PQMF) not finalized");
  TTS_CHECK(G.in_ch == 80, "vocoder input channels must be the decoder's 80 mel channels");
  TTS_CHECK(B >= 1 && B <= BMAX && r >= 1, "bad sizes");
  const int64_t id = c->next_ticket++;
  VocTicket& tk = c->vt[id % NVT];
  finish_ticket(c, tk, stream);  // the slot's previous submission completes first
  if (tk.id != 0) HIP_OK(hipStreamWaitEvent(c->s, tk.ev, 0));  // its vocoder is done with the slot
  tk.id = id;
  // per-row upper bounds of the decoded lengths (tile counts of the vocoder's persistent kernels)
  const int Lmin = vocoder_min_len(G, pad);
  std::vector<int32_t> bound(B);
  for (int b = 0; b < B; ++b) {
    TTS_CHECK(h_max_steps[b] >= 1 && h_max_steps[b] <= S_cap, "max_steps out of range");
    bound[b] = h_max_steps[b] * r;
    TTS_CHECK(bound[b] >= Lmin, VOC_SHORT_MSG);
  }
  const int64_t st[3] = {(int64_t)S_cap * r * 80, 1, 80};
  bool voc_x3 = false;
  const int k = (int)(id % NVT);
  int* slot = c->pinned + TK_PIN + k;
  int* vl = vslot_lens(c, k);
  unsigned* vf = vslot_flag(c, k);
  hipStream_t sv = c->sv;
  FusedVoc fv{vl, Lmin, [&] {
                voc_x3 = c->gemm_x3;
                // on sv behind the decode's status event (recorded just before), with the ticket
                // slot's lengths (the status kernel wrote them) and range flag; the vocoder's input
                // is the postnet output read in place, frame-major; rows are hop (S_cap r + 2 pad)
                // samples apart until the decoded lengths are on the host
                if (sv != c->s) HIP_OK(hipStreamWaitEvent(sv, c->ev_status, 0));
                if (voc_x3) HIP_OK(hipMemsetAsync(vf, 0, 4, sv));
                VocCall v{d_post, st, bound.data(), B, S_cap * r, pad, /*dev_lens=*/true, sv, vl, vf};
                mbmelgan_body(c, v, d_wav);
                if (voc_x3) HIP_OK(hipMemcpyAsync(slot, vf, 4, hipMemcpyDeviceToHost, sv));
                sv_mark(c);
              }};
  c->flag_read = false;
  call.run.fv = &fv;  // this submission's Tacotron2 does not wait for earlier vocoders on sv
  taco_run(c, call);
  call.run.fv = nullptr;
  const bool taco_oflow = c->gemm_x3 && c->flag_read && c->pinned[PIN_FLAG];
  c->flag_read = false;
  int S = 0;
  for (int b = 0; b < B; ++b) S = std::max(S, (int)h_steps[b]);
  std::vector<int32_t> mlens(B);
  for (int b = 0; b < B; ++b) mlens[b] = h_steps[b] * r;
  int up = 1;
  for (int u : G.ups) up *= u;
  const size_t row = (size_t)G.out_ch * up;  // hop: samples per mel frame
  if (taco_oflow) {
    // the decode left the f16 range: decode and vocoder again on the fp32 kernels (the split
    // vocoder already queued is overwritten), as the two separate calls would each have done
    {
      Fp32Rerun f32(c);
      sv_join(c);  // the split vocoder queued on sv writes d_wav before the fp32 one below
      taco_run(c, call);
      S = 0;
      for (int b = 0; b < B; ++b) {
        S = std::max(S, (int)h_steps[b]);
        mlens[b] = h_steps[b] * r;
      }
      mbmelgan_body(c, VocCall{d_post, st, mlens.data(), B, S * r, pad}, d_wav);
    }
    leave(c, stream);
    return id;
  }
  if (S < S_cap) {  // pack the rows to hop (S r + 2 pad) samples apart, as the two calls return them
    const size_t P = row * ((size_t)S * r + 2 * pad), Pc = row * ((size_t)S_cap * r + 2 * pad);
    c->mws.bands.ensure((size_t)B * P * 4);
    HIP_OK(hipMemcpy2DAsync(c->mws.bands.p, P * 4, d_wav, Pc * 4, P * 4, B, hipMemcpyDeviceToDevice, sv));
    HIP_OK(hipMemcpyAsync(d_wav, c->mws.bands.p, (size_t)B * P * 4, hipMemcpyDeviceToDevice, sv));
  }
  HIP_OK(hipEventRecord(tk.ev, sv));
  sv_mark(c);
  tk.pending = true;
  tk.x3 = voc_x3;
  tk.d_post = d_post;
  std::copy(st, st + 3, tk.st);
  tk.lens = mlens;
  tk.B = B;
  tk.M = S * r;
  tk.pad = pad;
  tk.d_wav = d_wav;
  return id;
}

}  // namespace

extern "C" {

int tts_taco_mbmelgan_submit(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                             const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                             const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                             int pad, float* d_wav, int32_t* h_steps, int32_t* h_status, int64_t* h_ticket,
                             void* stream) {
  TacoCall call;
  call.ids = d_ids, call.h_lens = h_lens, call.B = B, call.T_max = T_max, call.r = r, call.stream = stream;
  call.d_spk_ids = d_spk_ids, call.d_spk_emb = d_spk_emb;
  call.d_dec = d_dec, call.d_post = d_post, call.d_align = d_align, call.d_stop = d_stop;
  call.run = TacoFree{h_max_steps, S_cap, thr, h_steps, h_status};
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && h_ticket, "null argument");
    DeviceGuard g(c->device);
    *h_ticket = taco_mbmelgan_submit(c, call, pad, d_wav);
  });
}

int tts_taco_mbmelgan_finish(tts_ctx* c, int64_t ticket, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(ticket >= 1 && ticket < c->next_ticket, "unknown ticket");
    DeviceGuard g(c->device);
    VocTicket& tk = c->vt[ticket % NVT];
    if (tk.id == ticket) finish_ticket(c, tk, stream);  // else a later submission already finished it
  });
}

int tts_taco_mbmelgan_infer(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                            const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                            const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                            int pad, float* d_wav, int32_t* h_steps, int32_t* h_status, void* stream) {
  TacoCall call;
  call.ids = d_ids, call.h_lens = h_lens, call.B = B, call.T_max = T_max, call.r = r, call.stream = stream;
  call.d_spk_ids = d_spk_ids, call.d_spk_emb = d_spk_emb;
  call.d_dec = d_dec, call.d_post = d_post, call.d_align = d_align, call.d_stop = d_stop;
  call.run = TacoFree{h_max_steps, S_cap, thr, h_steps, h_status};
  return guarded_ctx(c, [&] {
    DeviceGuard g(c->device);
    const int64_t id = taco_mbmelgan_submit(c, call, pad, d_wav);
    VocTicket& tk = c->vt[id % NVT];
    if (tk.id == id) finish_ticket(c, tk, stream);
    HIP_OK(hipStreamSynchronize(c->sv));  // returns with the call's work done, as before
    HIP_OK(hipStreamSynchronize(c->s));
  });
}

}  // extern "C"
