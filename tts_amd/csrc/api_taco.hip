// Tacotron2, running: the encoder and postnet, the persistent decoder, taco_run (one driver for the
// free-running and the teacher-forced decode), and the tts_taco_* inference entry points.
#include "host.h"
#include "decoder.h"
#include "gsync.h"
#include "split16.h"
#include "switches.h"

#include <cstdio>

using namespace ttsh;

DecCtlBlock* ttsh::ctl_block(const TacoWS& W) { return static_cast<DecCtlBlock*>(W.ctl.p); }

DecDev ttsh::make_dev(tts_ctx* c, int Bact) {
  auto& W = c->tws;
  DecDev d{};
  DecCtlBlock* cb = ctl_block(W);
  d.ctl = &cb->ctl;
  d.done = cb->done;
  d.steps = cb->steps;
  d.status = cb->status;
  d.max_steps = cb->max_steps;
  d.lens = W.lens.i();
  d.dec_out = W.dec.f();
  d.align_out = W.align.f();
  d.stop_out = W.stop.f();
  d.S_cap = W.S_cap;
  d.T_max = W.T_max;
  d.B = Bact;
  return d;
}

namespace {

__global__ void bcast_rows_kernel(const float* src, int n, float* dst, int rows) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * rows; i += gridDim.x * blockDim.x)
    dst[i] = src[i % n];
}

// Per-row biases of the persistent decoder, one column per thread:
//   out[m][n] = base[n] + sum_e spk[m][e] WT[e][n]   (m < B; rows B..Bp-1 get base[n])
// base = 0 on the attention_rnn / decoder_rnn / processed-inputs columns, the projection bias on
// the projection columns [pj0, N). With no speaker (Es = 0) only the projection columns are built.
constexpr int SPK_BMAX = 64;
// Per-row speaker biases W_s s (+ the projection bias for the projection columns): out[m][n] for
// rows m < Bp. Workgroup = 64 columns x 4 waves, wave q summing the speaker dims e = q, q + 4, ...
// (the speaker values are wave-uniform scalar loads), the 4 partials added in a fixed order
// through LDS. Round 4: the previous form (one column per thread over all dims, 64 accumulators
// predicated on B) ran ~40 workgroups for ~400 us per call.
template <int MB>
__global__ __launch_bounds__(256) void spk_bias_kernel(const float* __restrict__ spk, int B, int Es,
                                                       const float* __restrict__ WT, int N,
                                                       const float* __restrict__ pjb, int pj0, int Bp,
                                                       float* __restrict__ out) {
  __shared__ float red[3][MB][64];
  const int c = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x * 64 + c;
  const int nc = min(n, N - 1);
  float acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = 0.f;
  for (int e = q; e < Es; e += 4) {
    const float w = WT[(long)e * N + nc];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const float sv = m < B ? spk[m * Es + e] : 0.f;  // wave-uniform
      acc[m] = fmaf(sv, w, acc[m]);
    }
  }
  if (q > 0) {
#pragma unroll
    for (int m = 0; m < MB; ++m) red[q - 1][m][c] = acc[m];
  }
  __syncthreads();
  if (q != 0 || n >= N) return;
  const float base = n >= pj0 ? pjb[n - pj0] : 0.f;
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < Bp) out[(long)m * N + n] = base + (m < B ? ((acc[m] + red[0][m][c]) + red[1][m][c]) + red[2][m][c] : 0.f);
  for (int m = MB; m < Bp; ++m) out[(long)m * N + n] = base;  // rows past the speaker rows (Bp > MB)
}

// rowmap (optional, device): encoder row b reads ids row rowmap[b] (the decode order)
void run_encoder(tts_ctx* c, const int64_t* ids, int B, int T_max, float* enc_out, hipStream_t s,
                 const int* rowmap = nullptr) {
  auto& M = c->taco;
  auto& W = c->tws;
  const int* lens = W.lens.i();
  launch_embed_gather(ids, T_max, M.emb.f(), M.num_chars, 512, lens, B, W.x0.f(), s, rowmap);
  const Layout x512 = bct(512, T_max);
  auto conv = [&](const ConvLayer& L, const float* in, Layout li, float* out, Layout lo, int epi) {
    ConvCall cc = conv_call(c, lens, B, T_max).in(in, li, 512).to(out, lo);
    cc.epi = epi;
    run_conv(L, cc, s);
  };
  conv(M.enc[0], W.x0.f(), btc(T_max, 512), W.ca.f(), x512, 1);
  conv(M.enc[1], W.ca.f(), x512, W.cb.f(), x512, 1);
  conv(M.enc[2], W.cb.f(), x512, W.ca.f(), x512, 1);
  // (B, T_max, 2048): time-major, so one step's gates of a tile are contiguous
  conv(M.lstm_in, W.ca.f(), x512, W.gin.f(), btc(T_max, 2048), 0);
  // one cooperative launch for the whole recurrence (W.lc then holds its grid-barrier words; its
  // fill zeroes enc_out too); per-step launches when cooperative launch is unavailable or
  // TTS_ENCODER=steps
  W.enc_ndom = sw::encoder_steps()
                   ? 0
                   : launch_bilstm_persist(W.gin.f(), M.whhT.f(), c->gemm_x3 ? M.whhT16.h() : nullptr, lens, T_max, B,
                                           W.lh.f(), reinterpret_cast<unsigned*>(W.lc.p), enc_out, s);
  W.enc_persist = W.enc_ndom > 0;
  if (!W.enc_persist) {
    HIP_OK(hipMemsetAsync(enc_out, 0, (size_t)B * T_max * 512 * 4, s));
    launch_bilstm(W.gin.f(), M.whhT.f(), lens, T_max, B, W.lh.f(), W.lc.f(), enc_out, s);
  }
}

// a persistent BiLSTM whose grid barrier timed out set its error word. The words are read on the
// library stream (ordered after the BiLSTM launch and its arm fill; c->s is non-blocking, so a
// null-stream copy would not be), then the stream is drained before they are looked at.
constexpr const char* ENC_BAR_MSG =
    "persistent BiLSTM: grid barrier timed out (workgroups not co-resident) or preempted past "
    "TTS_BARRIER_TIMEOUT_MS; retrying the call is safe)";
bool all_zero(const int* p, int n) {
  return std::all_of(p, p + n, [](int w) { return w == 0; });
}
void check_encoder_barrier(tts_ctx* c) {
  if (!c->tws.enc_persist) return;
  int* pw = c->pinned + PIN_ENC;  // one error word per recurrence (2 directions x up to 2 row groups)
  const int nd = std::min(c->tws.enc_ndom, ENC_NDOM_MAX);
  std::fill(pw, pw + ENC_NDOM_MAX, 0);
  const unsigned* words = reinterpret_cast<const unsigned*>(c->tws.lc.p);
  for (int i = 0; i < nd; ++i) HIP_OK(hipMemcpyAsync(&pw[i], words + i * BAR_WORDS + 16, 4, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipStreamSynchronize(c->s));
  TTS_CHECK(all_zero(pw, ENC_NDOM_MAX), ENC_BAR_MSG);
}

void run_postnet(tts_ctx* c, const float* dec, long dec_b, const int* mlens, int B, int Mmax_alloc, int max_q,
                 float* out, long out_b, hipStream_t s) {
  auto& M = c->taco;
  auto& W = c->tws;
  const Layout x512 = bct(512, Mmax_alloc), frames{dec_b, 1, 80};
  auto conv = [&](const ConvLayer& L, const float* in, Layout li, int Cin, float* o, Layout lo, int epi,
                  const float* resid) {
    ConvCall cc = conv_call(c, mlens, B, max_q).in(in, li, Cin).to(o, lo);
    if (resid) cc.add(resid, frames);
    cc.epi = epi;
    run_conv(L, cc, s);
  };
  conv(M.post[0], dec, frames, 80, W.pa.f(), x512, 2, nullptr);
  float* bufs[2] = {W.pa.f(), W.pbb.f()};
  for (int i = 1; i < 4; ++i) conv(M.post[i], bufs[(i - 1) & 1], x512, 512, bufs[i & 1], x512, 2, nullptr);
  conv(M.post[4], bufs[1], x512, 512, out, Layout{out_b, 1, 80}, 0, dec);
}

template <class T>
__global__ void gather_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ map,
                                   long row) {
  const long i = blockIdx.y;
  const T* sr = src + (long)map[i] * row;
  T* dr = dst + i * row;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < row; e += (long)gridDim.x * blockDim.x) dr[e] = sr[e];
}

// dst row i <- src row map[i], i < B
template <class T>
void gather_rows(const T* src, T* dst, const int* d_map, long row, int B, hipStream_t s) {
  if (row <= 0 || B <= 0) return;
  dim3 g((unsigned)std::min<long>((row + 255) / 256, 64), B);
  gather_rows_kernel<T><<<g, 256, 0, s>>>(src, dst, d_map, row);
  HIP_OK(hipGetLastError());
}

// the decoder's four outputs scattered back to the caller's row order in one launch (entry z)
struct Gather4 {
  const float* src[4];
  float* dst[4];
  long row[4];
};
__global__ void gather4_rows_kernel(Gather4 g, const int* __restrict__ map) {
  const int z = blockIdx.z;
  const long row = g.row[z], i = blockIdx.y;
  const float* __restrict__ sr = g.src[z] + (long)map[i] * row;
  float* __restrict__ dr = g.dst[z] + i * row;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < row; e += (long)gridDim.x * blockDim.x) dr[e] = sr[e];
}
void gather4_rows(const Gather4& g, const int* d_map, int B, hipStream_t s) {
  long mx = 0;
  for (int z = 0; z < 4; ++z) mx = std::max(mx, g.row[z]);
  if (mx <= 0 || B <= 0) return;
  gather4_rows_kernel<<<dim3((unsigned)std::min<long>((mx + 255) / 256, 64), B, 4), 256, 0, s>>>(g, d_map);
  HIP_OK(hipGetLastError());
}

// Per-call host arguments as kernel arguments (one launch instead of three pageable uploads):
// decode order and its inverse, lengths in decode order, and the decoder control block
// (DecCtlBlock: base = 0, all_done = 0, active_tiles = MT, done / steps / status = 0, max_steps)
struct TacoSetup {
  int B, MT;
  int perm[BMAX], inv[BMAX], lens[BMAX], max_steps[BMAX];
};
__global__ void taco_setup_kernel(TacoSetup a, int* map, int* lens, DecCtlBlock* cb, unsigned* zero_flag) {
  if (zero_flag && threadIdx.x == 0) *zero_flag = 0u;  // a fused call's range flag (no separate fill)
  if (threadIdx.x == 0) cb->ctl = DecCtl{0, 0, a.MT, 0};
  for (int b = threadIdx.x; b < BMAX; b += blockDim.x) {
    cb->done[b] = cb->steps[b] = cb->status[b] = 0;
    cb->max_steps[b] = b < a.B ? a.max_steps[b] : 0;
  }
  const int i = threadIdx.x;
  if (i < a.B) {
    map[i] = a.perm[i];
    map[BMAX + i] = a.inv[i];
    lens[i] = a.lens[i];
  }
}

// element (m, k) of a fragment-order activation; ps: published pre-split (decoder_persist.hip
// stc_quad_x3: the f16 hi / lo halves of k & ~3 .. + 3 as [hi 4 | lo 4] in their 16 bytes), read back
// as hi + 2^-11 lo, the value the decoder's split-f16 GEMMs consumed
__device__ __forceinline__ float frag_value(const float* p, int m, int k, int K, int ps) {
  if (!ps) return p[frag_idx(m, k, K)];
  const _Float16* q = reinterpret_cast<const _Float16*>(p + frag_idx(m, k & ~3, K));
  return (float)q[k & 3] + (float)q[4 + (k & 3)] * SPLIT_INV;
}

// decoder state in the caller's row order (tts_taco_decoder_state): fragment-order activations
// (h_att, h_dec, ctx) and row-major cells / attention rows of decode row inv[b] -> row b
__global__ void taco_state_kernel(const float* hatt, const float* catt, const float* hdec, const float* cdec,
                                  const float* ctx, const float* alpha, const float* acum, const int* inv, int T_max,
                                  int ps, float* o_ha, float* o_ca, float* o_hd, float* o_cd, float* o_ctx,
                                  float* o_al, float* o_ac) {
  const int b = blockIdx.y, m = inv[b];
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < 1024; k += gridDim.x * blockDim.x) {
    if (o_ha) o_ha[(long)b * 1024 + k] = frag_value(hatt, m, k, 1024, ps);
    if (o_ca) o_ca[(long)b * 1024 + k] = catt[(long)m * 1024 + k];
    if (o_hd) o_hd[(long)b * 1024 + k] = frag_value(hdec, m, k, 1024, ps);
    if (o_cd) o_cd[(long)b * 1024 + k] = cdec[(long)m * 1024 + k];
    if (o_ctx && k < 512) o_ctx[(long)b * 512 + k] = frag_value(ctx, m, k, 512, ps);
  }
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < T_max; k += gridDim.x * blockDim.x) {
    if (o_al) o_al[(long)b * T_max + k] = alpha[(long)m * T_max + k];
    if (o_ac) o_ac[(long)b * T_max + k] = acum[(long)m * T_max + k];
  }
}

// decode-order mel lengths for the postnet (steps * r), from the decoder results on the device
__global__ void taco_mlens_kernel(const DecCtlBlock* cb, int B, int r, int* mlens) {
  const int i = threadIdx.x;
  if (i < B) mlens[i] = cb->steps[i] * r;
}

// the output mask of a teacher-forced decode: frames [M_i, steps_i r) of decode row i zeroed (at most
// r - 1 frames: the padded part of the row's last group); one workgroup per row
__global__ void mask_frames_kernel(float* x, RowInts ml, const int* __restrict__ flens, int r, long row) {
  const int i = blockIdx.x;
  const int f0 = ml.v[i], f1 = min(flens[i], f0 + r);  // flens = steps * r <= S_cap r: inside the row
  float* p = x + i * row;
  for (int e = f0 * 80 + threadIdx.x; e < f1 * 80; e += blockDim.x) p[e] = 0.f;
}
void mask_frames(float* x, const RowInts& ml, const int* d_flens, int B, int r, long row, hipStream_t s) {
  mask_frames_kernel<<<B, 256, 0, s>>>(x, ml, d_flens, r, row);
  HIP_OK(hipGetLastError());
}

// gather every status word the host checks after a Tacotron2 call into one block (TS_* layout)
struct DecSlots {
  int v[PMAX_LAUNCH];
};
// A fused call (vlens set) also writes the vocoder's mel lengths in caller order, steps * r of
// decode row inv[b], raised to Lmin where shorter (TS_VERR: the call fails)
__global__ void taco_status_kernel(const unsigned* enc_bar, int nenc, const unsigned* dec_bar, DecSlots dslot, int ndec,
                                   const DecCtlBlock* cb, const unsigned* flag, int* st, int B, const int* inv,
                                   int r, int Lmin, int* vlens) {
  const int i = threadIdx.x;
  int short_row = 0;
  if (vlens && i < B) {
    int L = cb->steps[inv[i]] * r;
    if (L < Lmin) {
      short_row = 1;
      L = Lmin;
    }
    vlens[i] = L;
  }
  short_row = __syncthreads_or(short_row);
  if (i == 0) st[TS_VERR] = short_row;
  const int* res = cb->done;  // done | steps | status, contiguous (decoder.h)
  if (i < 3 * BMAX) st[TS_RES + i] = res[i];
  if (i < ENC_NDOM_MAX) st[TS_ENC + i] = enc_bar && i < nenc ? (int)enc_bar[i * BAR_WORDS + 16] : 0;
  if (i < PMAX_LAUNCH) {
    st[TS_DEC + i] = dec_bar && i < ndec ? (int)dec_bar[dslot.v[i] * BAR_WORDS + 16] : 0;
  }
  if (i == 0) st[TS_FLAG] = flag ? (int)*flag : 0;
}


bool use_persistent(tts_ctx* c) {
  if (sw::decoder_graph()) return false;
  return c->tws.MT <= PMAX_LAUNCH && persist_supported(c->device);
}

// the persistent decoder's arguments: weights, workspace and per-call scalars (no stream work)
PArgs persist_args(tts_ctx* c, int r, float thr) {
  auto& M = c->taco;
  auto& W = c->tws;
  PArgs a{};
  a.dec_w = M.dec_w.f();
  a.dec_b = M.dec_bias.f();
  a.apre_w = M.att_pre.f();
  a.apre_b = M.att_bias.f();
  a.attp_w = M.att_p.f();
  a.x3flag = x3_flag(c);  // null in fp32 mode
  // split-f16 decoder GEMM parts: only with every split weight set in range, and Q = 1024,
  // E = 512, prenet 256 (the kernel's fixed geometry, checked by build_pj's callers)
  const bool dx3 = a.x3flag && M.att_p_x3.p && M.dec_x3.p && M.apre_x3.p && M.pj_x3.p && !sw::decoder_f32();
  a.attp_x3 = dx3 ? M.att_p_x3.h() : nullptr;
  a.dec_x3 = dx3 ? M.dec_x3.h() : nullptr;
  a.apre_x3 = dx3 ? M.apre_x3.h() : nullptr;
  a.pj_x3 = dx3 ? M.pj_x3.h() : nullptr;
  a.pj_w = M.pj_w.f();
  a.pj_b = M.pj_b.f();
  // per-row biases in W.spkb (stage_row_biases): the projection's (always) behind the speaker
  // columns, which exist when the model has speakers
  const int YP = (1 + 5 * r + 16) * 16, pj0 = M.spk_dim ? 8320 : 0;
  a.spk_ld = pj0 + YP;
  // Graves with speakers: the projection columns hold W_s s alone; the kernel adds the bias and
  // scales W_s s by the step's sum of attention weights
  a.spk_scale = M.graves && M.spk_dim ? 1 : 0;
  a.pjb_rows = W.spkb.f() + pj0;
  a.spk_att = M.spk_dim ? W.spkb.f() : nullptr;
  a.spk_dec = M.spk_dim ? W.spkb.f() + 4096 : nullptr;
  a.spk_penc = M.spk_dim ? W.spkb.f() + 8192 : nullptr;
  // decoder variants
  a.pre1_b0 = M.prenet_bn ? M.pre1_b0.f() : nullptr;
  a.pre2_b = M.prenet_bn ? M.pre2_b.f() : nullptr;
  a.win = M.windowing;
  a.fwd = M.forward_attn;
  a.trans = M.forward_attn && M.trans_agent;
  a.fwd_mask = M.forward_attn && M.forward_attn_mask;
  a.ta_w = M.trans_agent ? M.ta_w.f() : nullptr;
  a.ta_b = M.ta_b;
  a.win_idx = W.win_idx.i();
  a.fwd_u = W.fwd_u.f();
  a.part_f = W.apf.f();
  a.gK = M.graves ? M.graves_K : 0;
  a.na1_w = M.na1_w.f();
  a.na1_b = M.na1_b.f();
  a.na2_w = M.na2_w.f();
  a.na2_b = M.na2_b.f();
  a.gh = W.gh.f();
  a.gmu = W.gmu.f();
  a.pre2_w = M.pre2.f();
  a.WqT = M.WqT.f();
  a.Wcomb = M.Wcomb.f();
  a.v = M.v.f();
  a.bv = M.bv;
  a.nt_proj = 1 + 5 * r;
  a.ntj = a.nt_proj + 16;
  a.r = r;
  a.penc = W.penc.f();
  a.enc = W.enc.f();
  a.ypart = W.ypart.f();
  a.pb = W.pb.f();
  a.gatt = W.gatt.f();
  a.hatt = W.hatt.f();
  a.catt = W.catt.f();
  a.hdec0 = W.hdec0.f();
  a.hdec1 = W.hdec1.f();
  a.cdec = W.cdec.f();
  a.ctx = W.ctx.f();
  a.pq = W.pq.f();
  a.alpha = W.alpha.f();
  a.acum = W.acum.f();
  a.energy = W.energy.f();
  a.part_s = W.aps.f();
  a.part_m = W.apm.f();
  a.part_u = W.apu.f();
  a.counter = reinterpret_cast<unsigned*>(W.acnt.p);
  a.nchmax = (W.T_max + persist_attn_tc() - 1) / persist_attn_tc();
  a.anorm = W.anorm.f();
  a.defer_align = persist_defer_ok(W.B * a.nchmax) && !sw::align_in_p4();
  a.softmax = M.softmax;
  a.thr = thr;
  a.bar = reinterpret_cast<unsigned*>(W.pbar.p);
  return a;
}

// the per-row biases the kernel reads through a.pjb_rows / a.spk_*: projection columns (always),
// speaker columns when the model has them
void stage_row_biases(tts_ctx* c, const PArgs& a, hipStream_t s) {
  auto& M = c->taco;
  auto& W = c->tws;
  const int N = a.spk_ld, pj0 = (int)(a.pjb_rows - W.spkb.f()), Bp = W.MT * 16;
  TTS_CHECK(W.B <= SPK_BMAX || !M.spk_dim, "multi-speaker decoding: at most 64 utterances per call");
  const int Bs = M.spk_dim ? W.B : 0;
  TTS_CHECK(M.spk_dim <= 1024, "conditioning vectors ([style | speaker]) of at most 1024 dims");
  const float* wt = M.spk_dim ? M.spk_wT.f() : nullptr;
  const int es = M.spk_dim, p0 = a.spk_scale ? N : pj0;
  const dim3 g((N + 63) / 64);
  if (Bs <= 16) spk_bias_kernel<16><<<g, 256, 0, s>>>(W.spk.f(), Bs, es, wt, N, M.pj_b.f(), p0, Bp, W.spkb.f());
  else if (Bs <= 32) spk_bias_kernel<32><<<g, 256, 0, s>>>(W.spk.f(), Bs, es, wt, N, M.pj_b.f(), p0, Bp, W.spkb.f());
  else spk_bias_kernel<64><<<g, 256, 0, s>>>(W.spk.f(), Bs, es, wt, N, M.pj_b.f(), p0, Bp, W.spkb.f());
  HIP_OK(hipGetLastError());
}

// state the decoder variants carry across steps, at its value before the first step
void reset_variant_state(tts_ctx* c, hipStream_t s) {
  auto& M = c->taco;
  auto& W = c->tws;
  if (M.windowing) HIP_OK(hipMemsetAsync(W.win_idx.p, 0xff, 64 * 4, s));  // -1: before the first step
  if (M.graves) HIP_OK(hipMemsetAsync(W.gmu.p, 0, 64 * 16 * 4, s));  // mu_prev = 0 (common_layers.py:143)
  if (M.forward_attn) {
    static const std::vector<float> half(64, 0.5f);  // u = 0.5 (common_layers.py:241)
    HIP_OK(hipMemcpyAsync(W.fwd_u.p, half.data(), 64 * 4, hipMemcpyHostToDevice, s));
  }
}

constexpr size_t PTRACE_WORDS = (size_t)8 * 24 * 256;
// TTS_PTRACE=<file>: the traced launch's phase timestamps, written out once it has run
void dump_ptrace(const char* file, const DevBuf& buf, hipStream_t s) {
  HIP_OK(hipStreamSynchronize(s));
  std::vector<unsigned long long> h(PTRACE_WORDS);
  HIP_OK(hipMemcpy(h.data(), buf.p, h.size() * 8, hipMemcpyDeviceToHost));
  if (FILE* fp = std::fopen(file, "wb")) {
    std::fwrite(h.data(), 8, h.size(), fp);
    std::fclose(fp);
  }
}

// TTS_DIAG_XCC: print each launch's workgroup -> XCD map and the hand-off addresses
void print_xdiag(tts_ctx* c, const PArgs& a, hipStream_t s) {
  auto& W = c->tws;
  HIP_OK(hipStreamSynchronize(s));
  std::vector<unsigned> h((size_t)PMAX_LAUNCH * 256);
  HIP_OK(hipMemcpy(h.data(), W.xdiag.p, h.size() * 4, hipMemcpyDeviceToHost));
  for (int li = 0; li < c->dec_nlaunch; ++li) {
    std::fprintf(stderr, "TTS_DIAG_XCC launch %d: wg0 xcc %u, wg0..15:", li, h[li * 256]);
    for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %u", h[li * 256 + k]);
    std::fprintf(stderr, "\n");
  }
  std::fprintf(stderr, "TTS_DIAG_XCC addresses: bar %p pq %p hatt %p ctx %p hdec0 %p pb %p\n", (void*)W.pbar.p,
               (void*)a.pq, (void*)a.hatt, (void*)a.ctx, (void*)a.hdec0, (void*)a.pb);
}

// one cooperative launch per batch-tile count, MT down to 1; each launch takes over where the last
// one's trailing tile finished
void launch_cascade(tts_ctx* c, PArgs a, hipStream_t s) {
  auto& W = c->tws;
  // TTS_PTRACE=<file>: phase timestamps of 8 steps from step TTS_PTRACE_T0 (default 100)
  const char* tr = sw::ptrace_file();
  TTS_CHECK(!tr || persist_trace_built(), "TTS_PTRACE needs a library built with -DTTS_PHASE_TRACE "
                                          "(tools/build_variants.sh trace -DTTS_PHASE_TRACE; TTSHIP_LIB=tools/var/lib_trace.so)");
  unsigned long long* trace_p = nullptr;
  if (tr) {
    W.trace.ensure(PTRACE_WORDS * 8);
    HIP_OK(hipMemsetAsync(W.trace.p, 0, PTRACE_WORDS * 8, s));
    trace_p = static_cast<unsigned long long*>(W.trace.p);
    a.trace_t0 = sw::ptrace_t0();
  }
  const int trace_li = sw::ptrace_launch();
  const bool xdiag = sw::diag_xcc();
  if (xdiag) W.xdiag.ensure((size_t)PMAX_LAUNCH * 256 * 4);
  c->dec_nlaunch = 0;
  c->dec_presplit = persist_presplit(a);
  for (int mt = W.MT; mt >= 1; --mt) {
    const int li = W.MT - mt;  // launch index: its barrier block (armed in taco_run's state fill)
    const bool traced = trace_p && li == trace_li;  // one launch is traced
    a.bar = reinterpret_cast<unsigned*>(W.pbar.p) + BAR_WORDS * W.pslot[li];
    a.base_out = W.stat.i() + TS_END + li;
    a.D = make_dev(c, std::min(W.B, 16 * mt));
    a.trace = traced ? trace_p : nullptr;
    a.atrace = traced ? trace_p + (size_t)8 * 16 * 256 : nullptr;
    a.diag = xdiag ? static_cast<unsigned*>(W.xdiag.p) + 256 * li : nullptr;
    // launch timing from the dispatches themselves: ev_dec[0] at the first launch's start, ev_dec[i + 1]
    // at launch i's end (event-record packets between the launches cost ~5 us of idle each)
    launch_persist_decoder(a, mt, s, false, li == 0 ? c->ev_dec[0] : nullptr, c->ev_dec[li + 1]);
    if (traced) dump_ptrace(tr, W.trace, s);
    c->dec_nlaunch++;
  }
  if (xdiag) print_xdiag(c, a, s);
}

// the whole decode on the persistent kernel (decoder_persist.hip)
// teach_steps > 0: teacher mode on W.teach (a teacher-forced call)
void run_persistent(tts_ctx* c, int r, float thr, hipStream_t s, int teach_steps = 0) {
  build_pj(c, r);
  grow<float>(c->tws.spkb, (size_t)64 * (8320 + 112 * 16), c->tws.gen);
  PArgs a = persist_args(c, r, thr);
  if (teach_steps > 0) {
    a.teach = c->tws.teach.f();
    a.teach_steps = teach_steps;
    a.teach_rows = c->tws.MT * 16;
  }
  stage_row_biases(c, a, s);
  reset_variant_state(c, s);
  launch_cascade(c, a, s);
}

// ---- the steps of taco_run, in call order ----

// returns the largest max_decoder_steps of the batch
int check_infer_args(const TacoModel& M, const int32_t* h_lens, int B, int T_max, int r, const int32_t* h_max_steps,
                     int S_cap) {
  TTS_CHECK(M.ready, "tacotron2 weights not finalized");
  TTS_CHECK(B >= 1 && B <= BMAX, "B must be in [1, 64]");
  TTS_CHECK(T_max >= 1 && T_max <= 4096, "T_max must be in [1, 4096]");
  TTS_CHECK(r >= 1 && r <= M.r_init, "r must be in [1, r_init]");
  int max_ms = 0;
  for (int b = 0; b < B; ++b) {
    TTS_CHECK(h_lens[b] >= 1 && h_lens[b] <= T_max, "lens out of range");
    TTS_CHECK(h_max_steps[b] >= 1, "max_decoder_steps must be >= 1");
    max_ms = std::max(max_ms, (int)h_max_steps[b]);
  }
  TTS_CHECK(S_cap >= max_ms, "S_cap < max(max_steps)");
  return max_ms;
}

// Decode order: longest expected first (max_decoder_steps, then text length), so the rows still
// decoding at the end sit in the first batch tiles and the step can shrink to fewer tiles.
// Every row is independent, so the order changes nothing but speed; outputs are scattered back.
// Returns the order (decode row i = caller row perm[i]) and launches TacoSetup.
std::vector<int> stage_decode_order(tts_ctx* c, const int32_t* h_lens, const int32_t* h_max_steps, int B,
                                    unsigned* zero_flag, hipStream_t s) {
  auto& W = c->tws;
  std::vector<int> perm(B);
  for (int b = 0; b < B; ++b) perm[b] = b;
  std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) {
    if (h_max_steps[x] != h_max_steps[y]) return h_max_steps[x] > h_max_steps[y];
    return h_lens[x] > h_lens[y];
  });
  // decode order, its inverse, lengths and the control block in one launch, as kernel arguments
  TacoSetup ta{};
  ta.B = B;
  ta.MT = W.MT;
  for (int i = 0; i < B; ++i) {
    ta.perm[i] = perm[i];
    ta.inv[perm[i]] = i;
    ta.lens[i] = h_lens[perm[i]];
    ta.max_steps[i] = h_max_steps[perm[i]];
  }
  taco_setup_kernel<<<1, 256, 0, s>>>(ta, W.map.i(), W.lens.i(), ctl_block(W), zero_flag);
  HIP_OK(hipGetLastError());
  return perm;
}

// GST models: decode row i's conditioning vector [style of caller row map[i] (zeros without one) | speaker i]
__global__ void gst_cond_kernel(const float* __restrict__ style, const int* __restrict__ map,
                                const float* __restrict__ spk, int G, int Es, float* __restrict__ out) {
  const int i = blockIdx.x;
  const float* st = style ? style + (long)map[i] * G : nullptr;
  for (int e = threadIdx.x; e < G + Es; e += blockDim.x)
    out[(long)i * (G + Es) + e] = e < G ? (st ? st[e] : 0.f) : spk[(long)i * Es + e - G];
}

// conditioning vectors in decode order: the speaker vectors (external embeddings, or rows of the
// learned table), behind the style vectors when the model has GST
void stage_speakers(tts_ctx* c, const int64_t* d_spk_ids, const float* d_spk_emb, const float* d_style, int B,
                    hipStream_t s) {
  auto& M = c->taco;
  auto& W = c->tws;
  TTS_CHECK(!d_style || M.gst_dim, "a style vector was given, but the model has no gst_layer");
  if (!M.spk_dim) return;
  if (M.gst_dim) grow<float>(W.spk_only, (size_t)64 * 1024, W.gen);
  float* spk_out = M.gst_dim ? W.spk_only.f() : W.spk.f();
  TTS_CHECK(d_spk_ids || d_spk_emb, "multi-speaker model: speaker ids or speaker embeddings are required");
  TTS_CHECK(use_persistent(c), "multi-speaker decoding runs on the persistent decoder only (<= 64 utterances "
                               "per call on a 256-CU device)");
  if (d_spk_emb) {
    gather_rows<float>(d_spk_emb, spk_out, W.map.i(), M.es, B, s);
  } else {
    TTS_CHECK(M.num_spk > 0, "model has no speaker_embedding table: pass speaker embeddings");
    gather_rows<int64_t>(d_spk_ids, reinterpret_cast<int64_t*>(W.spkid.p), W.map.i(), 1, B, s);
    launch_embed_gather(reinterpret_cast<const int64_t*>(W.spkid.p), 1, M.spk_table.f(), M.num_spk, M.es,
                        W.lens.i(), B, spk_out, s);
  }
  if (M.gst_dim) {
    gst_cond_kernel<<<B, 256, 0, s>>>(d_style, W.map.i(), spk_out, M.gst_dim, M.es, W.spk.f());
    HIP_OK(hipGetLastError());
  }
}

// encoder (rows in decode order) + processed inputs
void run_encoder_penc(tts_ctx* c, const int64_t* ids, int B, int T_max, hipStream_t s) {
  auto& W = c->tws;
  run_encoder(c, ids, B, T_max, W.enc.f(), s, W.map.i());
  run_conv(c->taco.penc,
           conv_call(c, W.lens.i(), B, T_max).in(W.enc.f(), btc(T_max, 512), 512).to(W.penc.f(), btc(T_max, 128)), s);
}

// decoder state and outputs zeroed in one launch (the postnet output too, and the persistent
// launches' barrier blocks), attention_rnn gate biases broadcast
void fill_decoder_state(tts_ctx* c, int B, int T_max, int S_cap, int r, bool persist, hipStream_t s) {
  auto& M = c->taco;
  auto& W = c->tws;
  const int Bp = W.MT * 16;
  FillList f;
  for (const DevBuf* b : {&W.catt, &W.hatt, &W.hdec0, &W.hdec1, &W.cdec}) f.add(b->p, (size_t)Bp * 1024 * 4);
  f.add(W.ctx.p, (size_t)Bp * 512 * 4);
  f.add(W.y.p, (size_t)Bp * 80 * M.r_init * 4);
  f.add(W.alpha.p, (size_t)B * T_max * 4);
  f.add(W.acum.p, (size_t)B * T_max * 4);
  f.add(W.dec.p, (size_t)B * S_cap * r * 80 * 4);
  f.add(W.align.p, (size_t)B * S_cap * T_max * 4);
  f.add(W.stop.p, (size_t)B * S_cap * 4);
  f.add(W.acnt.p, BMAX * sizeof(unsigned));
  f.add(W.post.p, (size_t)B * S_cap * r * 80 * 4);
  if (persist)
    for (int li = 0; li < W.MT; ++li) add_barrier_fills(f, reinterpret_cast<unsigned*>(W.pbar.p) + BAR_WORDS * W.pslot[li], 1);
  launch_fills(f, s);
  bcast_rows_kernel<<<256, 256, 0, s>>>(M.att_bias.f(), 4096, W.gatt.f(), Bp);
  HIP_OK(hipGetLastError());
}


// postnet over each row's own frames: lengths from the decoder results on the device, grid sized
// by S_cap (tiles past a row's length exit at entry), so the decode needs no host round trip; then
// the scatter back to the caller's row order: output row b <- decode row inv[b]
// ml (a teacher-forced call): the rows' mel lengths M_i in decode order; the decoder outputs are zeroed at
// frames >= M_i before the postnet, its output after it (the reference's output mask,
// models/tacotron2.py:123-130)
void run_postnet_scatter(tts_ctx* c, int B, int T_max, int S_cap, int r, float* d_dec, float* d_post, float* d_align,
                         float* d_stop, hipStream_t s, const RowInts* ml = nullptr) {
  auto& W = c->tws;
  taco_mlens_kernel<<<1, 64, 0, s>>>(ctl_block(W), B, r, W.mlens.i());
  HIP_OK(hipGetLastError());
  const long fb = (long)S_cap * r * 80;  // W.post was zeroed with the decoder state
  if (ml) mask_frames(W.dec.f(), *ml, W.mlens.i(), B, r, fb, s);
  run_postnet(c, W.dec.f(), fb, W.mlens.i(), B, S_cap * r, S_cap * r, W.post.f(), fb, s);
  if (ml) mask_frames(W.post.f(), *ml, W.mlens.i(), B, r, fb, s);
  gather4_rows(Gather4{{W.post.f(), W.dec.f(), W.align.f(), W.stop.f()}, {d_post, d_dec, d_align, d_stop},
                       {fb, fb, (long)S_cap * T_max, (long)S_cap}},
               W.map.i() + BMAX, B, s);
}

// one host round trip per call: barrier error words, per-row results, range flag, launch steps
// gathered by one kernel and copied to the pinned page; a fused call's vocoder goes in behind the
// copy, and the host waits for the words only
void read_status(tts_ctx* c, int B, int r, bool persist, const FusedVoc* fv, hipStream_t s) {
  auto& W = c->tws;
  const unsigned* lc = reinterpret_cast<const unsigned*>(W.lc.p);
  DecSlots ds;
  std::copy(W.pslot, W.pslot + PMAX_LAUNCH, ds.v);
  taco_status_kernel<<<1, 256, 0, s>>>(W.enc_persist ? lc : nullptr, W.enc_ndom,
                                       persist ? reinterpret_cast<const unsigned*>(W.pbar.p) : nullptr, ds,
                                       c->dec_nlaunch, ctl_block(W), c->gemm_x3 ? x3_flag(c) : nullptr, W.stat.i(), B,
                                       W.map.i() + BMAX, r, fv ? fv->Lmin : 0, fv ? fv->vlens : nullptr);
  HIP_OK(hipGetLastError());
  int* pin = c->pinned;
  HIP_OK(hipMemcpyAsync(pin + TS_ENC, W.stat.i() + TS_ENC, (TS_N - TS_ENC) * 4, hipMemcpyDeviceToHost, s));
  if (fv) {
    HIP_OK(hipEventRecord(c->ev_status, s));
    fv->enqueue();
    HIP_OK(hipEventSynchronize(c->ev_status));
  } else {
    HIP_OK(hipStreamSynchronize(s));
  }
  TTS_CHECK(!W.enc_persist || all_zero(pin + TS_ENC, ENC_NDOM_MAX), ENC_BAR_MSG);
  TTS_CHECK(!persist || all_zero(pin + TS_DEC, PMAX_LAUNCH),
            "persistent decoder: grid barrier timed out (workgroups not co-resident) or preempted past "
            "TTS_BARRIER_TIMEOUT_MS; retrying the call is safe)");
  if (c->gemm_x3) {  // with_x3_fallback reads the flag from here
    pin[PIN_FLAG] = pin[TS_FLAG];
    c->flag_read = true;
  }
  for (int i = 0; i < PMAX_LAUNCH; ++i) c->dec_end[i] = persist && i < c->dec_nlaunch ? pin[TS_END + i] : 0;
  TTS_CHECK(!fv || pin[TS_VERR] == 0, VOC_SHORT_MSG);
}

// the rows' steps and status from the status words (decode order) to the caller's order
void report_rows(tts_ctx* c, const std::vector<int>& perm, int32_t* h_steps, int32_t* h_status) {
  const int* res = c->pinned + TS_RES;
  for (size_t i = 0; i < perm.size(); ++i) {
    TTS_CHECK(res[i] == 1, "decoder did not finish an utterance (internal error)");
    const int b = perm[i];
    h_steps[b] = res[BMAX + i];
    h_status[b] = res[2 * BMAX + i];
  }
}

}  // namespace

// One Tacotron2 call, free-running or teacher-forced (k.teach set: Tacotron2.forward in eval). The
// teacher-forced decode is the same sequence with the prenet fed from the ground-truth mel
// (teacher_prenet.hip + the persistent decoder's teacher variant), exactly S_i = ceil(M_i / r) steps
// per row, raw stop logits, and the reference's output mask.
void ttsh::taco_run(tts_ctx* c, const TacoCall& k) {
  auto& M = c->taco;
  const TacoTeach* t = k.teach;
  const int B = k.B, T_max = k.T_max, r = k.r;
  const FusedVoc* fv = t ? nullptr : k.run.fv;
  const int32_t* h_max_steps = k.run.h_max_steps;
  int S_cap = k.run.S_cap;
  int32_t tsteps[BMAX], rsteps[BMAX], rstatus[BMAX];
  if (t) {  // the step counts come from the mel lengths
    TTS_CHECK(M.ready, "tacotron2 weights not finalized");
    TTS_CHECK(t->M_max >= 1 && t->M_max <= (1 << 20) && r >= 1 && t->M_max % r == 0,
              "M_max must be a positive multiple of r");
    TTS_CHECK(!M.windowing && !M.forward_attn && !M.graves,
              "teacher-forced forward: attention windowing, forward attention and Graves attention are not implemented");
    TTS_CHECK(B >= 1 && B <= BMAX, "B must be in [1, 64]");
    for (int b = 0; b < B; ++b) {
      TTS_CHECK(t->h_mel_lens[b] >= 1 && t->h_mel_lens[b] <= t->M_max, "mel lens out of range");
      tsteps[b] = (t->h_mel_lens[b] + r - 1) / r;
    }
    h_max_steps = tsteps;
    S_cap = t->M_max / r;
  }
  const int max_ms = check_infer_args(M, k.h_lens, B, T_max, r, h_max_steps, S_cap);
  taco_workspace(c, B, T_max, S_cap, r);
  auto& W = c->tws;
  if (t) grow<float>(W.teach, (size_t)S_cap * W.MT * 16 * 256, W.gen);
  hipStream_t s = c->s;
  enter(c, k.stream, /*join_voc=*/!fv);  // a fused submission's decode does not wait for earlier vocoders
  // a fused call's range flag is zeroed by the setup launch (no separate fill)
  const std::vector<int> perm = stage_decode_order(c, k.h_lens, h_max_steps, B, fv ? x3_flag(c) : nullptr, s);
  W.thr = t ? 0.5f : k.run.thr;  // teacher-forced: unused, a row never stops by its stop token
  const bool persist = use_persistent(c);
  TTS_CHECK(!t || persist, "teacher-forced forward runs on the persistent decoder only (<= 64 utterances per "
                           "call on a 256-CU device, TTS_DECODER=graph unset)");
  TTS_CHECK(!M.variant() || persist, "BN prenet / attention windowing / forward / Graves attention run on "
                                     "the persistent decoder only (<= 64 utterances per call on a 256-CU "
                                     "device)");
  stage_speakers(c, k.d_spk_ids, k.d_spk_emb, k.d_style, B, s);
  run_encoder_penc(c, k.ids, B, T_max, s);
  if (persist && !W.pslot_cal) {  // ordered after the caller's work (enter above) and this call's encoder
    pick_barrier_blocks(reinterpret_cast<unsigned*>(W.pbar.p), PBAR_CAND, PMAX_LAUNCH, W.pslot, s);
    W.pslot_cal = true;
  }
  fill_decoder_state(c, B, T_max, S_cap, r, persist, s);
  RowInts ml{};  // teacher-forced: the output mask's lengths, decode order
  if (t) {  // prenet layer 1 of every ground-truth frame the decoder will be fed, into W.teach
    TeachArgs ta{};
    ta.mel = t->d_mel;
    ta.mel_b = (long)t->M_max * 80;
    ta.map = W.map.i();
    ta.max_steps = ctl_block(W)->max_steps;
    ta.W1 = M.pre1.f();
    ta.b1 = M.prenet_bn ? M.pre1_b0.f() : nullptr;
    ta.teach = W.teach.f();
    ta.B = B;
    ta.Bp = W.MT * 16;
    ta.r = r;
    ta.steps = S_cap;
    launch_teacher_prenet(ta, s);
    for (int i = 0; i < B; ++i) ml.v[i] = t->h_mel_lens[perm[i]];
  }
  c->dec_path = persist ? 1 : 0;
  if (persist) run_persistent(c, r, W.thr, s, t ? S_cap : 0);
  else run_graph_decoder(c, B, T_max, S_cap, r, W.thr, max_ms, s);
  run_postnet_scatter(c, B, T_max, S_cap, r, k.d_dec, k.d_post, k.d_align, k.d_stop, s, t ? &ml : nullptr);
  read_status(c, B, r, persist, fv, s);
  report_rows(c, perm, t ? rsteps : k.run.h_steps, t ? rstatus : k.run.h_status);
  for (int b = 0; t && b < B; ++b)
    TTS_CHECK(rsteps[b] == tsteps[b], "teacher-forced decode: a row's step count (internal error)");
  if (fv)  // the caller's stream waits for the decode's outputs here, for the vocoder at finish
    HIP_OK(hipStreamWaitEvent((hipStream_t)k.stream, c->ev_status, 0));
  else
    leave(c, k.stream);
  c->last_B = B;
  c->last_T = T_max;
  c->last_S = S_cap;
  c->last_r = r;
}

extern "C" {

int tts_taco_forward(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                     const float* d_mel, const int32_t* h_mel_lens, int M_max, const int64_t* d_spk_ids,
                     const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                     void* stream) {
  return tts_taco_forward_style(c, d_ids, h_lens, B, T_max, r, d_mel, h_mel_lens, M_max, d_spk_ids, d_spk_emb, nullptr,
                                d_dec, d_post, d_align, d_stop, stream);
}

int tts_taco_forward_style(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                           const float* d_mel, const int32_t* h_mel_lens, int M_max, const int64_t* d_spk_ids,
                           const float* d_spk_emb, const float* d_style, float* d_dec, float* d_post, float* d_align,
                           float* d_stop, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && d_ids && h_lens && d_mel && h_mel_lens && d_dec && d_post && d_align && d_stop, "null argument");
    DeviceGuard g(c->device);
    const TacoTeach teach{d_mel, h_mel_lens, M_max};
    TacoCall k;
    k.ids = d_ids, k.h_lens = h_lens, k.B = B, k.T_max = T_max, k.r = r, k.stream = stream;
    k.d_spk_ids = d_spk_ids, k.d_spk_emb = d_spk_emb, k.d_style = d_style;
    k.d_dec = d_dec, k.d_post = d_post, k.d_align = d_align, k.d_stop = d_stop;
    k.teach = &teach;
    with_x3_fallback(c, [&] { taco_run(c, k); });
  });
}

int tts_taco_infer(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                   const int32_t* h_max_steps, int S_cap, float thr, float* d_dec, float* d_post, float* d_align,
                   float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream) {
  return tts_taco_infer_spk(c, d_ids, h_lens, B, T_max, r, h_max_steps, S_cap, thr, nullptr, nullptr, d_dec, d_post,
                            d_align, d_stop, h_steps, h_status, stream);
}

int tts_taco_infer_spk(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                       const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                       const float* d_spk_emb, float* d_dec, float* d_post, float* d_align, float* d_stop,
                       int32_t* h_steps, int32_t* h_status, void* stream) {
  return tts_taco_infer_style(c, d_ids, h_lens, B, T_max, r, h_max_steps, S_cap, thr, d_spk_ids, d_spk_emb, nullptr,
                              d_dec, d_post, d_align, d_stop, h_steps, h_status, stream);
}

int tts_taco_infer_style(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, int r,
                         const int32_t* h_max_steps, int S_cap, float thr, const int64_t* d_spk_ids,
                         const float* d_spk_emb, const float* d_style, float* d_dec, float* d_post, float* d_align,
                         float* d_stop, int32_t* h_steps, int32_t* h_status, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && d_ids && h_lens && h_max_steps && d_dec && d_post && d_align && d_stop && h_steps && h_status,
              "null argument");
    DeviceGuard g(c->device);
    TacoCall k;
    k.ids = d_ids, k.h_lens = h_lens, k.B = B, k.T_max = T_max, k.r = r, k.stream = stream;
    k.d_spk_ids = d_spk_ids, k.d_spk_emb = d_spk_emb, k.d_style = d_style;
    k.d_dec = d_dec, k.d_post = d_post, k.d_align = d_align, k.d_stop = d_stop;
    k.run = TacoFree{h_max_steps, S_cap, thr, h_steps, h_status};
    with_x3_fallback(c, [&] { taco_run(c, k); });
  });
}

int tts_taco_encoder(tts_ctx* c, const int64_t* d_ids, const int32_t* h_lens, int B, int T_max, float* d_out,
                     void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && d_ids && h_lens && d_out, "null argument");
    TTS_CHECK(c->taco.ready, "tacotron2 weights not finalized");
    TTS_CHECK(B >= 1 && B <= BMAX && T_max >= 1, "bad sizes");
    check_rows(h_lens, B, 1, T_max, "lens out of range");
    DeviceGuard g(c->device);
    taco_workspace(c, B, T_max, std::max(1, c->tws.S_cap), std::max(1, c->tws.r));
    enter(c, stream);
    put_rows(c->tws.lens, h_lens, B, c->s);
    with_x3_fallback(c, [&] { run_encoder(c, d_ids, B, T_max, d_out, c->s); });
    check_encoder_barrier(c);
    leave(c, stream);
  });
}

int tts_taco_postnet(tts_ctx* c, const float* d_dec, const int32_t* h_lens, int B, int M_max, float* d_out,
                     void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && d_dec && h_lens && d_out, "null argument");
    TTS_CHECK(c->taco.ready, "tacotron2 weights not finalized");
    TTS_CHECK(B >= 1 && B <= BMAX && M_max >= 1, "bad sizes");
    DeviceGuard g(c->device);
    auto& W = c->tws;
    long gen = W.gen;
    grow<int>(W.mlens, BMAX, gen);
    grow<float>(W.pa, (size_t)B * 512 * M_max, gen);
    grow<float>(W.pbb, (size_t)B * 512 * M_max, gen);
    W.gen = gen;
    check_rows(h_lens, B, 1, M_max, "lens out of range");
    const int maxM = *std::max_element(h_lens, h_lens + B);
    enter(c, stream);
    put_rows(W.mlens, h_lens, B, c->s);
    HIP_OK(hipMemsetAsync(d_out, 0, (size_t)B * M_max * 80 * 4, c->s));
    with_x3_fallback(c, [&] {
      run_postnet(c, d_dec, (long)M_max * 80, W.mlens.i(), B, M_max, maxM, d_out, (long)M_max * 80, c->s);
    });
    HIP_OK(hipStreamSynchronize(c->s));
    leave(c, stream);
  });
}

int tts_taco_decoder_state(tts_ctx* c, int B, int T_max, float* d_att_h, float* d_att_c, float* d_dec_h,
                           float* d_dec_c, float* d_context, float* d_alpha, float* d_alpha_cum, void* stream) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c->last_B > 0, "run tts_taco_infer first");
    TTS_CHECK(B == c->last_B && T_max == c->last_T,
              "decoder state: the buffers' (B, T_max) differ from the last decode on this context");
    TTS_CHECK(c->dec_path == 1 && c->dec_nlaunch >= 1, "decoder state: the last decode did not run the persistent "
                                                       "decoder (TTS_DECODER=graph or a non-256-CU device)");
    DeviceGuard g(c->device);
    auto& W = c->tws;
    // the last executed step t_end - 1 wrote h_dec into hdec[(t_end - 1) & 1 ? 0 : 1]
    // (decoder_persist.hip P5: hd_nxt = (t & 1) ? hdec0 : hdec1)
    const int t_end = c->dec_end[c->dec_nlaunch - 1];
    TTS_CHECK(t_end >= 1, "decoder state: no decoder step ran");
    const float* hdec = ((t_end - 1) & 1) ? W.hdec0.f() : W.hdec1.f();
    enter(c, stream);
    taco_state_kernel<<<dim3(4, c->last_B), 256, 0, c->s>>>(W.hatt.f(), W.catt.f(), hdec, W.cdec.f(), W.ctx.f(),
                                                            W.alpha.f(), W.acum.f(), W.map.i() + BMAX, c->last_T,
                                                            c->dec_presplit ? 1 : 0, d_att_h, d_att_c, d_dec_h, d_dec_c, d_context, d_alpha,
                                                            d_alpha_cum);
    HIP_OK(hipGetLastError());
    leave(c, stream);
  });
}

int tts_decoder_stats(tts_ctx* c, int* path, int* nlaunch, float* ms, int* steps) {
  return guarded_ctx(c, [&] {
    TTS_CHECK(c && path && nlaunch && ms && steps, "bad arguments");
    TTS_CHECK(c->last_B > 0, "run tts_taco_infer first");
    *path = c->dec_path;
    *nlaunch = c->dec_path ? c->dec_nlaunch : 0;
    int prev = 0;
    for (int i = 0; i < *nlaunch; ++i) {
      HIP_OK(hipEventElapsedTime(&ms[i], c->ev_dec[i], c->ev_dec[i + 1]));
      steps[i] = c->dec_end[i] - prev;
      prev = c->dec_end[i];
    }
  });
}


}  // extern "C"
