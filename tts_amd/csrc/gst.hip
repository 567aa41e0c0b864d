// Global Style Tokens (TTS/tts/layers/gst_layers.py): the style vector a multi-speaker Tacotron2
// concatenates to its encoder outputs, from a mel spectrogram or from token weights.
//
//   reference encoder   6 x [Conv2d 3x3, stride 2, pad 1 -> BatchNorm2d (eval) -> ReLU] over the
//                       (frames, 80 mel bins) image, channels 1-32-32-64-64-128-128, then a GRU over
//                       the remaining ceil(N / 64) columns of 128 x 2 features; its last hidden state
//   style-token layer   multi-head attention of [hidden state | speaker embedding] over the
//                       tanh(token) keys; keys and values are tables built at load
//
// Arithmetic is plain fp32 FMA with one fixed summation order per output element,
// so a row's style vector does not depend on the batch it sits in. Every sum of more than a few
// terms runs as 4 interleaved chains (k mod 4) added as (c0 + c1) + (c2 + c3): a quarter of the
// rounding-error growth of one chain at no cost.
//
// Activations are channel-last, (B, W_max, H, C). Row b is bounded by its own width at every layer
// (W_0 = N_b, W_l = ceil(W_{l-1} / 2)): the zero padding sits at the row's own edge, nothing past
// it is read, and nothing past it is written.
#include "common.h"
#include "launch.h"

namespace {

__device__ __forceinline__ int gst_width(int n, int halvings) {
  for (int i = 0; i < halvings; ++i) n = (n + 1) >> 1;
  return n;
}

__device__ __forceinline__ float sum4(const float* a) { return (a[0] + a[1]) + (a[2] + a[3]); }

// Layer `layer` (0-based): in (B, Wi_max, Hi, CIN) -> out (B, Wo_max, Ho, COUT), BatchNorm and bias
// folded into W [kt][kh][ci][co] and bias. Workgroup = 256 / COUT position groups x COUT channels;
// a group computes P = 4 consecutive positions p = t Ho + h of its row for every channel, so each
// weight is loaded once per 4 FMAs and the inputs as float4 over ci (the same address in all lanes
// of a group). Per output element the sum runs over (kt, kh, ci) ascending, ci in 4 chains.
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void gst_conv_kernel(const float* __restrict__ in, long in_b, int Wi_max, int Hi,
                                                       RowInts lens, int layer, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       long out_b, int Ho) {
  constexpr int P = 4, NG = 256 / COUT, Q = CIN == 1 ? 1 : 4;
  const int b = blockIdx.y;
  const int wi = gst_width(lens.v[b], layer), wo = (wi + 1) >> 1;
  const int npos = wo * Ho;
  if ((int)blockIdx.x * NG * P >= npos) return;
  const int co = threadIdx.x % COUT, g = threadIdx.x / COUT;
  const int p0 = (blockIdx.x * NG + g) * P;
  const float* inb = in + b * in_b;
  int t[P], h[P];
  float acc[P][Q];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int p = p0 + j;
    t[j] = p < npos ? p / Ho : -4;  // a position past the row: every tap falls outside
    h[j] = p - (p / Ho) * Ho;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[j][q] = 0.f;
  }
  for (int kt = 0; kt < 3; ++kt) {
    for (int kh = 0; kh < 3; ++kh) {
      const float* xp[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int ti = 2 * t[j] + kt - 1, hi = 2 * h[j] + kh - 1;
        const bool ok = ti >= 0 && ti < wi && hi >= 0 && hi < Hi;  // wi <= Wi_max: inside the buffer
        xp[j] = ok ? inb + ((long)ti * Hi + hi) * CIN : nullptr;
      }
      const float* wp = W + (long)(kt * 3 + kh) * CIN * COUT + co;
      if constexpr (CIN == 1) {
        const float w = wp[0];
#pragma unroll
        for (int j = 0; j < P; ++j) acc[j][0] = fmaf(xp[j] ? xp[j][0] : 0.f, w, acc[j][0]);
      } else {
#pragma unroll 2
        for (int ci = 0; ci < CIN; ci += 4) {
          float w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) w[q] = wp[(long)(ci + q) * COUT];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float4 x = xp[j] ? *reinterpret_cast<const float4*>(xp[j] + ci) : float4{0.f, 0.f, 0.f, 0.f};
            acc[j][0] = fmaf(x.x, w[0], acc[j][0]);
            acc[j][1] = fmaf(x.y, w[1], acc[j][1]);
            acc[j][2] = fmaf(x.z, w[2], acc[j][2]);
            acc[j][3] = fmaf(x.w, w[3], acc[j][3]);
          }
        }
      }
    }
  }
  const float bs = bias[co];
  float* ob = out + b * out_b;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (p0 + j >= npos) continue;
    const float v = (Q == 1 ? acc[j][0] : sum4(acc[j])) + bs;
    ob[(long)(p0 + j) * COUT + co] = fmaxf(v, 0.f);
  }
}

template <int CIN, int COUT>
void conv_layer(const float* in, long in_b, int Wi_max, int Hi, const RowInts& lens, int layer, const float* W,
                const float* bias, float* out, int B, hipStream_t s) {
  const int Wo_max = (Wi_max + 1) / 2, Ho = (Hi + 1) / 2;
  const int per_block = (256 / COUT) * 4;
  const dim3 grid((unsigned)((Wo_max * Ho + per_block - 1) / per_block), B);
  gst_conv_kernel<CIN, COUT><<<grid, 256, 0, s>>>(in, in_b, Wi_max, Hi, lens, layer, W, bias, out,
                                                  (long)Wo_max * Ho * COUT, Ho);
  HIP_OK(hipGetLastError());
}

// One workgroup per row: the GRU over the row's own ceil(N_b / 64) steps (thread u < Hg owns hidden
// unit u: its three gates' input and hidden sums, weights transposed so that adjacent threads read
// adjacent columns), then the query projection, the scores of every (head, token), the softmax per
// head and the weighted values. PyTorch's cell: r, z = sigmoid, n = tanh(gi_n + r gh_n),
// h' = (h - n) z + n. expf / tanhf are the library forms (the fast forms' 2e-7 is the size of the
// tolerance here).
__global__ __launch_bounds__(256) void gst_head_kernel(GstHeadArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[256];
  __shared__ __attribute__((aligned(16))) float qin[GST_HG_MAX + GST_ES_MAX];
  __shared__ float q[GST_G_MAX];
  __shared__ float sc[GST_HEADS_MAX * GST_TOK_MAX];
  const int b = blockIdx.x, u = threadIdx.x;
  const int Hg = a.Hg, G3 = 3 * a.Hg;
  const int steps = gst_width(a.lens.v[b], 6);
  for (int k = u; k < Hg; k += 256) qin[k] = 0.f;  // h_0 = 0
  float hprev = 0.f;
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    xs[u] = a.x[b * a.xb + (long)t * 256 + u];
    __syncthreads();
    float hn = 0.f;
    if (u < Hg) {
      float ir[4] = {0.f, 0.f, 0.f, 0.f}, iz[4] = {0.f, 0.f, 0.f, 0.f}, in_[4] = {0.f, 0.f, 0.f, 0.f};
      const float* w = a.wihT + u;
      for (int k = 0; k < 256; k += 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float x = xs[k + c];
          const float* wk = w + (long)(k + c) * G3;
          ir[c] = fmaf(x, wk[0], ir[c]);
          iz[c] = fmaf(x, wk[Hg], iz[c]);
          in_[c] = fmaf(x, wk[2 * Hg], in_[c]);
        }
      }
      float hr[4] = {0.f, 0.f, 0.f, 0.f}, hz[4] = {0.f, 0.f, 0.f, 0.f}, hh[4] = {0.f, 0.f, 0.f, 0.f};
      w = a.whhT + u;
      for (int k = 0; k < Hg; k += 4) {  // Hg is a multiple of 4 (host check)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float x = qin[k + c];
          const float* wk = w + (long)(k + c) * G3;
          hr[c] = fmaf(x, wk[0], hr[c]);
          hz[c] = fmaf(x, wk[Hg], hz[c]);
          hh[c] = fmaf(x, wk[2 * Hg], hh[c]);
        }
      }
      const float gr = (sum4(ir) + a.bih[u]) + (sum4(hr) + a.bhh[u]);
      const float gz = (sum4(iz) + a.bih[Hg + u]) + (sum4(hz) + a.bhh[Hg + u]);
      const float r = 1.f / (1.f + expf(-gr)), z = 1.f / (1.f + expf(-gz));
      const float n = tanhf((sum4(in_) + a.bih[2 * Hg + u]) + r * (sum4(hh) + a.bhh[2 * Hg + u]));
      hn = (hprev - n) * z + n;
    }
    __syncthreads();  // every thread has read the old state
    if (u < Hg) {
      hprev = hn;
      qin[u] = hn;
    }
    __syncthreads();
  }
  // query = W_query [h | speaker embedding]
  const int Kq = Hg + a.Es;
  for (int k = u; k < a.Es; k += 256) qin[Hg + k] = a.spk[(long)b * a.Es + k];
  __syncthreads();
  for (int j = u; j < a.G; j += 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* w = a.wqT + j;
    for (int k = 0; k < Kq; k += 4) {  // Kq is a multiple of 4 (host check)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = fmaf(qin[k + c], w[(long)(k + c) * a.G], acc[c]);
    }
    q[j] = sum4(acc);
  }
  __syncthreads();
  const int dk = a.G / a.heads;
  if (u < a.heads * a.ntok) {
    const int hd = u / a.ntok, k = u - hd * a.ntok;
    const float* kr = a.Kt + (long)k * a.G + hd * dk;
    const float* qr = q + hd * dk;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < dk; d += 4) {  // dk is a multiple of 4 (host check)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = fmaf(qr[d + c], kr[d + c], acc[c]);
    }
    sc[u] = sum4(acc) / a.scale;
  }
  __syncthreads();
  if (u < a.heads) {  // softmax over the tokens of head u, in token order
    float* s = sc + u * a.ntok;
    float m = s[0];
    for (int k = 1; k < a.ntok; ++k) m = fmaxf(m, s[k]);
    float sum = 0.f;
    for (int k = 0; k < a.ntok; ++k) {
      s[k] = expf(s[k] - m);
      sum += s[k];
    }
    for (int k = 0; k < a.ntok; ++k) s[k] = s[k] / sum;
  }
  __syncthreads();
  for (int j = u; j < a.G; j += 256) {
    const float* s = sc + (j / dk) * a.ntok;
    float acc = 0.f;
    for (int k = 0; k < a.ntok; ++k) acc = fmaf(s[k], a.Vt[(long)k * a.G + j], acc);
    a.out[(long)b * a.G + j] = acc;
  }
}

// sum_i w_i V[id_i], in the order given; each term rounded before it is added, as the reference's
// gst_outputs + attention(query, key) * amplifier
__global__ void gst_tokens_kernel(GstTokenArgs a, const float* __restrict__ Vt, int G, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= G) return;
  float acc = 0.f;
  for (int i = 0; i < a.n; ++i) acc = __fadd_rn(acc, __fmul_rn(Vt[(long)a.id[i] * G + j], a.w[i]));
  out[j] = acc;
}

}  // namespace

void launch_gst_convs(const float* mel, const RowInts& lens, int B, int N_max, const float* const* W,
                      const float* const* bias, float* bufA, float* bufB, hipStream_t s) {
  TTS_CHECK(B >= 1 && B <= 64 && N_max >= 1, "gst convs: sizes");
  int w = N_max;
  conv_layer<1, 32>(mel, (long)N_max * 80, w, 80, lens, 0, W[0], bias[0], bufA, B, s);
  w = (w + 1) / 2;
  conv_layer<32, 32>(bufA, (long)w * 40 * 32, w, 40, lens, 1, W[1], bias[1], bufB, B, s);
  w = (w + 1) / 2;
  conv_layer<32, 64>(bufB, (long)w * 20 * 32, w, 20, lens, 2, W[2], bias[2], bufA, B, s);
  w = (w + 1) / 2;
  conv_layer<64, 64>(bufA, (long)w * 10 * 64, w, 10, lens, 3, W[3], bias[3], bufB, B, s);
  w = (w + 1) / 2;
  conv_layer<64, 128>(bufB, (long)w * 5 * 64, w, 5, lens, 4, W[4], bias[4], bufA, B, s);
  w = (w + 1) / 2;
  conv_layer<128, 128>(bufA, (long)w * 3 * 128, w, 3, lens, 5, W[5], bias[5], bufB, B, s);
}

void launch_gst_head(const GstHeadArgs& a, int B, hipStream_t s) {
  TTS_CHECK(B >= 1 && B <= 64, "gst head: B");
  TTS_CHECK(a.Hg >= 4 && a.Hg <= GST_HG_MAX && a.Hg % 4 == 0 && a.G == 2 * a.Hg && a.G <= GST_G_MAX, "gst head: sizes");
  TTS_CHECK(a.Es >= 0 && a.Es <= GST_ES_MAX && a.Es % 4 == 0 && (a.Es == 0 || a.spk), "gst head: speaker embedding");
  TTS_CHECK(a.heads >= 1 && a.heads <= GST_HEADS_MAX && a.ntok >= 1 && a.ntok <= GST_TOK_MAX && a.G % a.heads == 0 &&
                (a.G / a.heads) % 4 == 0,
            "gst head: heads / tokens");
  gst_head_kernel<<<B, 256, 0, s>>>(a);
  HIP_OK(hipGetLastError());
}

void launch_gst_tokens(const GstTokenArgs& a, const float* Vt, int G, int ntok, float* out, hipStream_t s) {
  TTS_CHECK(a.n >= 0 && a.n <= GST_DICT_MAX, "gst tokens: at most 64 token weights");
  for (int i = 0; i < a.n; ++i) TTS_CHECK(a.id[i] >= 0 && a.id[i] < ntok, "gst tokens: token index out of range");
  gst_tokens_kernel<<<(G + 255) / 256, 256, 0, s>>>(a, Vt, G, out);
  HIP_OK(hipGetLastError());
}
