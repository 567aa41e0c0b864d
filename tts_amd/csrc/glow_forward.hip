// Glow-TTS analysis direction (gfx950): GlowTts.forward in eval (TTS/tts/models/glow_tts.py:114-156).
//   The flows run first to last (decoder.py:86-99) with their log-determinant, then the likelihood
//   matrix logp (glow_tts.py:141-150), the monotonic alignment search (monotonic_align/core.pyx) and
//   the encoder means expanded along the found path. The convolutions of a coupling block (start, WN,
//   end) are the ones the reverse direction uses (conv.hip, epi 0 / 3); everything between two blocks
//   is one glue kernel here. Activations are channel-major (B, C, T) with lanes along time, as in
//   glow.hip; only positions below a row's length are written.
#include "common.h"
#include "launch.h"

#include <algorithm>

// Between coupling block k-1 and block k, for the squeezed (B, 2C, K) activations:
//   coupling forward of block k-1 (glow.py:253-266): z0 = x0, z1 = m + exp(logs) * x1, with
//     [m_c, logs_c] = rows (2c, 2c + 1) of the end conv's plain output `eo` (rows interleaved at
//     pack time); eo == nullptr for the very first call (x is the squeezed mel)
//   ActNorm forward of block k (normalization.py:82): a = bias + exp(logs) * z
//   InvConvNear forward of block k (glow.py:180-203): the 4 channels {2j, 2j+1, C+2j, C+2j+1} mix
//     through the 4 x 4 weight itself; tab == nullptr after the last block (z goes out as it is)
//   tab: 2C x {w[s'][0..3], actnorm bias, exp(actnorm logs)}; the first four belong to the row as an
//     OUTPUT channel, the last two to the row as an INPUT channel.
// A workgroup owns 64 positions (lanes) and the 4 waves split the C/2 mixing groups. The coupling
// block's log-determinant sum_{c, t < K_b} logs[c, t] (glow.py:264) leaves as one double per
// workgroup, summed in a fixed order (threads in index order), so a rerun repeats it bit for bit.
__global__ __launch_bounds__(256) void glow_fwd_glue_kernel(const float* __restrict__ x, const float* __restrict__ eo,
                                                            const float* __restrict__ tab, float* __restrict__ out,
                                                            int C, int K, const int* klens,
                                                            double* __restrict__ part) {
  __shared__ double red[256];
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const bool valid = k < K && k < klens[b];
  const long base = (long)b * 2 * C * K + (valid ? k : 0);
  double ls = 0.0;
  if (valid) {
    for (int j = w; j < C / 2; j += 4) {
      const int ch[4] = {2 * j, 2 * j + 1, C + 2 * j, C + 2 * j + 1};
      float v[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = x[base + (long)ch[s] * K];
      if (eo) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const float m = eo[base + (long)(4 * j + 2 * p) * K], lg = eo[base + (long)(4 * j + 2 * p + 1) * K];
          v[2 + p] = m + expf(lg) * v[2 + p];
          ls += (double)lg;
        }
      }
      if (tab) {
        float a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = tab[ch[s] * 6 + 4] + tab[ch[s] * 6 + 5] * v[s];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const float* wr = tab + ch[o] * 6;
          float r = wr[0] * a[0];
          r = fmaf(wr[1], a[1], r);
          r = fmaf(wr[2], a[2], r);
          r = fmaf(wr[3], a[3], r);
          out[base + (long)ch[o] * K] = r;
        }
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) out[base + (long)ch[s] * K] = v[s];
      }
    }
  }
  if (!part) return;
  red[threadIdx.x] = ls;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    part[(long)b * gridDim.x + blockIdx.x] = t;
  }
}

// logdet[b] = K_b * wconst + sum of the row's coupling partials (part: (nblk, B, tiles)), in index
// order. wconst = sum_k [sum_c actnorm.logs_k + logdet(W_k) * 2C / 4], folded on the host in double.
__global__ void glow_logdet_kernel(const double* __restrict__ part, int nblk, int tiles, int B, const int* klens,
                                   double wconst, float* __restrict__ logdet) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double t = 0.0;
  for (int k = 0; k < nblk; ++k)
    for (int i = 0; i < tiles; ++i) t += part[((long)k * B + b) * tiles + i];
  logdet[b] = (float)(t + wconst * (double)klens[b]);
}

// logp[t, j] = -C/2 log(2 pi) - 1/2 sum_d z[d, j]^2 + sum_d o_mean[d, t] z[d, j] - 1/2 sum_d o_mean[d, t]^2
// (glow_tts.py:141-150 with o_log_scale = 0: mean_only), zero outside the row's (x_len, y_len) as
// maximum_path's value * mask leaves it. A workgroup owns 64 frames (lanes; the frame's z column
// stays in registers) x 32 tokens (LDS tile, 8 per wave); the sums run in double, so the result is
// the correctly rounded fp32 value of its inputs.
constexpr int LOGP_C = 80, LOGP_TT = 32;
__global__ __launch_bounds__(256) void glow_logp_kernel(const float* __restrict__ om, int Tx, const int* xlens,
                                                        const float* __restrict__ z, int Ty, const int* ylens,
                                                        float* __restrict__ logp) {
  __shared__ float oms[LOGP_C][LOGP_TT];
  __shared__ double omsq[LOGP_TT];
  const int b = blockIdx.z, t0 = blockIdx.y * LOGP_TT, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int xl = xlens[b], yl = ylens[b];
  for (int e = threadIdx.x; e < LOGP_C * LOGP_TT; e += 256) {
    const int d = e / LOGP_TT, tt = e % LOGP_TT;
    oms[d][tt] = t0 + tt < xl ? om[((long)b * LOGP_C + d) * Tx + t0 + tt] : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < LOGP_TT) {
    double s = 0.0;
    for (int d = 0; d < LOGP_C; ++d) s += (double)oms[d][threadIdx.x] * (double)oms[d][threadIdx.x];
    omsq[threadIdx.x] = s;
  }
  __syncthreads();
  if (j >= Ty) return;
  const bool jv = j < yl;
  float zc[LOGP_C];
  double zz = 0.0;
#pragma unroll
  for (int d = 0; d < LOGP_C; ++d) {
    zc[d] = jv ? z[((long)b * LOGP_C + d) * Ty + j] : 0.f;
    zz += (double)zc[d] * (double)zc[d];
  }
  const double c0 = -0.5 * LOGP_C * 1.8378770664093454835606594728112;  // log(2 pi)
  for (int i = 0; i < LOGP_TT / 4; ++i) {
    const int tt = w * (LOGP_TT / 4) + i, t = t0 + tt;
    if (t >= Tx) break;
    double dot = 0.0;
#pragma unroll
    for (int d = 0; d < LOGP_C; ++d) dot += (double)oms[d][tt] * (double)zc[d];
    logp[((long)b * Tx + t) * Ty + j] = (jv && t < xl) ? (float)(c0 - 0.5 * zz + dot - 0.5 * omsq[tt]) : 0.f;
  }
}

// Monotonic alignment search: maximum_path_each (monotonic_align/core.pyx:9-35) restated. One
// workgroup per utterance, threads along x (up to MAS_XPT chunks of blockDim.x tokens each), y
// stepped serially. Column y of Q needs column y - 1 only, which lives in LDS (double-buffered, one
// barrier per step):
//   Q[x, y] = max(x == y ? -1e9 : Q[x, y-1],  x == 0 ? (y == 0 ? 0 : -1e9) : Q[x-1, y-1]) + logp[x, y]
// over the band x in [max(0, tx + y - ty), min(tx, y + 1)); one max and one add per cell in fp32, in
// the reference's order, so Q and the path are bit-determined by logp. The sweep keeps one decision
// bit per cell, (x == y) or Q[x, y-1] < Q[x-1, y-1] (the backtrack's test, core.pyx:34), as one 64-bit
// ballot word per wave and step; logp is read 8 frames ahead. Wave 0 then walks back from
// (tx - 1, ty - 1): per 64 frames every lane fetches its frame's two decision words around the
// current index (the index moves by at most one per frame), and the walk runs over the lanes.
// xof[y] = the token of frame y (-1 at and past ty).
constexpr int MAS_XPT = 4, MAS_PF = 8, MAS_TX_MAX = 4096;
__global__ __launch_bounds__(1024) void glow_mas_kernel(const float* __restrict__ logp, long lb, int ldy,
                                                        const int* xlens, const int* ylens,
                                                        unsigned long long* __restrict__ bits, long bb, int wpr,
                                                        int* __restrict__ xof, int Ty) {
  __shared__ float q[2][MAS_TX_MAX];
  const int b = blockIdx.x, tid = threadIdx.x, BS = blockDim.x, lane = tid & 63;
  const int tx = xlens[b], ty = ylens[b];
  const float* v = logp + (long)b * lb;
  unsigned long long* bw = bits + (long)b * bb;
  constexpr float NEG = -1e9f;
  for (int y = ty + tid; y < Ty; y += BS) xof[(long)b * Ty + y] = -1;
  for (int y0 = 0; y0 < ty; y0 += MAS_PF) {
    float pf[MAS_XPT][MAS_PF];
#pragma unroll
    for (int c = 0; c < MAS_XPT; ++c) {
      const int x = c * BS + tid;
#pragma unroll
      for (int i = 0; i < MAS_PF; ++i) pf[c][i] = (x < tx && y0 + i < ty) ? v[(long)x * ldy + y0 + i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MAS_PF; ++i) {
      const int y = y0 + i;
      if (y < ty) {  // uniform over the workgroup
        const int p = y & 1, lo = max(0, tx + y - ty);
#pragma unroll
        for (int c = 0; c < MAS_XPT; ++c) {
          const int x = c * BS + tid;
          const bool in = x < tx && x >= lo && x <= y;
          bool dec = false;
          if (in) {
            const float v_cur = x == y ? NEG : q[p ^ 1][x];
            const float v_prev = x == 0 ? (y == 0 ? 0.f : NEG) : q[p ^ 1][x - 1];
            dec = x == y || v_cur < v_prev;
            q[p][x] = fmaxf(v_cur, v_prev) + pf[c][i];
          }
          const unsigned long long m = __ballot(dec);
          if (lane == 0 && (x >> 6) < wpr) bw[(long)y * wpr + (x >> 6)] = m;
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();  // the decision words of every wave are visible to wave 0
  if (tid >= 64) return;
  int idx = tx - 1;
  for (int ytop = ty - 1; ytop >= 0; ytop -= 64) {
    const int myy = ytop - lane, wbase = idx >> 6;
    unsigned long long hi = 0, lo = 0;
    if (myy >= 0) {
      hi = bw[(long)myy * wpr + wbase];
      if (wbase > 0) lo = bw[(long)myy * wpr + wbase - 1];
    }
    const int n = min(64, ytop + 1);
    int mine = -1;
    for (int l = 0; l < n; ++l) {
      if (lane == l) mine = idx;
      const unsigned h0 = __shfl((unsigned)hi, l), h1 = __shfl((unsigned)(hi >> 32), l);
      const unsigned l0 = __shfl((unsigned)lo, l), l1 = __shfl((unsigned)(lo >> 32), l);
      const unsigned long long word = (idx >> 6) == wbase ? ((unsigned long long)h1 << 32 | h0)
                                                          : ((unsigned long long)l1 << 32 | l0);
      if (idx != 0 && ((word >> (idx & 63)) & 1ull)) --idx;
    }
    if (myy >= 0) xof[(long)b * Ty + myy] = mine;
  }
}

// path (B, Tx, Ty) as maximum_path returns it: path[x, y] = [xof[y] == x]
__global__ __launch_bounds__(256) void glow_path_kernel(const int* __restrict__ xof, int Tx, int Ty,
                                                        float* __restrict__ path) {
  const int b = blockIdx.y, y = blockIdx.x * 256 + threadIdx.x;
  if (y >= Ty) return;
  const int xo = xof[(long)b * Ty + y];
  for (int x = 0; x < Tx; ++x) path[((long)b * Tx + x) * Ty + y] = x == xo ? 1.f : 0.f;
}

// glow_tts.py:153-155 along the found path: attn (B, Ty, Tx) as forward returns it, and
// y_mean[c, j] = o_mean[c, xof[j]] (zero past the row's frames). 64 frames per workgroup.
__global__ __launch_bounds__(256) void glow_align_out_kernel(const float* __restrict__ om, int C, int Tx,
                                                             const int* __restrict__ xof, int Ty,
                                                             float* __restrict__ y_mean, float* __restrict__ attn) {
  const int b = blockIdx.y, j0 = blockIdx.x * 64, tid = threadIdx.x;
  {
    const int j = j0 + (tid & 63);
    if (j < Ty) {
      const int xo = xof[(long)b * Ty + j];
      for (int c = tid >> 6; c < C; c += 4)
        y_mean[((long)b * C + c) * Ty + j] = xo >= 0 ? om[((long)b * C + c) * Tx + xo] : 0.f;
    }
  }
  const int nj = min(64, Ty - j0);
  for (int r = 0; r < nj; ++r) {
    const int xo = xof[(long)b * Ty + j0 + r];
    float* arow = attn + ((long)b * Ty + j0 + r) * Tx;
    for (int t = tid; t < Tx; t += 256) arow[t] = t == xo ? 1.f : 0.f;
  }
}

// o_attn_dur[t] = log(1 + sum_j path[t, j]) * x_mask (glow_tts.py:111). xof is non-decreasing over
// the row's frames, so a token's frame count is the distance of two lower bounds.
__global__ __launch_bounds__(256) void glow_attn_dur_kernel(const int* __restrict__ xof, int Ty, const int* xlens,
                                                            const int* ylens, int Tx, float* __restrict__ dur) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tx) return;
  const int yl = ylens[b];
  const int* xo = xof + (long)b * Ty;
  auto lower = [&](int key) {  // first frame whose token is >= key
    int lo = 0, hi = yl;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xo[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  dur[(long)b * Tx + t] = t < xlens[b] ? (float)log(1.0 + (double)(lower(t + 1) - lower(t))) : 0.f;
}

void launch_glow_fwd_glue(const float* x, const float* eo, const float* tab, float* out, int C, int K,
                          const int* klens, double* part, int B, hipStream_t s) {
  TTS_CHECK(C % 2 == 0, "glow forward: even channel count");
  glow_fwd_glue_kernel<<<dim3((K + 63) / 64, B), 256, 0, s>>>(x, eo, tab, out, C, K, klens, part);
  HIP_OK(hipGetLastError());
}
void launch_glow_logdet(const double* part, int nblk, int tiles, int B, const int* klens, double wconst, float* logdet,
                        hipStream_t s) {
  glow_logdet_kernel<<<1, 64, 0, s>>>(part, nblk, tiles, B, klens, wconst, logdet);
  HIP_OK(hipGetLastError());
}
void launch_glow_logp(const float* om, int C, int Tx, const int* xlens, const float* z, int Ty, const int* ylens,
                      float* logp, int B, hipStream_t s) {
  TTS_CHECK(C == LOGP_C, "glow: 80 mel channels");
  glow_logp_kernel<<<dim3((Ty + 63) / 64, (Tx + LOGP_TT - 1) / LOGP_TT, B), 256, 0, s>>>(om, Tx, xlens, z, Ty, ylens,
                                                                                         logp);
  HIP_OK(hipGetLastError());
}
long glow_mas_bits_words(int Tx, int Ty) { return (long)Ty * ((Tx + 63) / 64); }
void launch_glow_mas(const float* logp, int Tx, int Ty, const int* xlens, const int* ylens, int max_xlen,
                     unsigned long long* bits, int* xof, int B, hipStream_t s) {
  TTS_CHECK(Tx >= 1 && Tx <= MAS_TX_MAX && max_xlen <= Tx && B <= 64, "glow alignment search: sizes");
  // one thread per token up to 1024, then MAS_XPT tokens per thread
  const int bs = std::min(1024, std::max(64, (max_xlen + 63) / 64 * 64));
  const int wpr = (Tx + 63) / 64;
  glow_mas_kernel<<<B, bs, 0, s>>>(logp, (long)Tx * Ty, Ty, xlens, ylens, bits, glow_mas_bits_words(Tx, Ty), wpr, xof,
                                   Ty);
  HIP_OK(hipGetLastError());
}
void launch_glow_path(const int* xof, int Tx, int Ty, float* path, int B, hipStream_t s) {
  glow_path_kernel<<<dim3((Ty + 255) / 256, B), 256, 0, s>>>(xof, Tx, Ty, path);
  HIP_OK(hipGetLastError());
}
void launch_glow_align_out(const float* om, int C, int Tx, const int* xlens, const int* xof, int Ty, const int* ylens,
                           float* y_mean, float* attn, float* dur, int B, hipStream_t s) {
  glow_align_out_kernel<<<dim3((Ty + 63) / 64, B), 256, 0, s>>>(om, C, Tx, xof, Ty, y_mean, attn);
  HIP_OK(hipGetLastError());
  glow_attn_dur_kernel<<<dim3((Tx + 255) / 256, B), 256, 0, s>>>(xof, Ty, xlens, ylens, Tx, dur);
  HIP_OK(hipGetLastError());
}
