// Tacotron (v1) kernels (TTS/tts/layers/tacotron.py): the CBHG convolutions and linears as one
// channel-last fp32 conv, the highway stack, the bidirectional sequence GRU (H = 128) and the
// autoregressive GRU decoder as one launch with a workgroup per utterance. All plain fp32 FMA chains
// in a fixed order per output element, so a row's result does not depend on the rows around it.
#include "common.h"
#include "launch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Channel-last Conv1d / Linear: out[b][t][oc0 + co] = act(bias[co] + sum_{k,ci} W[k][ci][co] *
// x[b][t + k - padl][ci]) (+ resid[b][t][co]), zero padding at the row's own length, zero rows for
// t >= lens[b]. A workgroup computes CV_TT positions x 128 output channels; the input window goes
// through LDS in chunks of CV_CC channels.
// ---------------------------------------------------------------------------------------------
constexpr int CV_TT = 8, CV_CC = 32, CV_KMAX = 16;

__global__ __launch_bounds__(128) void t1_conv_kernel(const float* __restrict__ x, long xb, int ldx, int Cin,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      int K, int padl, int Cout, int act,
                                                      const float* __restrict__ resid, long rb, int ldr,
                                                      float* __restrict__ out, long ob, int ldo, int oc0,
                                                      const int* __restrict__ lens, int T_max) {
  __shared__ float xs[(CV_TT + CV_KMAX - 1) * CV_CC];
  const int b = blockIdx.z, t0 = blockIdx.x * CV_TT, co = blockIdx.y * 128 + threadIdx.x;
  const int len = lens[b];
  if (t0 >= len) {  // past the row: zeros (the grid covers the longest row)
    if (co < Cout)
      for (int p = 0; p < CV_TT && t0 + p < T_max; ++p) out[b * ob + (long)(t0 + p) * ldo + oc0 + co] = 0.f;
    return;
  }
  const int cw = co < Cout ? co : Cout - 1;  // clamp: idle lanes read a valid column
  float acc[CV_TT];
#pragma unroll
  for (int p = 0; p < CV_TT; ++p) acc[p] = 0.f;
  const int win = CV_TT + K - 1;
  for (int c0 = 0; c0 < Cin; c0 += CV_CC) {
    const int cn = min(CV_CC, Cin - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < win * CV_CC; i += 128) {
      const int w = i / CV_CC, c = i % CV_CC, t = t0 + w - padl;
      xs[i] = (c < cn && t >= 0 && t < len) ? x[b * xb + (long)t * ldx + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const float* wk = W + ((long)k * Cin + c0) * Cout + cw;
      const float* xk = xs + k * CV_CC;
#pragma unroll 4
      for (int c = 0; c < cn; ++c) {
        const float w = wk[(long)c * Cout];
#pragma unroll
        for (int p = 0; p < CV_TT; ++p) acc[p] = fmaf(w, xk[p * CV_CC + c], acc[p]);
      }
    }
  }
  if (co >= Cout) return;
  const float bv = bias ? bias[co] : 0.f;
#pragma unroll
  for (int p = 0; p < CV_TT; ++p) {
    const int t = t0 + p;
    if (t >= T_max) break;
    float v = acc[p] + bv;
    if (act == 1) v = fmaxf(v, 0.f);
    if (resid && t < len) v += resid[b * rb + (long)t * ldr + co];
    out[b * ob + (long)t * ldo + oc0 + co] = t < len ? v : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// Highway stack, 4 layers of y = relu(H x) sigmoid(T x) + x (1 - sigmoid(T x)) on 128 channels, in
// place; a workgroup of 128 threads carries HW_P positions through all layers.
//   Wt: [layer][H | T][in 128][out 128], bias: [layer][H | T][128]
// ---------------------------------------------------------------------------------------------
constexpr int HW_P = 4;

__global__ __launch_bounds__(128) void t1_highway_kernel(float* __restrict__ x, long xb, const float* __restrict__ Wt,
                                                         const float* __restrict__ bias, const int* __restrict__ lens) {
  __shared__ float xs[HW_P][128];
  const int b = blockIdx.y, t0 = blockIdx.x * HW_P, j = threadIdx.x;
  const int len = lens[b];
  if (t0 >= len) return;
  for (int p = 0; p < HW_P; ++p) xs[p][j] = t0 + p < len ? x[b * xb + (long)(t0 + p) * 128 + j] : 0.f;
  __syncthreads();
  for (int l = 0; l < 4; ++l) {
    const float* wh = Wt + (long)(2 * l) * 128 * 128 + j;
    const float* wt = wh + 128 * 128;
    float h[HW_P], g[HW_P];
#pragma unroll
    for (int p = 0; p < HW_P; ++p) h[p] = g[p] = 0.f;
#pragma unroll 4
    for (int c = 0; c < 128; ++c) {
      const float a = wh[c * 128], e = wt[c * 128];
#pragma unroll
      for (int p = 0; p < HW_P; ++p) {
        h[p] = fmaf(a, xs[p][c], h[p]);
        g[p] = fmaf(e, xs[p][c], g[p]);
      }
    }
    const float bh = bias[(2 * l) * 128 + j], bt = bias[(2 * l + 1) * 128 + j];
    float y[HW_P];
#pragma unroll
    for (int p = 0; p < HW_P; ++p) {
      const float tg = sigm_f(g[p] + bt);
      y[p] = fmaxf(h[p] + bh, 0.f) * tg + xs[p][j] * (1.f - tg);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < HW_P; ++p) xs[p][j] = y[p];
    __syncthreads();
  }
  for (int p = 0; p < HW_P; ++p)
    if (t0 + p < len) x[b * xb + (long)(t0 + p) * 128 + j] = xs[p][j];
}

// ---------------------------------------------------------------------------------------------
// Bidirectional sequence GRU, H = 128 (nn.GRU gate order r, z, n). One workgroup per (row,
// direction); thread i keeps row i of W_hh (384 x 128) in registers for the whole sequence, h lives
// in LDS. The reverse direction starts at the row's last position.
//   gin : (B, T, 768) = [dir][r | z | n] W_ih x + b_ih     Whh: [dir][384][128]   bhh: [dir][384]
//   out : (B, T, 256) = [forward h | reverse h], zero for t >= lens[b]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(384) void t1_bigru_kernel(const float* __restrict__ gin, long gb,
                                                       const float* __restrict__ Whh, const float* __restrict__ bhh,
                                                       const int* __restrict__ lens, int T_max,
                                                       float* __restrict__ out, long ob) {
  __shared__ __attribute__((aligned(16))) float hs[128];
  __shared__ float hh[384];
  const int b = blockIdx.x, dir = blockIdx.y, i = threadIdx.x;
  const int len = lens[b];
  float w[128];
  const float4* wr = reinterpret_cast<const float4*>(Whh + ((long)dir * 384 + i) * 128);
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const float4 v = wr[c];
    w[4 * c] = v.x, w[4 * c + 1] = v.y, w[4 * c + 2] = v.z, w[4 * c + 3] = v.w;
  }
  const float bi = bhh[dir * 384 + i];
  if (i < 128) hs[i] = 0.f;
  float hprev = 0.f;
  __syncthreads();
  for (int s = 0; s < len; ++s) {
    const int t = dir ? len - 1 - s : s;
    const float* g = gin + b * gb + (long)t * 768 + dir * 384;
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (i < 128) gr = g[i], gz = g[128 + i], gn = g[256 + i];  // in flight during the dot product
    float acc = bi;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const float4 h4 = reinterpret_cast<const float4*>(hs)[c];
      acc = fmaf(w[4 * c], h4.x, acc);
      acc = fmaf(w[4 * c + 1], h4.y, acc);
      acc = fmaf(w[4 * c + 2], h4.z, acc);
      acc = fmaf(w[4 * c + 3], h4.w, acc);
    }
    hh[i] = acc;
    __syncthreads();
    if (i < 128) {
      const float r = sigm_f(gr + hh[i]), z = sigm_f(gz + hh[128 + i]);
      const float n = tanh_f(gn + r * hh[256 + i]);
      hprev = (1.f - z) * n + z * hprev;
      hs[i] = hprev;
      out[b * ob + (long)t * 256 + dir * 128 + i] = hprev;
    }
    __syncthreads();
  }
  if (i < 128)
    for (int t = len; t < T_max; ++t) out[b * ob + (long)t * 256 + dir * 128 + i] = 0.f;
}

// ---------------------------------------------------------------------------------------------
// The decoder (layers/tacotron.py:383-495): one launch, one workgroup of DEC_NT threads per
// utterance, the whole loop on the device. Weights are transposed ([in][out]) so that adjacent threads
// of a GEMV read adjacent columns; a GEMV splits its K range over thread groups (dec_gemv).
// ---------------------------------------------------------------------------------------------
constexpr int DEC_NT = 1024, DEC_NW = DEC_NT / 64;

struct DecLds {
  float mem[T1_MEM_MAX * 80];  // memory input (prenet input)
  float p1[256];
  float xin[384];   // [prenet out 128 | context 256]
  float din[512];   // [attention_rnn hidden 256 | context 256]
  float gi[768], gh[768];
  float q[128];
  float d[256], h1[256], h2[256];
  float y[T1_R_MAX * 80];
  float alpha[T1_T_MAX], acum[T1_T_MAX], e[T1_T_MAX];
  __attribute__((aligned(16))) float part[4 * DEC_NT];
  float red[DEC_NW];
};

// partial dot products of a GEMV: the value of output j (bias excluded) lands in the return value
// of threads tid < N; every thread must call it. x in LDS, Wt [K][N] in global memory, N % 4 == 0.
// A thread owns 4 adjacent outputs (one 16-byte load per k) over one of S = DEC_NT / (N / 4) slices
// of K, eight loads in flight; the slices' partial sums are added in slice order.
__device__ __noinline__ float dec_gemv(const float* __restrict__ Wt, const float* x, int K, int N, float* part) {
  const int tid = threadIdx.x;
  const int NG = N >> 2, S = DEC_NT / NG;  // S * N <= 4 * DEC_NT floats of part
  const int g = tid % NG, s = tid / NG;
  if (s < S) {
    const int kc = (K + S - 1) / S, k0 = s * kc, k1 = min(K, k0 + kc);
    const float4* w = reinterpret_cast<const float4*>(Wt) + g;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int k = k0; k < k1; ++k) {
      const float4 wv = w[(long)k * NG];
      const float xv = x[k];
      a.x = fmaf(wv.x, xv, a.x);
      a.y = fmaf(wv.y, xv, a.y);
      a.z = fmaf(wv.z, xv, a.z);
      a.w = fmaf(wv.w, xv, a.w);
    }
    reinterpret_cast<float4*>(part)[s * NG + g] = a;
  }
  __syncthreads();
  float v = 0.f;
  if (tid < N)
    for (int q = 0; q < S; ++q) v += part[q * N + tid];
  __syncthreads();
  return v;
}

// sum of v over the workgroup, in a fixed order; every thread gets it
__device__ __forceinline__ float dec_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < DEC_NW; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ float dec_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1; w < DEC_NW; ++w) s = fmaxf(s, red[w]);
  return s;
}

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

// GRUCell update of h (LDS, 256) from gi = W_ih x + b_ih and gh = W_hh h + b_hh (gate order r, z, n)
__device__ __forceinline__ void dec_gru_update(const float* gi, const float* gh, float* h) {
  const int j = threadIdx.x;
  if (j < 256) {
    const float r = sigm_f(gi[j] + gh[j]), z = sigm_f(gi[256 + j] + gh[256 + j]);
    const float n = tanh_f(gi[512 + j] + r * gh[512 + j]);
    h[j] = (1.f - z) * n + z * h[j];
  }
  __syncthreads();
}

__global__ __launch_bounds__(DEC_NT) void t1_decoder_kernel(T1DecArgs a) {
  __shared__ DecLds L;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.lens[b], r = a.r, F = 80, Y = 80 * a.r_init;
  const int memw = a.mem_frames > 0 ? a.mem_frames * F : F;
  const float* enc = a.enc + (long)b * a.T_max * 256;
  const float* pin = a.pin + (long)b * a.T_max * 128;
  const int max_steps = a.max_steps[b];

  for (int i = tid; i < memw; i += DEC_NT) L.mem[i] = 0.f;
  for (int i = tid; i < 384; i += DEC_NT) L.xin[i] = 0.f;
  for (int i = tid; i < 512; i += DEC_NT) L.din[i] = 0.f;
  for (int i = tid; i < 256; i += DEC_NT) L.h1[i] = L.h2[i] = 0.f;
  for (int i = tid; i < T; i += DEC_NT) L.alpha[i] = L.acum[i] = 0.f;
  __syncthreads();

  int steps = 0, status = 0;
  for (int step = 0; step < a.S_cap; ++step) {
    // prenet (with bias, ReLU)
    float v = dec_gemv(a.pre1, L.mem, memw, 256, L.part);
    if (tid < 256) L.p1[tid] = fmaxf(v + a.pre1_b[tid], 0.f);
    __syncthreads();
    v = dec_gemv(a.pre2, L.p1, 256, 128, L.part);
    if (tid < 128) L.xin[tid] = fmaxf(v + a.pre2_b[tid], 0.f);
    __syncthreads();
    // attention_rnn = GRUCell([prenet, context]) on the hidden state din[0:256]
    v = dec_gemv(a.att_ih, L.xin, 384, 768, L.part);
    if (tid < 768) L.gi[tid] = v + a.att_bih[tid];
    v = dec_gemv(a.att_hh, L.din, 256, 768, L.part);
    if (tid < 768) L.gh[tid] = v + a.att_bhh[tid];
    __syncthreads();
    dec_gru_update(L.gi, L.gh, L.din);
    // location-sensitive attention: e[t] = v . tanh(Wq h + Wcomb * [alpha; acum] + pin[t]) + bv
    v = dec_gemv(a.wq, L.din, 256, 128, L.part);
    if (tid < 128) L.q[tid] = v;
    __syncthreads();
    {
      const float q0 = L.q[lane], q1 = L.q[lane + 64], v0 = a.v[lane], v1 = a.v[lane + 64];
      for (int t = wave; t < T; t += DEC_NW) {
        float s0 = q0 + pin[(long)t * 128 + lane], s1 = q1 + pin[(long)t * 128 + lane + 64];
        for (int k = 0; k < 31; ++k) {
          const int u = t + k - 15;
          if (u < 0 || u >= T) continue;  // wave-uniform
          const float a0 = L.alpha[u], a1 = L.acum[u];
          const float* wc = a.wcomb + k * 128;
          s0 = fmaf(wc[lane], a0, s0);
          s1 = fmaf(wc[lane + 64], a0, s1);
          s0 = fmaf(wc[31 * 128 + lane], a1, s0);
          s1 = fmaf(wc[31 * 128 + lane + 64], a1, s1);
        }
        float e = v0 * tanh_e(s0) + v1 * tanh_e(s1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        if (lane == 0) L.e[t] = e + a.bv;
      }
    }
    __syncthreads();
    {
      float mx = 0.f;
      if (a.softmax) {
        float m = -INFINITY;
        for (int t = tid; t < T; t += DEC_NT) m = fmaxf(m, L.e[t]);
        mx = dec_block_max(m, L.red);
      }
      float part = 0.f;
      for (int t = tid; t < T; t += DEC_NT) {
        const float w = a.softmax ? expf(L.e[t] - mx) : sigmoid_exact(L.e[t]);
        L.e[t] = w;
        part += w;
      }
      const float inv = 1.f / dec_block_sum(part, L.red);
      float* al = a.align + ((long)b * a.S_cap + step) * a.T_max;
      for (int t = tid; t < T; t += DEC_NT) {
        const float w = L.e[t] * inv;
        L.alpha[t] = w;
        L.acum[t] += w;
        al[t] = w;
      }
    }
    __syncthreads();
    {  // context = alpha . enc: 256 channels x 4 slices of the positions
      const int c = tid & 255, s = tid >> 8, tc = (T + 3) / 4, t1 = min(T, (s + 1) * tc);
      float acc = 0.f;
      for (int t = s * tc; t < t1; ++t) acc = fmaf(L.alpha[t], enc[(long)t * 256 + c], acc);
      L.part[tid] = acc;
      __syncthreads();
      if (tid < 256) {
        const float cx = (L.part[tid] + L.part[256 + tid]) + (L.part[512 + tid] + L.part[768 + tid]);
        L.xin[128 + tid] = cx;
        L.din[256 + tid] = cx;
      }
      __syncthreads();
    }
    // project_to_decoder_in, then two residual GRUCells
    v = dec_gemv(a.pdi, L.din, 512, 256, L.part);
    if (tid < 256) L.d[tid] = v + a.pdi_b[tid];
    __syncthreads();
    for (int l = 0; l < 2; ++l) {
      float* h = l ? L.h2 : L.h1;
      v = dec_gemv(a.rnn_ih[l], L.d, 256, 768, L.part);
      if (tid < 768) L.gi[tid] = v + a.rnn_bih[l][tid];
      v = dec_gemv(a.rnn_hh[l], h, 256, 768, L.part);
      if (tid < 768) L.gh[tid] = v + a.rnn_bhh[l][tid];
      __syncthreads();
      dec_gru_update(L.gi, L.gh, h);
      if (tid < 256) L.d[tid] += h[tid];
      __syncthreads();
    }
    // proj_to_mel (all 80 r_init columns feed the stopnet), stop token
    v = dec_gemv(a.mel, L.d, 256, Y, L.part);
    if (tid < Y) L.y[tid] = v + a.mel_b[tid];
    __syncthreads();
    float sp = 0.f;
    for (int i = tid; i < 256 + Y; i += DEC_NT) sp = fmaf(a.stop_w[i], i < 256 ? L.d[i] : L.y[i - 256], sp);
    const float logit = dec_block_sum(sp, L.red) + a.stop_b;
    const float stop = sigmoid_exact(logit);
    // outputs of the step, next memory input (_update_memory_input)
    float* dec = a.dec + ((long)b * a.S_cap + step) * r * F;
    for (int i = tid; i < r * F; i += DEC_NT) dec[i] = L.y[i];
    if (tid == 0) a.stop[(long)b * a.S_cap + step] = stop;
    const int nkeep = a.mem_frames > r ? (a.mem_frames - r) * F : 0;  // < 3 * DEC_NT (T1_MEM_MAX frames)
    float keep[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) keep[q] = tid + q * DEC_NT < nkeep ? L.mem[tid + q * DEC_NT] : 0.f;
    __syncthreads();
    if (a.mem_frames <= 0) {
      for (int i = tid; i < F; i += DEC_NT) L.mem[i] = L.y[(r - 1) * F + i];
    } else if (a.mem_frames > r) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (tid + q * DEC_NT < nkeep) L.mem[r * F + tid + q * DEC_NT] = keep[q];
      for (int i = tid; i < r * F; i += DEC_NT) L.mem[i] = L.y[i];
    } else {
      for (int i = tid; i < memw; i += DEC_NT) L.mem[i] = L.y[i];
    }
    __syncthreads();
    // stop rule (Decoder.inference:489-494), t = step + 1
    steps = step + 1;
    const bool late = 4 * steps > T;  // t > T / 4
    if (late && (stop > 0.6f || (double)L.alpha[T - 1] > 0.6)) {
      status = 1;
      break;
    }
    if (steps > max_steps) {
      status = 2;
      break;
    }
  }
  if (tid == 0) {
    a.steps[b] = steps;
    a.status[b] = status;
    a.mlens[b] = steps * r;
  }
}

}  // namespace

void launch_t1_conv(const T1Conv& c, const int* lens, int B, int T_max, hipStream_t s) {
  if (B <= 0 || T_max <= 0) return;
  dim3 grid((T_max + CV_TT - 1) / CV_TT, (c.Cout + 127) / 128, B);
  t1_conv_kernel<<<grid, 128, 0, s>>>(c.x, c.xb, c.ldx, c.Cin, c.W, c.bias, c.K, c.padl, c.Cout, c.act, c.resid,
                                      c.rb, c.ldr, c.out, c.ob, c.ldo, c.oc0, lens, T_max);
  HIP_OK(hipGetLastError());
}

void launch_t1_highway(float* x, long xb, const float* Wt, const float* bias, const int* lens, int B, int T_max,
                       hipStream_t s) {
  if (B <= 0 || T_max <= 0) return;
  t1_highway_kernel<<<dim3((T_max + HW_P - 1) / HW_P, B), 128, 0, s>>>(x, xb, Wt, bias, lens);
  HIP_OK(hipGetLastError());
}

void launch_t1_bigru(const float* gin, long gb, const float* Whh, const float* bhh, const int* lens, int B, int T_max,
                     float* out, long ob, hipStream_t s) {
  if (B <= 0 || T_max <= 0) return;
  t1_bigru_kernel<<<dim3(B, 2), 384, 0, s>>>(gin, gb, Whh, bhh, lens, T_max, out, ob);
  HIP_OK(hipGetLastError());
}

void launch_t1_decoder(const T1DecArgs& a, int B, hipStream_t s) {
  if (B <= 0) return;
  t1_decoder_kernel<<<B, DEC_NT, 0, s>>>(a);
  HIP_OK(hipGetLastError());
}
