// Vocoder scoring: PQMF analysis (TTS/vocoder/layers/pqmf.py:48-49) and the STFT distances of
// TTS/vocoder/layers/losses.py:7-52 (TorchSTFT, STFTLoss) on waveform rows of their own lengths. fp32.
//
// The STFT is a windowed DFT written as a GEMM on the exact-fp32 MFMA: [2F x K] basis times
// [K x frames], K = win_length (the window is zero elsewhere in the n_fft frame), the basis
// window[k] cos / -sin(2 pi f (k + offset) / n_fft) rounded once from double on the host. A workgroup
// owns ST_TB bins x ST_TF frames of ONE row and keeps the real and imaginary accumulators of both
// signals of a pair for that block, so the epilogue forms both magnitudes in registers: the spectra of
// the distance path never reach memory. Frames are gathered from the caller's rows through
// torch.stft's reflect index; there is no padded copy and no frame buffer. The distance path writes
// three fp32 partial sums per tile, and a second kernel adds a row's tiles in index order in float64.
// K is summed in chunks of ST_KCHUNK: a chain per chunk, the chunk sums added in order.
// A row's tiles depend on its own length only, so its sums are the same bits in any batch.
#include "common.h"
#include "launch.h"

namespace {

// workgroup tile: ST_TB bins x ST_TF frames, K in chunks of ST_KC; 4 waves as 2 (bins) x 2 (frames),
// each 32 x 32 = 2 x 2 MFMA16 blocks, times {re, im} x signals accumulators
constexpr int ST_THREADS = 256, ST_KC = ST_KCHUNK;
constexpr int ST_XS = ST_KC + 4;      // frame-major sample rows: 16 frames x 4 k hit every bank twice
constexpr int ST_WS = 2 * ST_TB + 8;  // k-major basis rows [cos ST_TB | sin ST_TB]: the same
static_assert(ST_TF == 64 && ST_TB == 64 && ST_KC % 4 == 0 && ST_WS % 4 == 0, "tile shape is wired into the wave map");

__device__ __forceinline__ int stft_frames(int len, int n_fft, int hop) {
  return 1 + (len + 2 * (n_fft / 2) - n_fft) / hop;
}

__device__ __forceinline__ float clamped_mag(float re, float im) {
  return sqrtf(fmaxf(fmaf(re, re, im * im), 1e-8f));
}

// grid (frame tiles x bin tiles, B). NSIG = 2, !STORE: partial[(b * tiles_max + tile) * 3 + {A, D, R}]
// of the pair (x0 = y_hat, x1 = y); NSIG = 1, STORE: mag (B, F, frames_max) of x0, zero past a row's
// frames. basis: [bin tile][Kp][cos ST_TB | sin ST_TB], zero for k >= K and bins >= F.
template <int NSIG, bool STORE>
__global__ void __launch_bounds__(ST_THREADS)
    stft_gemm_kernel(const float* __restrict__ x0, const float* __restrict__ x1, long L_max, RowInts nsamp,
                     const float* __restrict__ basis, int Kp, int K, int n_fft, int hop, int woff, int F, int nbt,
                     float* __restrict__ partial, int tiles_max, float* __restrict__ mag, int frames_max) {
  __shared__ __attribute__((aligned(16))) float Xs[NSIG][ST_TF * ST_XS];
  __shared__ __attribute__((aligned(16))) float Ws[ST_KC * ST_WS];
  __shared__ float red[ST_THREADS / 64][3];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ft = blockIdx.x / nbt, bt = blockIdx.x - ft * nbt;
  const int len = nsamp.v[b], half = n_fft / 2, nfr = stft_frames(len, n_fft, hop), t0 = ft * ST_TF;
  if (t0 >= nfr) {
    if constexpr (STORE) {
      for (int i = tid; i < ST_TB * ST_TF; i += ST_THREADS) {
        const int f = bt * ST_TB + i / ST_TF, t = t0 + i % ST_TF;
        if (f < F && t < frames_max) mag[((size_t)b * F + f) * frames_max + t] = 0.f;
      }
    }
    return;
  }
  const float* xs[2] = {x0 + (size_t)b * L_max, NSIG == 2 ? x1 + (size_t)b * L_max : nullptr};
  const int l = tid & 63, w = tid >> 6, wn = w & 1, wm = w >> 1, li = l & 15, lk = l >> 4;

  // [signal][frame block][bin block][re, im]. Summation order of one output: every K chunk is an
  // fma chain in k order from zero (part, on the MFMA), and the chunk sums are added in chunk order
  // (acc). One chain over a 1200-point window would round 1200 times at the size of the growing
  // sum; this way the large partial sums are rounded once per chunk.
  f32x4 acc[NSIG][2][2][2], part[NSIG][2][2][2];
#pragma unroll
  for (int s = 0; s < NSIG; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[s][i >> 2][(i >> 1) & 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Kp; k0 += ST_KC) {
#pragma unroll
    for (int s = 0; s < NSIG; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) part[s][i >> 2][(i >> 1) & 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // samples: thread -> (frame, k), consecutive k of a frame are consecutive samples
    for (int i = tid; i < ST_TF * ST_KC; i += ST_THREADS) {
      const int fr = i / ST_KC, kk = i - fr * ST_KC, k = k0 + kk, t = t0 + fr;
      int p = t * hop + k + woff - half;
      p = p < 0 ? -p : p;
      p = p >= len ? 2 * (len - 1) - p : p;
      p = min(max(p, 0), len - 1);
      const bool on = t < nfr && k < K;
#pragma unroll
      for (int s = 0; s < NSIG; ++s) Xs[s][fr * ST_XS + kk] = on ? xs[s][p] : 0.f;
    }
    const float4* src = reinterpret_cast<const float4*>(basis + ((size_t)bt * Kp + k0) * (2 * ST_TB));
    for (int i = tid; i < ST_KC * (2 * ST_TB / 4); i += ST_THREADS) {
      const int kk = i / (2 * ST_TB / 4), c4 = i - kk * (2 * ST_TB / 4);
      *reinterpret_cast<float4*>(&Ws[kk * ST_WS + 4 * c4]) = src[i];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < ST_KC; ks += 4) {
      const int k = ks + lk;
      float wv[2][2], xv[NSIG][2];
#pragma unroll
      for (int bs = 0; bs < 2; ++bs)
#pragma unroll
        for (int ri = 0; ri < 2; ++ri) wv[bs][ri] = Ws[k * ST_WS + ri * ST_TB + wn * 32 + bs * 16 + li];
#pragma unroll
      for (int s = 0; s < NSIG; ++s)
#pragma unroll
        for (int fs = 0; fs < 2; ++fs) xv[s][fs] = Xs[s][(wm * 32 + fs * 16 + li) * ST_XS + k];
#pragma unroll
      for (int s = 0; s < NSIG; ++s)
#pragma unroll
        for (int fs = 0; fs < 2; ++fs)
#pragma unroll
          for (int bs = 0; bs < 2; ++bs)
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) part[s][fs][bs][ri] = MFMA16(wv[bs][ri], xv[s][fs], part[s][fs][bs][ri]);
    }
#pragma unroll
    for (int s = 0; s < NSIG; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[s][i >> 2][(i >> 1) & 1][i & 1] += part[s][i >> 2][(i >> 1) & 1][i & 1];
    __syncthreads();
  }

  // D: column (l & 15) = frame, row 4 (l >> 4) + r = bin
  float sA = 0.f, sD = 0.f, sR = 0.f;
#pragma unroll
  for (int fs = 0; fs < 2; ++fs)
#pragma unroll
    for (int bs = 0; bs < 2; ++bs)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + wm * 32 + fs * 16 + li, f = bt * ST_TB + wn * 32 + bs * 16 + 4 * lk + r;
        const float m0 = clamped_mag(acc[0][fs][bs][0][r], acc[0][fs][bs][1][r]);
        if constexpr (STORE) {
          if (f < F && t < frames_max) mag[((size_t)b * F + f) * frames_max + t] = t < nfr ? m0 : 0.f;
        } else {
          const float m1 = clamped_mag(acc[NSIG - 1][fs][bs][0][r], acc[NSIG - 1][fs][bs][1][r]);
          if (f < F && t < nfr) {
            const float d = m1 - m0;
            sA += fabsf(logf(m1) - logf(m0));
            sD = fmaf(d, d, sD);
            sR = fmaf(m1, m1, sR);
          }
        }
      }
  if constexpr (!STORE) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      sA += __shfl_xor(sA, o);
      sD += __shfl_xor(sD, o);
      sR += __shfl_xor(sR, o);
    }
    if (l == 0) {
      red[w][0] = sA;
      red[w][1] = sD;
      red[w][2] = sR;
    }
    __syncthreads();
    if (tid < 3)
      partial[((size_t)b * tiles_max + blockIdx.x) * 3 + tid] =
          ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// grid B, 64 threads: thread q < 3 adds quantity q of the row's own tiles in index order, in float64
__global__ void __launch_bounds__(64) stft_row_sums_kernel(const float* __restrict__ partial, int tiles_max,
                                                           RowInts nsamp, int n_fft, int hop, int nbt,
                                                           double* __restrict__ sums) {
  const int b = blockIdx.x, q = threadIdx.x;
  if (q >= 3) return;
  const int nfr = stft_frames(nsamp.v[b], n_fft, hop);
  const int tiles = min((nfr + ST_TF - 1) / ST_TF * nbt, tiles_max);
  double s = 0.0;
  for (int i = 0; i < tiles; ++i) s += (double)partial[((size_t)b * tiles_max + i) * 3 + q];
  sums[b * 3 + q] = s;
}

// grid (ceil(Lout_max / 256), B): thread -> one output position of all N bands,
// y[b][n][j] = sum_k H[n][k] x[b][j N + k - pad], x zero outside [0, len_b), k ascending
constexpr int PQ_THREADS = 256;
__global__ void __launch_bounds__(PQ_THREADS)
    pqmf_analysis_kernel(const float* __restrict__ x, long L_max, RowInts lens, const float* __restrict__ H, int N,
                         int ntap, int pad, float* __restrict__ y, int Lout_max) {
  __shared__ float Hs[PQ_NMAX * PQ_NTAP_MAX];
  for (int i = threadIdx.x; i < N * ntap; i += PQ_THREADS) Hs[i] = H[i];
  __syncthreads();
  const int j = blockIdx.x * PQ_THREADS + threadIdx.x, b = blockIdx.y;
  if (j >= Lout_max) return;
  const int len = lens.v[b], Lout = len > 0 ? (len - 1) / N + 1 : 0;
  const float* xr = x + (size_t)b * L_max;
  float acc[PQ_NMAX] = {};
  if (j < Lout) {
    for (int k = 0; k < ntap; ++k) {
      const int q = j * N + k - pad;
      const float xv = (q >= 0 && q < len) ? xr[q] : 0.f;
#pragma unroll
      for (int n = 0; n < PQ_NMAX; ++n)
        if (n < N) acc[n] = fmaf(Hs[n * ntap + k], xv, acc[n]);
    }
  }
#pragma unroll
  for (int n = 0; n < PQ_NMAX; ++n)
    if (n < N) y[((size_t)b * N + n) * Lout_max + j] = acc[n];
}

}  // namespace

void launch_pqmf_analysis(const float* x, long L_max, const RowInts& lens, int B, const float* H, int N, int ntap,
                          float* y, int Lout_max, hipStream_t s) {
  pqmf_analysis_kernel<<<dim3((Lout_max + PQ_THREADS - 1) / PQ_THREADS, B), PQ_THREADS, 0, s>>>(
      x, L_max, lens, H, N, ntap, (ntap - 1) / 2, y, Lout_max);
  HIP_OK(hipGetLastError());
}

void launch_stft_pair_sums(const float* yhat, const float* y, long L_max, const RowInts& nsamp, int B,
                           const StftBasis& W, int hop, int frames_max, float* partial, double* sums, hipStream_t s) {
  const int tiles_max = (frames_max + ST_TF - 1) / ST_TF * W.nbt;
  stft_gemm_kernel<2, false><<<dim3(tiles_max, B), ST_THREADS, 0, s>>>(yhat, y, L_max, nsamp, W.d, W.Kp, W.K, W.n_fft,
                                                                      hop, W.woff, W.F, W.nbt, partial, tiles_max,
                                                                      nullptr, 0);
  HIP_OK(hipGetLastError());
  stft_row_sums_kernel<<<B, 64, 0, s>>>(partial, tiles_max, nsamp, W.n_fft, hop, W.nbt, sums);
  HIP_OK(hipGetLastError());
}

void launch_stft_mag_store(const float* wav, long L_max, const RowInts& nsamp, int B, const StftBasis& W, int hop,
                           float* mag, int frames_max, hipStream_t s) {
  const int tiles_max = (frames_max + ST_TF - 1) / ST_TF * W.nbt;
  stft_gemm_kernel<1, true><<<dim3(tiles_max, B), ST_THREADS, 0, s>>>(wav, nullptr, L_max, nsamp, W.d, W.Kp, W.K,
                                                                     W.n_fft, hop, W.woff, W.F, W.nbt, nullptr,
                                                                     tiles_max, mag, frames_max);
  HIP_OK(hipGetLastError());
}
