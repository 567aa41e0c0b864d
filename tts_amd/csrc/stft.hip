// Batched audio analysis, the forward direction of griffin_lim.hip: waveform rows -> STFT magnitudes
// (AudioProcessor._stft on librosa.stft conventions, with the pre-emphasis of audio.py:198-202 folded
// into the gather) -> normalised dB features (audio.py:108-124, 216-230). fp32.
//
// One workgroup per STFT frame, reading its samples straight from the caller's waveform row, so no
// padded or pre-emphasised copy of the signal and no frame buffer is ever written. n_fft = 1024 runs
// the 512-point complex FFT of gl_math.h in one wave; any other n_fft a direct DFT. stft_math.h
// holds the arithmetic; the kernels here only place it between barriers.
#include "common.h"
#include "stft_math.h"
#include "launch.h"

namespace {

using namespace gl;

// in-place 512-point complex FFT of the wave's LDS buffer (as in griffin_lim.hip)
template <int SIGN>
__device__ __forceinline__ void fft512(float2* buf, const float2* __restrict__ W, int j) {
  float2 v[8];
#pragma unroll
  for (int Ns = 1; Ns < NH; Ns *= 8) {
    fft512_load<SIGN>(buf, W, Ns, j, v);
    __syncthreads();
    fft512_store(buf, Ns, j, v);
    __syncthreads();
  }
}

// grid (M_max, B), 64 threads: |STFT| of frame t of row b, 513 bins. nsamp.v[b] = samples of row b;
// frames t >= 1 + nsamp / hop read nothing and are written as zeros.
__global__ void __launch_bounds__(LANES) stft_frame_kernel(const float* __restrict__ wav, long L_max, RowInts nsamp,
                                                           const float2* __restrict__ W,
                                                           const float* __restrict__ win, int M_max, int hop, int wlo,
                                                           int whi, float preemph, float* __restrict__ out) {
  __shared__ float2 buf[BUF];
  const int t = blockIdx.x, b = blockIdx.y, j = threadIdx.x, L = nsamp.v[b];
  float* o = out + ((size_t)b * M_max + t) * NBIN;
  if (t >= 1 + L / hop) {
    for (int k = j; k < NBIN; k += LANES) o[k] = 0.f;
    return;
  }
  stft::gather1024(buf, wav + (size_t)b * L_max, L, win, hop, wlo, whi, preemph, t, j);
  __syncthreads();
  fft512<-1>(buf, W, j);
  stft::split_mag(buf, W, o, j);
}

// grid (M_max, B), DFT_THREADS threads, LDS: the n_fft-entry twiddle table, then the windowed frame.
// Thread-strided bins, each a direct sum over the window's support.
constexpr int DFT_THREADS = 256;
__global__ void __launch_bounds__(DFT_THREADS) dft_frame_kernel(const float* __restrict__ wav, long L_max,
                                                                RowInts nsamp, const float2* __restrict__ W,
                                                                const float* __restrict__ win, int M_max, int n_fft,
                                                                int hop, int wlo, int whi, float preemph,
                                                                float* __restrict__ out) {
  extern __shared__ float2 dft_lds[];  // [n_fft] twiddles, [n_fft] floats
  float2* tab = dft_lds;
  float* x = reinterpret_cast<float*>(dft_lds + n_fft);
  const int t = blockIdx.x, b = blockIdx.y, L = nsamp.v[b], nbin = n_fft / 2 + 1;
  float* o = out + ((size_t)b * M_max + t) * nbin;
  if (t >= 1 + L / hop) {
    for (int k = threadIdx.x; k < nbin; k += DFT_THREADS) o[k] = 0.f;
    return;
  }
  const float* y = wav + (size_t)b * L_max;
  for (int n = threadIdx.x; n < n_fft; n += DFT_THREADS) {
    tab[n] = W[n];
    x[n] = (n >= wlo && n < whi) ? stft::frame_sample(y, L, win, n_fft / 2, hop, preemph, t, n) : 0.f;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nbin; k += DFT_THREADS) o[k] = stft::dft_bin(x, tab, n_fft, wlo, whi, k);
}

// out = clip(gain log10(max(1e-5, X)) scale + offset), X = basis @ mag (or mag itself without a
// basis), on FEAT_TF frames per block: the frames' magnitudes in LDS, each thread one output channel
// of all the frames (plain FMA), the mirror of mel_to_linear_kernel
constexpr int FEAT_TF = 8, FEAT_THREADS = 256;
__global__ void __launch_bounds__(FEAT_THREADS)
    mag_to_feature_kernel(const float* __restrict__ mag, RowInts lens, int M_max, int F, int C,
                          const float* __restrict__ basis, float gain, const float* __restrict__ scale,
                          const float* __restrict__ offset, float clip_lo, float clip_hi, int use_clip,
                          float* __restrict__ out) {
  extern __shared__ float amp[];  // [FEAT_TF][F]
  const int b = blockIdx.y, t0 = blockIdx.x * FEAT_TF, M = lens.v[b];
  const int nfr = min(FEAT_TF, M_max - t0);
  for (int i = threadIdx.x; i < FEAT_TF * F; i += FEAT_THREADS) {
    const int f = i / F, k = i - f * F;
    amp[i] = t0 + f < M ? mag[((size_t)b * M_max + t0 + f) * F + k] : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += FEAT_THREADS) {
    float acc[FEAT_TF] = {};
    if (basis) {
      const float* w = basis + (size_t)c * F;
      for (int k = 0; k < F; ++k) {
        const float wv = w[k];
#pragma unroll
        for (int f = 0; f < FEAT_TF; ++f) acc[f] = fmaf(wv, amp[f * F + k], acc[f]);
      }
    } else {
#pragma unroll
      for (int f = 0; f < FEAT_TF; ++f) acc[f] = amp[f * F + c];
    }
    const float sc = scale[c], of = offset[c];
#pragma unroll
    for (int f = 0; f < FEAT_TF; ++f)
      if (f < nfr)
        out[((size_t)b * M_max + t0 + f) * C + c] =
            t0 + f < M ? stft::feature(acc[f], gain, sc, of, clip_lo, clip_hi, use_clip) : 0.f;
  }
}

}  // namespace

void launch_stft_frames(bool fft, const float* wav, long L_max, const RowInts& nsamp, int B, int M_max, int n_fft,
                        int hop, int wlo, int whi, float preemph, const float* W, const float* win, float* out,
                        hipStream_t s) {
  const dim3 grid(M_max, B);
  const float2* W2 = reinterpret_cast<const float2*>(W);
  if (fft) {
    stft_frame_kernel<<<grid, LANES, 0, s>>>(wav, L_max, nsamp, W2, win, M_max, hop, wlo, whi, preemph, out);
  } else {
    const size_t lds = (size_t)n_fft * (sizeof(float2) + sizeof(float));
    dft_frame_kernel<<<grid, DFT_THREADS, lds, s>>>(wav, L_max, nsamp, W2, win, M_max, n_fft, hop, wlo, whi, preemph,
                                                    out);
  }
  HIP_OK(hipGetLastError());
}

void launch_mag_to_feature(const float* mag, const RowInts& lens, int B, int M_max, int F, int C, const float* basis,
                           float gain, const float* scale, const float* offset, float clip_lo, float clip_hi,
                           int use_clip, float* out, hipStream_t s) {
  mag_to_feature_kernel<<<dim3((M_max + FEAT_TF - 1) / FEAT_TF, B), FEAT_THREADS, FEAT_TF * F * sizeof(float), s>>>(
      mag, lens, M_max, F, C, basis, gain, scale, offset, clip_lo, clip_hi, use_clip, out);
  HIP_OK(hipGetLastError());
}
