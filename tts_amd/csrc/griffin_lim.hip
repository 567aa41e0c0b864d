// Batched Griffin-Lim (TTS/utils/audio.py:259-279 on librosa.stft / istft conventions) and the
// mel -> linear magnitude step before it (audio.py:213-214, 241-248). fp32, n_fft = 1024.
//
// One wave per STFT frame. A Griffin-Lim iteration is one launch: the wave of frame t gathers its
// 1024 samples by overlap-add from the previous iteration's windowed frames (envelope division,
// centre trim and reflect padding applied on the fly), transforms them, projects every bin onto
// the target magnitude, transforms back and writes its windowed frame into the other frame
// buffer. No spectrum and no waveform is written between iterations. gl_math.h holds the
// arithmetic; the kernels here only place it between barriers.
#include "common.h"
#include "gl_math.h"
#include "launch.h"

namespace {

using namespace gl;

// in-place 512-point complex FFT of the wave's LDS buffer
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

// grid (M_max, B), 64 threads. START: frames of S e^{2 pi i u}; else one Griffin-Lim iteration
// from the frames in Fin. Frames t >= lens[b] are neither read nor written.
template <bool START>
__global__ void __launch_bounds__(LANES) gl_frame_kernel(const float* __restrict__ S, const float* __restrict__ u,
                                                         const float* __restrict__ Fin, float* __restrict__ Fout,
                                                         const float* __restrict__ env, const float2* __restrict__ W,
                                                         const float* __restrict__ win, RowInts lens, int M_max,
                                                         int hop, int wlo, int whi, long env_stride) {
  __shared__ float2 buf[BUF];
  const int t = blockIdx.x, b = blockIdx.y, j = threadIdx.x, M = lens.v[b];
  if (t >= M) return;
  const size_t row = (size_t)b * M_max, fr = row + t;
  if (!START) {
    gather(buf, Fin + row * NFFT, env + b * env_stride, win, M, hop, wlo, whi, t, j);
    __syncthreads();
    fft512<-1>(buf, W, j);
  }
  project<START>(buf, W, S + fr * NBIN, START ? u + fr * NBIN : nullptr, j);
  __syncthreads();
  fft512<1>(buf, W, j);
  scatter(buf, Fout + fr * NFFT, win, j);
}

// window-square envelope of each row's overlap-add, over the padded signal: grid (ceil(P/256), B)
__global__ void gl_env_kernel(float* __restrict__ env, const float* __restrict__ win, RowInts lens, int hop, int wlo,
                              int whi, long env_stride) {
  const int b = blockIdx.y, M = lens.v[b];
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long)hop * (M - 1) + NFFT) return;
  const int num = (int)p - whi + 1;
  const int t0 = num <= 0 ? 0 : (num + hop - 1) / hop;
  int t1 = p < wlo ? -1 : ((int)p - wlo) / hop;
  t1 = t1 < M - 1 ? t1 : M - 1;
  float e = 0.f;
  for (int t = t0; t <= t1; ++t) {
    const float w = win[p - (long)t * hop];
    e += w * w;
  }
  env[b * env_stride + p] = e;
}

// the last overlap-add: wav (B, Lmax), row b zero past hop (lens[b] - 1)
__global__ void gl_finish_kernel(const float* __restrict__ F, const float* __restrict__ env, float* __restrict__ wav,
                                 RowInts lens, int M_max, int hop, int wlo, int whi, long env_stride, int Lmax) {
  const int b = blockIdx.y, M = lens.v[b];
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Lmax) return;
  float y = 0.f;
  if (q < hop * (M - 1)) y = ola_sample(F + (size_t)b * M_max * NFFT, env + b * env_stride, M, hop, wlo, whi, q);
  wav[(size_t)b * Lmax + q] = y;
}

// S = max(1e-10, inv_basis @ 10^((clip(mel) scale + offset) / gain)) ^ power on MEL_TF frames per
// block: the frames' amplitudes in LDS, each thread one bin of all the frames (plain FMA: 513 x 80)
constexpr int MEL_TF = 8, MEL_THREADS = 256;
__global__ void __launch_bounds__(MEL_THREADS)
    mel_to_linear_kernel(const float* __restrict__ mel, RowInts lens, int M_max, int n_mels, int F,
                         const float* __restrict__ inv, const float* __restrict__ scale,
                         const float* __restrict__ offset, float clip_lo, float clip_hi, int use_clip, float gain,
                         float power, float* __restrict__ S) {
  extern __shared__ float amp[];  // [MEL_TF][n_mels]
  const int b = blockIdx.y, t0 = blockIdx.x * MEL_TF, M = lens.v[b];
  const int nfr = min(MEL_TF, M_max - t0);
  for (int i = threadIdx.x; i < MEL_TF * n_mels; i += MEL_THREADS) {
    const int f = i / n_mels, m = i - f * n_mels;
    float a = 0.f;
    if (t0 + f < M) {
      float x = mel[((size_t)b * M_max + t0 + f) * n_mels + m];
      if (use_clip) x = fminf(fmaxf(x, clip_lo), clip_hi);
      a = powf(10.f, (x * scale[m] + offset[m]) / gain);
    }
    amp[i] = a;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < F; k += MEL_THREADS) {
    float acc[MEL_TF] = {};
    const float* w = inv + (size_t)k * n_mels;
    for (int m = 0; m < n_mels; ++m) {
      const float wv = w[m];
#pragma unroll
      for (int f = 0; f < MEL_TF; ++f) acc[f] = fmaf(wv, amp[f * n_mels + m], acc[f]);
    }
    for (int f = 0; f < nfr; ++f)
      S[((size_t)b * M_max + t0 + f) * F + k] = t0 + f < M ? powf(fmaxf(1e-10f, acc[f]), power) : 0.f;
  }
}

}  // namespace

void launch_gl_env(float* env, const float* win, const RowInts& lens, int B, int M_max, int hop, int wlo, int whi,
                   long env_stride, hipStream_t s) {
  const long P = (long)hop * (M_max - 1) + gl::NFFT;
  gl_env_kernel<<<dim3((unsigned)((P + 255) / 256), B), 256, 0, s>>>(env, win, lens, hop, wlo, whi, env_stride);
  HIP_OK(hipGetLastError());
}

void launch_gl_frames(bool start, const float* S, const float* u, const float* Fin, float* Fout, const float* env,
                      const float* W, const float* win, const RowInts& lens, int B, int M_max, int hop, int wlo,
                      int whi, long env_stride, hipStream_t s) {
  const dim3 grid(M_max, B);
  const float2* W2 = reinterpret_cast<const float2*>(W);
  if (start)
    gl_frame_kernel<true><<<grid, LANES, 0, s>>>(S, u, nullptr, Fout, env, W2, win, lens, M_max, hop, wlo, whi,
                                                 env_stride);
  else
    gl_frame_kernel<false><<<grid, LANES, 0, s>>>(S, nullptr, Fin, Fout, env, W2, win, lens, M_max, hop, wlo, whi,
                                                  env_stride);
  HIP_OK(hipGetLastError());
}

void launch_gl_finish(const float* F, const float* env, float* wav, const RowInts& lens, int B, int M_max, int hop,
                      int wlo, int whi, long env_stride, hipStream_t s) {
  const int Lmax = hop * (M_max - 1);
  if (Lmax <= 0) return;
  gl_finish_kernel<<<dim3((Lmax + 255) / 256, B), 256, 0, s>>>(F, env, wav, lens, M_max, hop, wlo, whi, env_stride,
                                                               Lmax);
  HIP_OK(hipGetLastError());
}

void launch_mel_to_linear(const float* mel, const RowInts& lens, int B, int M_max, int n_mels, int F, const float* inv,
                          const float* scale, const float* offset, float clip_lo, float clip_hi, int use_clip,
                          float spec_gain, float power, float* S, hipStream_t s) {
  mel_to_linear_kernel<<<dim3((M_max + MEL_TF - 1) / MEL_TF, B), MEL_THREADS, MEL_TF * n_mels * sizeof(float), s>>>(
      mel, lens, M_max, n_mels, F, inv, scale, offset, clip_lo, clip_hi, use_clip, spec_gain, power, S);
  HIP_OK(hipGetLastError());
}
