// Per-frame arithmetic of the analysis kernels (stft.hip): the forward half of gl_math.h. A frame's
// samples come straight from the caller's waveform row (reflect padding, pre-emphasis and window
// applied on the fly); n_fft = 1024 goes through gl_math.h's 512-point complex FFT and the even/odd
// split, every other n_fft through a direct DFT over a twiddle table. As in gl_math.h every
// function is the work of ONE lane between two barriers, so the same code runs on the host.
#pragma once
#include "gl_math.h"

namespace stft {

// sample q (0 <= q < L) of the pre-emphasised row, lfilter([1, -a], [1], y): y[q] - a y[q-1], y[-1] = 0
GL_HD float sample(const float* __restrict__ y, int q, float a) {
  const float v = y[q];
  return (a != 0.f && q > 0) ? fmaf(-a, y[q - 1], v) : v;
}

// windowed sample n of frame t: the signal is pre-emphasised, then reflect-padded by n_fft / 2
// (L > n_fft / 2, so one reflection reaches [0, L)); win is the window zero-padded to n_fft
GL_HD float frame_sample(const float* __restrict__ y, int L, const float* __restrict__ win, int half, int hop,
                         float a, int t, int n) {
  return win[n] * sample(y, gl::reflect(t * hop + n - half, L), a);
}

// n_fft = 1024: lane j's 8 sample pairs of frame t into the FFT buffer, z[n] = x[2n] + i x[2n+1];
// pairs outside the window's support [wlo, whi) are zero and read nothing
GL_HD void gather1024(float2* buf, const float* __restrict__ y, int L, const float* __restrict__ win, int hop,
                      int wlo, int whi, float a, int t, int j) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = j + gl::LANES * r;
    float2 x = float2{0.f, 0.f};
    if (2 * n + 1 >= wlo && 2 * n < whi) {
      x.x = frame_sample(y, L, win, gl::CENTER, hop, a, t, 2 * n);
      x.y = frame_sample(y, L, win, gl::CENTER, hop, a, t, 2 * n + 1);
    }
    buf[gl::phys(n)] = x;
  }
}

GL_HD float mag(float re, float im) { return sqrtf(re * re + im * im); }

// buf holds Z = FFT512(z). X[k] = E[k] + W^k O[k] with E, O the transforms of the even and odd
// samples (gl::project's split): lane j writes |X| of the bin pairs (k, 512 - k), k = 1 + j + 64 m,
// lane 0 also bins 0 and 512. W[m] = e^{-2 pi i m / 1024}.
GL_HD void split_mag(const float2* buf, const float2* __restrict__ W, float* __restrict__ out, int j) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int k = 1 + j + gl::LANES * m, kn = gl::NH - k;
    const float2 Zk = buf[gl::phys(k)], Zn = buf[gl::phys(kn)];
    const float2 E = float2{Zk.x + Zn.x, Zk.y - Zn.y};   // Zk + conj Zn      (2 E)
    const float2 O = float2{Zk.y + Zn.y, Zn.x - Zk.x};   // -i (Zk - conj Zn) (2 O)
    const float2 T = gl::cmul(W[k], O);
    out[k] = 0.5f * mag(E.x + T.x, E.y + T.y);
    if (kn != k) out[kn] = 0.5f * mag(E.x - T.x, T.y - E.y);
  }
  if (j == 0) {
    const float2 Z0 = buf[0];
    out[0] = fabsf(Z0.x + Z0.y);
    out[gl::NH] = fabsf(Z0.x - Z0.y);
  }
}

// |X[k]| of the N-point DFT of the windowed frame x, summed over the window's support only.
// tab[m] = e^{-2 pi i m / N}; its index (k n) mod N is carried as an integer (k < N, so one
// subtraction per step reduces it). Four interleaved partial sums keep the rounding error of a
// long window near that of a blocked sum.
GL_HD float dft_bin(const float* x, const float2* tab, int N, int wlo, int whi, int k) {
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  int idx = (int)(((long)k * wlo) % N);
  int n = wlo;
  for (; n + 4 <= whi; n += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float2 w = tab[idx];
      const float v = x[n + u];
      re[u] = fmaf(v, w.x, re[u]);
      im[u] = fmaf(v, w.y, im[u]);
      idx += k;
      idx -= idx >= N ? N : 0;
    }
  }
  for (; n < whi; ++n) {
    const float2 w = tab[idx];
    re[0] = fmaf(x[n], w.x, re[0]);
    im[0] = fmaf(x[n], w.y, im[0]);
    idx += k;
    idx -= idx >= N ? N : 0;
  }
  return mag((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
}

// one feature value: dB of the (floored) magnitude, then the per-channel affine normalisation
GL_HD float feature(float X, float gain, float scale, float offset, float clip_lo, float clip_hi, int use_clip) {
  float v = fmaf(gain * log10f(fmaxf(1e-5f, X)), scale, offset);
  if (use_clip) v = fminf(fmaxf(v, clip_lo), clip_hi);
  return v;
}

}  // namespace stft
