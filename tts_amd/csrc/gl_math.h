// Per-frame arithmetic of the Griffin-Lim kernels (griffin_lim.hip): a 1024-point real FFT as a
// 512-point complex FFT of z[n] = x[2n] + i x[2n+1], three radix-8 Stockham passes over one LDS
// buffer, 64 lanes x 8 points. Every function is the work of ONE lane `j` of the frame's wave
// between two barriers, so the same code runs lane by lane on the host.
#pragma once
#include <hip/hip_runtime.h>

#define GL_HD __host__ __device__ __forceinline__

namespace gl {

constexpr int NFFT = 1024, NH = NFFT / 2, NBIN = NH + 1, LANES = 64, CENTER = NFFT / 2;
// LDS image of the 512 complex points: one pad slot per 8, so that the stride-8 and stride-64
// stores of the Stockham passes (ds_write_b64, 16-lane groups) and the unit-stride loads each
// touch every bank once
constexpr int BUF = NH + NH / 8;
GL_HD int phys(int i) { return i + (i >> 3); }

GL_HD float2 cmul(float2 a, float2 b) { return float2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// SIGN = -1: forward transform (e^{-i...}), +1: inverse (unnormalised)
GL_HD void bfly(float2& a, float2& b) {
  const float2 t = a;
  a = float2{t.x + b.x, t.y + b.y};
  b = float2{t.x - b.x, t.y - b.y};
}
template <int SIGN>
GL_HD float2 mul_si(float2 a) {  // a * (SIGN i)
  return SIGN > 0 ? float2{-a.y, a.x} : float2{a.y, -a.x};
}
template <int SIGN>
GL_HD void fft4(float2& a0, float2& a1, float2& a2, float2& a3) {  // out: a0, a2, a1, a3 = X0..X3
  bfly(a0, a2);
  bfly(a1, a3);
  a3 = mul_si<SIGN>(a3);
  bfly(a0, a1);
  bfly(a2, a3);
}
// 8-point DFT in place; X[k] is left in v[rev3(k)]
template <int SIGN>
GL_HD void fft8(float2* v) {
  constexpr float R = 0.70710678118654752440f, s = (float)SIGN;
  bfly(v[0], v[4]);
  bfly(v[1], v[5]);
  bfly(v[2], v[6]);
  bfly(v[3], v[7]);
  v[5] = float2{R * (v[5].x - s * v[5].y), R * (s * v[5].x + v[5].y)};    // * (1 + s i) / sqrt 2
  v[6] = mul_si<SIGN>(v[6]);
  v[7] = float2{R * (-v[7].x - s * v[7].y), R * (s * v[7].x - v[7].y)};   // * (-1 + s i) / sqrt 2
  fft4<SIGN>(v[0], v[1], v[2], v[3]);
  fft4<SIGN>(v[4], v[5], v[6], v[7]);
}

// One Stockham pass (Ns = 1, 8, 64): lane j takes points j + 64 r, twiddles them by
// e^{SIGN 2 pi i r k / (8 Ns)}, k = j mod Ns, and transforms; W[m] = e^{-2 pi i m / 1024}.
// The loads of all lanes come before the stores of any (a barrier between the two).
template <int SIGN>
GL_HD void fft512_load(const float2* buf, const float2* __restrict__ W, int Ns, int j, float2* v) {
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[phys(j + LANES * r)];
  if (Ns > 1) {
    const int step = (NFFT / (8 * Ns)) * (j & (Ns - 1));
#pragma unroll
    for (int r = 1; r < 8; ++r) {
      float2 w = W[r * step];
      if (SIGN > 0) w.y = -w.y;
      v[r] = cmul(v[r], w);
    }
  }
  fft8<SIGN>(v);
}
GL_HD void fft512_store(float2* buf, int Ns, int j, const float2* v) {
  const int k = j & (Ns - 1), j0 = (j - k) * 8 + k;
  buf[phys(j0)] = v[0];
  buf[phys(j0 + Ns)] = v[4];
  buf[phys(j0 + 2 * Ns)] = v[2];
  buf[phys(j0 + 3 * Ns)] = v[6];
  buf[phys(j0 + 4 * Ns)] = v[1];
  buf[phys(j0 + 5 * Ns)] = v[5];
  buf[phys(j0 + 6 * Ns)] = v[3];
  buf[phys(j0 + 7 * Ns)] = v[7];
}

// x / |x|, 1 + 0i for x == 0 (np.angle(0) == 0); scaled by the larger part first, so that no
// nonzero bin squares to zero or infinity
GL_HD float2 unit(float2 x) {
  const float m = fmaxf(fabsf(x.x), fabsf(x.y));
  if (!(m > 0.f)) return float2{1.f, 0.f};
  const float a = x.x / m, b = x.y / m, r = 1.0f / sqrtf(a * a + b * b);
  return float2{a * r, b * r};
}
GL_HD float2 cis2pi(float u) {  // e^{2 pi i u}
  float s, c;
#ifdef __HIP_DEVICE_COMPILE__
  sincospif(2.f * u, &s, &c);
#else
  s = (float)sin(2.0 * M_PI * (double)u);
  c = (float)cos(2.0 * M_PI * (double)u);
#endif
  return float2{c, s};
}

// The spectral step of one frame, on the half-size transform's own points. START = false: buf
// holds Z = FFT512(z); bins X[k] = E[k] + W^k O[k] (E, O the transforms of the even and odd
// samples) are projected to modulus S[k]. START = true: the bins are S[k] e^{2 pi i u[k]} (the
// imaginary parts of bins 0 and 512 dropped, as a complex-to-real transform does). Either way
// buf is left holding Z' with IFFT512(Z') / 1024 = the frame's samples, pairwise.
// Lane j owns the bin pairs (k, 512 - k), k = 1 + j + 64 m, and lane 0 also bins 0 and 512.
template <bool START>
GL_HD void project(float2* buf, const float2* __restrict__ W, const float* __restrict__ S,
                   const float* __restrict__ u, int j) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int k = 1 + j + LANES * m, kn = NH - k;
    const float2 w = W[k];
    float2 Xk, Xn;
    if (!START) {
      const float2 Zk = buf[phys(k)], Zn = buf[phys(kn)];
      const float2 E = float2{Zk.x + Zn.x, Zk.y - Zn.y};   // Zk + conj Zn      (2 E)
      const float2 O = float2{Zk.y + Zn.y, Zn.x - Zk.x};   // -i (Zk - conj Zn) (2 O)
      const float2 T = cmul(w, O);
      Xk = unit(float2{E.x + T.x, E.y + T.y});
      Xn = unit(float2{E.x - T.x, T.y - E.y});             // conj(E - T)
    } else {
      Xk = cis2pi(u[k]);
      Xn = cis2pi(u[kn]);
    }
    const float sk = S[k], sn = S[kn];
    Xk = float2{Xk.x * sk, Xk.y * sk};
    Xn = float2{Xn.x * sn, Xn.y * sn};
    const float2 E2 = float2{Xk.x + Xn.x, Xk.y - Xn.y};    // Xk + conj Xn
    const float2 D2 = float2{Xk.x - Xn.x, Xk.y + Xn.y};    // Xk - conj Xn
    const float2 O2 = cmul(D2, float2{w.x, -w.y});
    buf[phys(k)] = float2{E2.x - O2.y, E2.y + O2.x};       // E2 + i O2
    buf[phys(kn)] = float2{E2.x + O2.y, O2.x - E2.y};      // conj E2 + i conj O2
  }
  if (j == 0) {
    float x0, xh;
    if (!START) {
      const float2 Z0 = buf[0];
      x0 = (Z0.x + Z0.y) < 0.f ? -1.f : 1.f;
      xh = (Z0.x - Z0.y) < 0.f ? -1.f : 1.f;
    } else {
      x0 = cis2pi(u[0]).x;
      xh = cis2pi(u[NH]).x;
    }
    x0 *= S[0];
    xh *= S[NH];
    buf[0] = float2{x0 + xh, x0 - xh};
  }
}

// Sample q (0 <= q < hop (M - 1)) of a row's signal: the overlap-add of the windowed frames that
// cover it, divided by the window-square envelope where that exceeds 1e-11, after the centre trim.
// Only frames whose window support [wlo, whi) holds the sample are read (the rest of a frame is 0).
GL_HD float ola_sample(const float* __restrict__ F, const float* __restrict__ env, int M, int hop, int wlo,
                       int whi, int q) {
  const int p = q + CENTER, num = p - whi + 1;
  const int t0 = num <= 0 ? 0 : (num + hop - 1) / hop;
  int t1 = (p - wlo) / hop;
  t1 = t1 < M - 1 ? t1 : M - 1;
  float s = 0.f;
  for (int t = t0; t <= t1; ++t) s += F[(size_t)t * NFFT + (p - t * hop)];
  const float e = env[p];
  return e > 1e-11f ? s / e : s;
}
// index q of torch.stft's reflect padding back into [0, L)
GL_HD int reflect(int q, int L) {
  q = q < 0 ? -q : q;
  return q >= L ? 2 * (L - 1) - q : q;
}

// Frame t of the next STFT: windowed samples of the reflect-padded signal, pairwise into buf
GL_HD void gather(float2* buf, const float* __restrict__ F, const float* __restrict__ env,
                  const float* __restrict__ win, int M, int hop, int wlo, int whi, int t, int j) {
  const int L = hop * (M - 1);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = j + LANES * r, q = t * hop + 2 * n - CENTER;
    float2 x = float2{0.f, 0.f};
    if (2 * n + 1 >= wlo && 2 * n < whi) {
      const float2 w = reinterpret_cast<const float2*>(win)[n];
      x.x = w.x * ola_sample(F, env, M, hop, wlo, whi, reflect(q, L));
      x.y = w.y * ola_sample(F, env, M, hop, wlo, whi, reflect(q + 1, L));
    }
    buf[phys(n)] = x;
  }
}
// The frame's samples times the window into the frame buffer
GL_HD void scatter(const float2* buf, float* __restrict__ out, const float* __restrict__ win, int j) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = j + LANES * r;
    const float2 z = buf[phys(n)], w = reinterpret_cast<const float2*>(win)[n];
    reinterpret_cast<float2*>(out)[n] = float2{w.x * (z.x * (1.f / NFFT)), w.y * (z.y * (1.f / NFFT))};
  }
}

}  // namespace gl
