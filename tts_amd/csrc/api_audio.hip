// Audio post-processing entry points: mel -> linear magnitudes and batched Griffin-Lim
// (griffin_lim.hip), the waveform tail, linear spectrogram -> magnitudes, de-emphasis and the 16-bit
// join (wav_tail.hip), and the analysis direction, waveform -> STFT magnitudes -> normalised
// features (stft.hip). All of them only enqueue work: no host synchronisation, no graph capture.
#include "host.h"

#include <cmath>

using namespace ttsh;

namespace {

// The frame of a stream-asynchronous entry point: argument checks before anything touches a
// device or a stream, then the work on c->s between the two stream joins.
template <class Pre, class F>
int async_call(tts_ctx* c, void* stream, Pre&& pre, F&& fn) {
  return guarded_ctx(c, [&] {
    pre();
    DeviceGuard g(c->device);
    enter(c, stream);
    fn();
    leave(c, stream);
  });
}

// twiddles e^{-2 pi i m / 1024} and the periodic Hann window of win_length points, centred in
// 1024 as torch.stft pads it; computed in double, uploaded once per win_length
void gl_tables(tts_ctx* c, int win_length) {
  AudioWS& A = c->aws;
  if (A.win_length == win_length) return;
  const int N = 1024;
  if (!A.W.p) {
    std::vector<float> W(2 * N);
    for (int m = 0; m < N; ++m) {
      W[2 * m] = (float)std::cos(-2.0 * M_PI * m / N);
      W[2 * m + 1] = (float)std::sin(-2.0 * M_PI * m / N);
    }
    A.W.upload(W);
  }
  std::vector<float> win(N, 0.f);
  const int lo = (N - win_length) / 2;
  for (int n = 0; n < win_length; ++n) win[lo + n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / win_length));
  HIP_OK(hipStreamSynchronize(c->s));  // a queued call may still read the previous window
  A.win.upload(win);
  A.win_length = win_length;
}

// the analysis side's tables: twiddles e^{-2 pi i m / n_fft} (uploaded once per n_fft) and the
// periodic Hann window of win_length points centred in n_fft; computed in double
void stft_tables(tts_ctx* c, int n_fft, int win_length) {
  AudioWS& A = c->aws;
  if (A.s_nfft == n_fft && A.s_win == win_length) return;
  HIP_OK(hipStreamSynchronize(c->s));  // a queued call may still read the previous tables
  if (A.s_nfft != n_fft) {
    std::vector<float> W(2 * (size_t)n_fft);
    for (int m = 0; m < n_fft; ++m) {
      W[2 * m] = (float)std::cos(-2.0 * M_PI * m / n_fft);
      W[2 * m + 1] = (float)std::sin(-2.0 * M_PI * m / n_fft);
    }
    A.s_nfft = A.s_win = -1;
    A.sW.upload(W);
  }
  std::vector<float> win(n_fft, 0.f);
  const int lo = (n_fft - win_length) / 2;
  for (int n = 0; n < win_length; ++n) win[lo + n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / win_length));
  A.swin.upload(win);
  A.s_nfft = n_fft;
  A.s_win = win_length;
}

}  // namespace

extern "C" {

int tts_stft_mag(tts_ctx* c, const float* d_wav, const int32_t* h_nsamples, int B, int L_max, int n_fft,
                 int win_length, int hop_length, float preemphasis, int algo, float* d_mag, int M_max, void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_wav && h_nsamples && d_mag, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "stft_mag: 1 <= B <= 64");
        TTS_CHECK(n_fft >= 64 && n_fft <= 2048 && n_fft % 2 == 0, "stft_mag: n_fft must be even and in [64, 2048]");
        TTS_CHECK(win_length >= 1 && win_length <= n_fft, "stft_mag: win_length outside [1, n_fft]");
        TTS_CHECK(hop_length >= 16 && hop_length <= n_fft, "stft_mag: hop_length outside [16, n_fft]");
        TTS_CHECK(algo >= 0 && algo <= 2, "stft_mag: algo must be 0 (auto), 1 (FFT) or 2 (direct)");
        TTS_CHECK(algo != 1 || n_fft == 1024, "stft_mag: algo 1 (FFT) needs n_fft == 1024");
        TTS_CHECK(std::isfinite(preemphasis), "stft_mag: preemphasis must be finite");
        TTS_CHECK(L_max >= 1 && L_max < (1 << 30) && M_max >= 1, "stft_mag: L_max or M_max out of range");
        for (int b = 0; b < B; ++b)
          TTS_CHECK(h_nsamples[b] > n_fft / 2 && h_nsamples[b] <= L_max && 1 + h_nsamples[b] / hop_length <= M_max,
                    "stft_mag: every row needs n_fft / 2 < h_nsamples[b] <= L_max (the reflect padding of "
                    "torch.stft) and 1 + h_nsamples[b] / hop_length <= M_max");
      },
      [&] {
        AudioWS& A = c->aws;
        stft_tables(c, n_fft, win_length);
        const int wlo = (n_fft - win_length) / 2, whi = wlo + win_length;
        launch_stft_frames(n_fft == 1024 && algo != 2, d_wav, L_max, row_ints(h_nsamples, B), B, M_max, n_fft,
                           hop_length, wlo, whi, preemphasis, A.sW.f(), A.swin.f(), d_mag, c->s);
      });
}

int tts_mag_to_feature(tts_ctx* c, const float* d_mag, const int32_t* h_lens, int B, int M_max, int n_freq, int n_out,
                       const float* d_basis, float spec_gain, const float* d_scale, const float* d_offset,
                       float clip_lo, float clip_hi, int use_clip, float* d_out, void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_mag && h_lens && d_scale && d_offset && d_out, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "mag_to_feature: 1 <= B <= 64");
        TTS_CHECK(M_max >= 1, "mag_to_feature: M_max must be positive");
        TTS_CHECK(n_freq >= 1 && n_freq <= 1025, "mag_to_feature: 1 <= n_freq <= 1025");
        TTS_CHECK(n_out >= 1 && n_out <= 1025, "mag_to_feature: 1 <= n_out <= 1025");
        TTS_CHECK(d_basis || n_out == n_freq, "mag_to_feature: without a basis n_out must equal n_freq");
        check_rows(h_lens, B, 0, M_max, "mag_to_feature: h_lens[b] outside [0, M_max]");
      },
      [&] {
        launch_mag_to_feature(d_mag, row_ints(h_lens, B), B, M_max, n_freq, n_out, d_basis, spec_gain, d_scale,
                              d_offset, clip_lo, clip_hi, use_clip, d_out, c->s);
      });
}


int tts_mel_to_linear(tts_ctx* c, const float* d_mel, const int32_t* h_lens, int B, int M_max, int n_mels, int n_freq,
                      const float* d_inv_basis, const float* d_scale, const float* d_offset, float clip_lo,
                      float clip_hi, int use_clip, float spec_gain, float power, float* d_S, void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_mel && h_lens && d_inv_basis && d_scale && d_offset && d_S, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "mel_to_linear: 1 <= B <= 64");
        TTS_CHECK(M_max >= 1 && n_freq >= 1, "mel_to_linear: M_max and n_freq must be positive");
        TTS_CHECK(n_mels >= 1 && n_mels <= 512, "mel_to_linear: 1 <= n_mels <= 512");
        TTS_CHECK(spec_gain != 0.f, "mel_to_linear: spec_gain must not be 0");
        check_rows(h_lens, B, 0, M_max, "mel_to_linear: h_lens[b] outside [0, M_max]");
      },
      [&] {
        launch_mel_to_linear(d_mel, row_ints(h_lens, B), B, M_max, n_mels, n_freq, d_inv_basis, d_scale, d_offset,
                             clip_lo, clip_hi, use_clip, spec_gain, power, d_S, c->s);
      });
}

int tts_griffin_lim(tts_ctx* c, const float* d_S, const int32_t* h_lens, int B, int M_max, int n_fft, int win_length,
                    int hop_length, int iters, const float* d_phase0, float* d_wav, void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_S && h_lens && d_phase0 && d_wav, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "griffin_lim: 1 <= B <= 64");
        TTS_CHECK(n_fft == 1024, "griffin_lim: n_fft must be 1024");
        TTS_CHECK(win_length >= 1 && win_length <= n_fft, "griffin_lim: win_length outside [1, 1024]");
        TTS_CHECK(hop_length >= 64 && hop_length <= 512, "griffin_lim: hop_length outside [64, 512]");
        TTS_CHECK(iters >= 0, "griffin_lim: iters must be >= 0");
        TTS_CHECK(M_max >= 1 && (long)hop_length * M_max < (1L << 30), "griffin_lim: M_max out of range");
        for (int b = 0; b < B; ++b)
          TTS_CHECK(h_lens[b] >= 1 && h_lens[b] <= M_max && hop_length * (h_lens[b] - 1) > n_fft / 2,
                    "griffin_lim: every row needs h_lens[b] <= M_max and hop_length * (h_lens[b] - 1) > n_fft / 2 "
                    "(the reflect padding of torch.stft)");
      },
      [&] {
        AudioWS& A = c->aws;
        gl_tables(c, win_length);
        const size_t frames = (size_t)B * M_max * 1024 * sizeof(float);
        const long env_stride = (long)hop_length * (M_max - 1) + 1024;
        A.fa.ensure(frames);
        A.fb.ensure(frames);
        A.env.ensure((size_t)B * env_stride * sizeof(float));
        const RowInts L = row_ints(h_lens, B);
        const int wlo = (1024 - win_length) / 2, whi = wlo + win_length;
        float *cur = A.fa.f(), *nxt = A.fb.f();
        launch_gl_env(A.env.f(), A.win.f(), L, B, M_max, hop_length, wlo, whi, env_stride, c->s);
        launch_gl_frames(true, d_S, d_phase0, nullptr, cur, A.env.f(), A.W.f(), A.win.f(), L, B, M_max, hop_length, wlo,
                         whi, env_stride, c->s);
        for (int i = 0; i < iters; ++i) {
          launch_gl_frames(false, d_S, nullptr, cur, nxt, A.env.f(), A.W.f(), A.win.f(), L, B, M_max, hop_length, wlo,
                           whi, env_stride, c->s);
          std::swap(cur, nxt);
        }
        launch_gl_finish(cur, A.env.f(), d_wav, L, B, M_max, hop_length, wlo, whi, env_stride, c->s);
      });
}

int tts_spec_to_mag(tts_ctx* c, const float* d_spec, const int32_t* h_lens, int B, int M_max, int n_freq,
                    const float* d_scale, const float* d_offset, float clip_lo, float clip_hi, int use_clip,
                    float spec_gain, float power, float* d_S, void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_spec && h_lens && d_scale && d_offset && d_S, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "spec_to_mag: 1 <= B <= 64");
        TTS_CHECK(n_freq >= 1 && n_freq <= 1025, "spec_to_mag: 1 <= n_freq <= 1025");
        TTS_CHECK(M_max >= 1 && (long)M_max * n_freq < (1L << 30), "spec_to_mag: M_max out of range");
        TTS_CHECK(spec_gain != 0.f, "spec_to_mag: spec_gain must not be 0");
        check_rows(h_lens, B, 0, M_max, "spec_to_mag: h_lens[b] outside [0, M_max]");
      },
      [&] {
        launch_spec_to_mag(d_spec, row_ints(h_lens, B), B, M_max, n_freq, d_scale, d_offset, clip_lo, clip_hi,
                           use_clip, spec_gain, power, d_S, c->s);
      });
}

int tts_deemphasis(tts_ctx* c, const float* d_in, const int32_t* h_nsamples, int B, int L_max, double a, float* d_out,
                   void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_in && h_nsamples && d_out, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "deemphasis: 1 <= B <= 64");
        TTS_CHECK(a > 0.0 && a < 1.0, "deemphasis: the coefficient a must be in (0, 1)");
        TTS_CHECK(L_max >= 1 && L_max < (1 << 30), "deemphasis: L_max out of range");
        check_rows(h_nsamples, B, 0, L_max, "deemphasis: h_nsamples[b] outside [0, L_max]");
      },
      [&] {
        DeemphTable tab;
        for (int k = 0; k <= DE_C; ++k) tab.pw[k] = (float)std::pow(a, (double)k);
        for (int s = 0; s < DE_LOG; ++s) tab.pwc[s] = (float)std::pow(a, (double)(DE_C << s));
        launch_deemphasis(d_in, d_out, row_ints(h_nsamples, B), B, L_max, tab, c->s);
      });
}

int tts_wav_finish(tts_ctx* c, const float* d_wav, const int32_t* h_nsamples, int B, int L_max, int window_length,
                   int hop_length, double threshold, int gap, int16_t* d_pcm, int32_t* d_ends, int32_t* d_total,
                   void* stream) {
  return async_call(
      c, stream,
      [&] {
        TTS_CHECK(d_wav && h_nsamples && d_pcm && d_ends && d_total, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "wav_finish: 1 <= B <= 64");
        TTS_CHECK(L_max >= 1 && L_max < (1 << 30), "wav_finish: L_max out of range");
        TTS_CHECK(hop_length >= 1 && window_length >= hop_length && window_length / hop_length <= 64,
                  "wav_finish: needs 1 <= hop_length <= window_length and window_length / hop_length <= 64");
        TTS_CHECK(window_length < (1 << 30), "wav_finish: window_length out of range");
        TTS_CHECK(!std::isnan(threshold), "wav_finish: threshold is NaN");
        TTS_CHECK(gap >= 0 && gap < (1 << 24), "wav_finish: gap outside [0, 2^24)");
        check_rows(h_nsamples, B, 0, L_max, "wav_finish: h_nsamples[b] outside [0, L_max]");
        long cap = 0;
        for (int b = 0; b < B; ++b) cap += (long)h_nsamples[b] + gap;
        TTS_CHECK(cap < (1L << 31), "wav_finish: the joined signal would pass 2^31 samples");
      },
      [&] {
        AudioWS& A = c->aws;
        const int nblk = (L_max + hop_length - 1) / hop_length;
        const size_t maxima = (size_t)B * nblk;
        A.tail.ensure((2 * maxima + BMAX + 1) * sizeof(float));
        float* smax = A.tail.f();
        float* amax = smax + maxima;
        int* offs = reinterpret_cast<int*>(amax + maxima);
        float* factor = reinterpret_cast<float*>(offs + BMAX);
        launch_wav_finish(d_wav, row_ints(h_nsamples, B), B, L_max, window_length, hop_length, threshold, gap, smax,
                          amax, nblk, offs, factor, d_pcm, d_ends, d_total, c->s);
      });
}

}  // extern "C"
