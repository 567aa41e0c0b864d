// Vocoder scoring entry points (voc_eval.hip): PQMF analysis, the paired STFT distance sums of
// STFTLoss and the magnitudes of TorchSTFT. All of them only enqueue work: no host synchronisation
// (but for the first use of a DFT basis, which uploads it), no graph capture.
#include "host.h"

#include <cmath>

using namespace ttsh;

namespace {

template <class Pre, class F>
int enqueue_call(tts_ctx* c, void* stream, Pre&& pre, F&& fn) {
  return guarded_ctx(c, [&] {
    pre();
    DeviceGuard g(c->device);
    enter(c, stream);
    fn();
    leave(c, stream);
  });
}

int stft_frames(int len, int n_fft, int hop) { return 1 + (len + 2 * (n_fft / 2) - n_fft) / hop; }

// the checks the two STFT entries share; `who` names the entry in the messages
void check_stft_args(const std::string& who, const int32_t* h_nsamples, int B, int L_max, int n_fft, int win_length,
                     int hop_length) {
  TTS_CHECK(B >= 1 && B <= BMAX, who + ": 1 <= B <= 64");
  TTS_CHECK(n_fft >= 16 && n_fft <= 2048, who + ": n_fft outside [16, 2048]");
  TTS_CHECK(win_length >= 16 && win_length <= n_fft, who + ": win_length outside [16, n_fft]");
  TTS_CHECK(hop_length >= 1, who + ": hop_length must be >= 1");
  TTS_CHECK(L_max >= 1 && L_max < (1 << 30), who + ": L_max out of range");
  for (int b = 0; b < B; ++b) {
    TTS_CHECK(h_nsamples[b] <= L_max, who + ": h_nsamples[b] above L_max");
    TTS_CHECK(h_nsamples[b] > n_fft / 2,
              who + ": Padding size should be less than the corresponding input dimension: every row needs "
                    "h_nsamples[b] > n_fft / 2 (the reflect padding of torch.stft)");
  }
}

// The basis of (n_fft, win_length): the periodic Hann window of win_length points at offset
// (n_fft - win_length) / 2 of the frame, times cos / -sin of 2 pi (f n mod n_fft) / n_fft; the angle
// is reduced in integers, everything else is in double and rounded once.
StftBasis stft_basis(tts_ctx* c, int n_fft, int win_length) {
  VocEvalWS& V = c->vews;
  const int F = n_fft / 2 + 1, woff = (n_fft - win_length) / 2;
  auto it = V.bases.find({n_fft, win_length});
  if (it == V.bases.end()) {
    if (V.bases.size() >= 32) {  // queued calls may still read the bases about to be dropped
      HIP_OK(hipStreamSynchronize(c->s));
      V.bases.clear();
    }
    const int Kp = (win_length + ST_KCHUNK - 1) / ST_KCHUNK * ST_KCHUNK, nbt = (F + ST_TB - 1) / ST_TB;
    std::vector<double> cs(n_fft), sn(n_fft), win(win_length);
    for (int m = 0; m < n_fft; ++m) {
      cs[m] = std::cos(2.0 * M_PI * m / n_fft);
      sn[m] = std::sin(2.0 * M_PI * m / n_fft);
    }
    for (int k = 0; k < win_length; ++k) win[k] = 0.5 - 0.5 * std::cos(2.0 * M_PI * k / win_length);
    std::vector<float> h((size_t)nbt * Kp * 2 * ST_TB, 0.f);
    for (int f = 0; f < F; ++f)
      for (int k = 0; k < win_length; ++k) {
        const int m = (int)((long)f * (k + woff) % n_fft);
        float* row = &h[((size_t)(f / ST_TB) * Kp + k) * 2 * ST_TB];
        row[f % ST_TB] = (float)(win[k] * cs[m]);
        row[ST_TB + f % ST_TB] = (float)(-win[k] * sn[m]);
      }
    VocEvalWS::Basis& nb = V.bases[{n_fft, win_length}];
    nb.d.upload(h);
    nb.Kp = Kp;
    nb.nbt = nbt;
    it = V.bases.find({n_fft, win_length});
  }
  return StftBasis{it->second.d.f(), n_fft, win_length, it->second.Kp, woff, F, it->second.nbt};
}

}  // namespace

extern "C" {

int tts_pqmf_analysis(tts_ctx* c, const float* d_x, const int32_t* h_lens, int B, int L_max, int N, const float* d_H,
                      int taps, float* d_y, int Lout_max, void* stream) {
  return enqueue_call(
      c, stream,
      [&] {
        TTS_CHECK(d_x && h_lens && d_H && d_y, "null argument");
        TTS_CHECK(B >= 1 && B <= BMAX, "pqmf_analysis: 1 <= B <= 64");
        TTS_CHECK(N >= 1 && N <= PQ_NMAX, "pqmf_analysis: N outside [1, 8]");
        TTS_CHECK(taps >= 0 && taps % 2 == 0 && taps + 1 <= PQ_NTAP_MAX,
                  "pqmf_analysis: taps must be even and in [0, 254] (the filters hold taps + 1 coefficients)");
        TTS_CHECK(L_max >= 1 && L_max < (1 << 30) && Lout_max >= 1, "pqmf_analysis: L_max or Lout_max out of range");
        for (int b = 0; b < B; ++b)
          TTS_CHECK(h_lens[b] >= 0 && h_lens[b] <= L_max && (h_lens[b] == 0 || (h_lens[b] - 1) / N + 1 <= Lout_max),
                    "pqmf_analysis: every row needs 0 <= h_lens[b] <= L_max and (h_lens[b] - 1) / N + 1 <= Lout_max");
      },
      [&] { launch_pqmf_analysis(d_x, L_max, row_ints(h_lens, B), B, d_H, N, taps + 1, d_y, Lout_max, c->s); });
}

int tts_stft_pair_sums(tts_ctx* c, const float* d_yhat, const float* d_y, const int32_t* h_nsamples, int B, int L_max,
                       int n_fft, int win_length, int hop_length, double* d_sums, void* stream) {
  return enqueue_call(
      c, stream,
      [&] {
        TTS_CHECK(d_yhat && d_y && h_nsamples && d_sums, "null argument");
        check_stft_args("stft_pair_sums", h_nsamples, B, L_max, n_fft, win_length, hop_length);
        for (int b = 0; b < B; ++b)
          TTS_CHECK(stft_frames(h_nsamples[b], n_fft, hop_length) <= (1 << 22),
                    "stft_pair_sums: a row has more than 2^22 frames");
      },
      [&] {
        const StftBasis W = stft_basis(c, n_fft, win_length);
        int frames_max = 1;
        for (int b = 0; b < B; ++b) frames_max = std::max(frames_max, stft_frames(h_nsamples[b], n_fft, hop_length));
        const size_t tiles = (size_t)(frames_max + ST_TF - 1) / ST_TF * W.nbt;
        ensure<float>(c->vews.partial, (size_t)B * tiles * 3);
        launch_stft_pair_sums(d_yhat, d_y, L_max, row_ints(h_nsamples, B), B, W, hop_length, frames_max,
                              c->vews.partial.f(), d_sums, c->s);
      });
}

int tts_torch_stft_mag(tts_ctx* c, const float* d_wav, const int32_t* h_nsamples, int B, int L_max, int n_fft,
                       int win_length, int hop_length, float* d_mag, int frames_max, void* stream) {
  return enqueue_call(
      c, stream,
      [&] {
        TTS_CHECK(d_wav && h_nsamples && d_mag, "null argument");
        check_stft_args("torch_stft_mag", h_nsamples, B, L_max, n_fft, win_length, hop_length);
        TTS_CHECK(frames_max >= 1 && (long)frames_max * (n_fft / 2 + 1) < (1L << 31),
                  "torch_stft_mag: frames_max out of range");
        for (int b = 0; b < B; ++b)
          TTS_CHECK(stft_frames(h_nsamples[b], n_fft, hop_length) <= frames_max,
                    "torch_stft_mag: a row has more frames than frames_max");
      },
      [&] {
        launch_stft_mag_store(d_wav, L_max, row_ints(h_nsamples, B), B, stft_basis(c, n_fft, win_length), hop_length,
                              d_mag, frames_max, c->s);
      });
}

}  // extern "C"
