"""Inputs and case tables shared by tests/golden/make_vocoder_eval_golden.py and the vocoder scoring
tests: the fixture stores seeds, lengths and results, the signals are rebuilt from the seeds here."""
import numpy as np

# (n_fft, hop_length, win_length): MultiScaleSTFTLoss's defaults, then the sub-band resolutions of the
# reference's multiband_melgan_config.json
FULLBAND = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
SUBBAND = ((384, 30, 150), (683, 60, 300), (171, 10, 60))
RESOLUTIONS = FULLBAND + SUBBAND
PQMF_LENGTHS = (1, 4, 5, 62, 63, 64, 1001)
PQMF_SEED = 100
MULTI_FULL_SEED, MULTI_SUB_SEED = 300, 301
# a quiet pair whose noise floor lies under TorchSTFT's clamp (magnitude 1e-4) and whose sines lie above
CLAMP_RESOLUTION, CLAMP_LENGTH, CLAMP_SEED, CLAMP_GAIN = (171, 10, 60), 340, 2000, np.float32(2e-4)


def resolution_lengths(n_fft, hop):
    """The shortest row torch.stft accepts, a multiple of hop near 2 n_fft, and that minus 1."""
    m = hop * int(round(2 * n_fft / hop))
    return (n_fft // 2 + 1, m, m - 1)


def resolution_seeds(i):
    """Seeds of resolution i: its three ragged rows, then its three equal-length rows."""
    return [1000 + 10 * i + j for j in range(3)], [1000 + 10 * i + 5 + j for j in range(3)]


def stft_frames(n, n_fft, hop):
    return 1 + (n + 2 * (n_fft // 2) - n_fft) // hop


def _signal(rs, n):
    """Gaussian noise at 0.05 plus six sines at 0.1, frequencies in cycles per sample."""
    t = np.arange(n)
    y = 0.05 * rs.randn(n)
    for _ in range(6):
        f, ph = rs.uniform(0.002, 0.45), rs.uniform(0, 2 * np.pi)
        y = y + 0.1 * np.sin(2 * np.pi * f * t + ph)
    return y


def signal(seed, n):
    return _signal(np.random.RandomState(seed), n).astype(np.float32)


def pair(seed, n):
    """(y_hat, y) float32: a signal and its distorted copy y + 0.03 noise + 0.2 another such signal."""
    rs = np.random.RandomState(seed)
    y = _signal(rs, n)
    y_hat = y + 0.03 * rs.randn(n) + 0.2 * _signal(rs, n)
    return y_hat.astype(np.float32), y.astype(np.float32)


def tolerance(dev32, value):
    """8 x max(the reference's float32-vs-float64 deviation, 2^-23 |value|): the project's 8 x float32
    yardstick, floored at one float32 spacing of the value, since the result is itself a float32."""
    return 8.0 * max(float(dev32), 2.0 ** -23 * float(np.max(np.abs(value))))


def pqmf_analysis64(x, H):
    """PQMF.analysis of one row in float64: F.conv1d(x, H, padding=taps // 2, stride=N), H (N, taps + 1)."""
    N, ntap = H.shape
    xp = np.pad(np.asarray(x, np.float64), (ntap - 1) // 2)
    return np.stack([np.correlate(xp, H[n].astype(np.float64), mode="valid")[::N] for n in range(N)])
