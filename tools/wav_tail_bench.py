"""Time the waveform tail on the 32-row LJ-length batch: ``python tools/wav_tail_bench.py`` on an MI355X.

1. The end of ``Synthesizer.tts``, from the (32, L_max) float32 waveforms on the device to the wav
   bytes: the host path (copy, ``find_endpoint`` per row, the Python-list join, ``save_wav``) against
   ``AudioProcessor.finish_batch`` + ``scipy.io.wavfile.write``. Wall time around a synchronised
   call; the two byte strings are compared.
2. ``inv_spectrogram_batch`` on 32 rows against 32 B = 1 calls of it (60 Griffin-Lim iterations,
   pre-emphasis 0.97, so spec -> magnitudes -> Griffin-Lim -> de-emphasis), and ``deemphasis_batch``
   alone. Recorded in profiles/wav_tail/tail_time.txt."""
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.io.wavfile  # noqa: E402
import torch  # noqa: E402

from tts_amd.audio import AudioProcessor, wav_bytes  # noqa: E402
from tts_amd.workload import HOP, lj_profile  # noqa: E402

AUDIO = dict(fft_size=1024, win_length=1024, hop_length=HOP, sample_rate=22050, preemphasis=0.97, ref_level_db=20,
             power=1.5, griffin_lim_iters=60, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0, spec_gain=20,
             signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0, clip_norm=True,
             griffin_lim_device="gpu", wav_tail_device="gpu")


def _wall(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def _line(name, ts):
    print(f"{name}: median {np.median(ts):.3f} ms ({len(ts)} runs: min {min(ts):.3f} max {max(ts):.3f})", flush=True)


def host_tail(ap, wav, counts):
    rows = wav.cpu().numpy()
    wavs = []
    for i, n in enumerate(counts):
        w = rows[i, :n]
        w = w[:ap.find_endpoint(w)]
        wavs += list(w)
        wavs += [0] * 10000
    return wav_bytes(ap, np.asarray(wavs, np.float32)).getvalue()


def device_tail(ap, wav, counts):
    pcm, _ = ap.finish_batch(wav, counts)
    out = io.BytesIO()
    scipy.io.wavfile.write(out, ap.sample_rate, pcm)
    return out.getvalue()


def main():
    dev = torch.device("cuda:0")
    ap = AudioProcessor(**AUDIO)
    _, M = lj_profile()
    B = len(M)
    rs = np.random.RandomState(0)

    # 1. the tts() tail: speech-like rows (noise under a slow envelope) that end in 1.2 s of near-silence
    counts = [m * HOP for m in M]
    x = np.zeros((B, max(counts)), np.float32)
    for b, n in enumerate(counts):
        t = np.arange(n) / ap.sample_rate
        x[b, :n] = 0.2 * rs.randn(n) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
        x[b, max(0, n - 26460):n] *= 0.01
    wav = torch.from_numpy(x).to(dev)
    print(f"tts() tail, B={B}, {sum(counts)} samples, L_max={max(counts)}")
    device_tail(ap, wav, counts)  # first call: workspace
    dev_bytes, ts = _wall(lambda: device_tail(ap, wav, counts), 10)
    _line("  device path (finish_batch + wavfile.write)", ts)
    host_bytes, ts = _wall(lambda: host_tail(ap, wav, counts), 3)
    _line("  host path (copy, find_endpoint, list join, save_wav)", ts)
    print(f"  bytes equal: {dev_bytes == host_bytes} ({len(dev_bytes)} bytes)")

    # 2. inv_spectrogram_batch: 32 rows in one call against 32 B = 1 calls
    specs = torch.from_numpy(rs.uniform(-4, 4, (B, max(M), 513)).astype(np.float32)).to(dev)
    phase = torch.rand(B, max(M), 513, device=dev)
    ap.inv_spectrogram_batch(specs, M, phase)
    _, ts = _wall(lambda: ap.inv_spectrogram_batch(specs, M, phase), 5)
    _line(f"inv_spectrogram_batch B={B} M_max={max(M)} ({sum(M)} frames), one call", ts)
    rows = [(specs[b:b + 1, :m].contiguous(), phase[b:b + 1, :m].contiguous()) for b, m in enumerate(M)]
    _, ts = _wall(lambda: [ap.inv_spectrogram_batch(s, [s.shape[1]], p) for s, p in rows], 5)
    _line(f"inv_spectrogram_batch, {B} calls at B=1", ts)
    g, counts = ap.inv_spectrogram_batch(specs, M, phase, deemphasis=False)
    _, ts = _wall(lambda: ap.deemphasis_batch(g, counts), 10)
    _line(f"deemphasis_batch B={B} L_max={g.shape[1]}", ts)


if __name__ == "__main__":
    main()
