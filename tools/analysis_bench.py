"""Audio analysis on the LJSpeech-shaped batch (32 utterances, lj_profile mel lengths): the batched GPU
path (AudioProcessor.melspectrogram_batch: tts_stft_mag + tts_mag_to_feature) against the CPU path it
replaces (AudioProcessor.melspectrogram per utterance, float64 torch.stft).

fft 1024 / win 1024 / hop 256, pre-emphasis 0.97. Each waveform is a deterministic chirp + noise
signal of hop * (M - 1) samples. GPU times are hipEvent times around the calls on the current stream,
warm-up excluded, median of --steps calls: the whole batch call, the two library calls on their own,
the direct DFT kernel forced at 1024 (algo = 2), and the batch at the GE2E parameters (400 / 400 /
160, the direct kernel). Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tts_amd._lib import get_engine  # noqa: E402
from tts_amd.audio import AudioProcessor  # noqa: E402
from tts_amd.workload import lj_profile  # noqa: E402

AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.97, ref_level_db=20,
             power=1.5, griffin_lim_iters=60, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0, spec_gain=20,
             signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0, clip_norm=True)
GE2E = dict(AUDIO, fft_size=400, win_length=400, hop_length=160, sample_rate=16000, preemphasis=0.98, num_mels=40,
            mel_fmin=0.0, mel_fmax=8000.0)


def _wav(sr, n, seed):
    t = np.arange(n) / sr
    y = 0.3 * np.sin(2 * np.pi * (200 + 300 * t / max(t[-1], 1e-9)) * t) + 0.05 * np.random.RandomState(seed).randn(n)
    return y.astype(np.float32)


def _event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "min": float(np.min(out)), "max": float(np.max(out))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--cpu-utts", type=int, default=32, help="utterances timed on the CPU path (0: skip)")
    p.add_argument("--cpu-threads", type=int, default=16)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    _, M = lj_profile()
    gpu, cpu = AudioProcessor(**AUDIO, analysis_device="gpu"), AudioProcessor(**AUDIO)
    ns = [256 * (m - 1) for m in M]
    ys = [_wav(22050, n, i) for i, n in enumerate(ns)]
    B, L = len(ns), max(ns)
    batch = np.zeros((B, L), np.float32)
    for i, y in enumerate(ys):
        batch[i, :len(y)] = y
    d_wav = torch.from_numpy(batch).to(dev)
    long_i = int(np.argmax(ns))
    d_wav1 = d_wav[long_i:long_i + 1].contiguous()

    t_batch = _event_ms(lambda: gpu.melspectrogram_batch(d_wav, ns), a.steps, a.warmup)
    t_one = _event_ms(lambda: gpu.melspectrogram_batch(d_wav1, [ns[long_i]]), a.steps, a.warmup)

    # the two library calls on their own, and the direct kernel on the same frames
    eng = get_engine(dev)
    frames = [1 + n // 256 for n in ns]
    mag = torch.empty(B, max(frames), 513, device=dev)
    out = torch.empty(B, max(frames), 80, device=dev)
    scale, offset, clip = gpu._norm_affine(80)
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)  # noqa: E731
    basis, scale, offset = put(gpu.mel_basis), put(scale), put(offset)
    t_fft = _event_ms(lambda: eng.stft_mag(d_wav, ns, 1024, 1024, 256, 0.97, mag), a.steps, a.warmup)
    t_dft = _event_ms(lambda: eng.stft_mag(d_wav, ns, 1024, 1024, 256, 0.97, mag, algo=2), a.steps, a.warmup)
    eng.stft_mag(d_wav, ns, 1024, 1024, 256, 0.97, mag)
    t_feat = _event_ms(lambda: eng.mag_to_feature(mag, frames, basis, 20.0, scale, offset, clip, out), a.steps,
                       a.warmup)
    ge = AudioProcessor(**GE2E, analysis_device="gpu")
    t_ge2e = _event_ms(lambda: ge.melspectrogram_batch(d_wav, ns), a.steps, a.warmup)

    res = {"metric": "melspectrogram_batch_ms", "value": t_batch["median"], "batch": B, "frames": int(sum(frames)),
           "samples": int(sum(ns)), "M_max": max(frames), "gpu_batch_ms": t_batch,
           "gpu_single_ms": dict(t_one, frames=frames[long_i]), "stft_mag_fft_ms": t_fft,
           "stft_mag_direct_1024_ms": t_dft, "mag_to_feature_ms": t_feat,
           "ge2e_400_160_batch_ms": dict(t_ge2e, frames=int(sum(1 + n // 160 for n in ns))),
           "steps": a.steps, "warmup": a.warmup}

    g = gpu.melspectrogram_batch(d_wav, ns)[0].cpu().numpy()
    if a.cpu_utts:
        torch.set_num_threads(a.cpu_threads)
        n = min(a.cpu_utts, B)
        cpu.melspectrogram(ys[0].astype(np.float64))  # warm-up: thread pool, FFT plan
        t0 = time.perf_counter()
        refs = [cpu.melspectrogram(ys[i].astype(np.float64)) for i in range(n)]
        cpu_batch = time.perf_counter() - t0
        t1 = time.perf_counter()
        cpu.melspectrogram(ys[long_i].astype(np.float64))
        cpu_one = time.perf_counter() - t1
        res["cpu"] = {"threads": a.cpu_threads, "utterances": n, "batch_ms": cpu_batch * 1e3, "single_ms": cpu_one * 1e3,
                      "kind": "AudioProcessor.melspectrogram, float64 torch.stft, one utterance at a time"}
        res["speedup_batch"] = cpu_batch * 1e3 * (B / n) / t_batch["median"]
        res["speedup_single"] = cpu_one * 1e3 / t_one["median"]
        res["gpu_vs_cpu_max_abs_err"] = float(max(np.abs(g[i, :frames[i]].T - refs[i]).max() for i in range(n)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
