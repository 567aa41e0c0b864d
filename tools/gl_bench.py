"""Griffin-Lim waveform stage on the LJSpeech-shaped batch (32 utterances, lj_profile mel lengths):
the batched GPU path (AudioProcessor.inv_melspectrogram_batch: tts_mel_to_linear + tts_griffin_lim)
against the CPU path it replaces (AudioProcessor.inv_melspectrogram per sentence, float64).

60 iterations, fft 1024 / win 1024 / hop 256. Mels are those of a deterministic chirp + noise signal
of each utterance's length. GPU times are hipEvent times around the calls on the current stream,
warm-up excluded, median of --steps calls; the per-iteration kernel time is the difference between
a 60-iteration and a 0-iteration tts_griffin_lim call, over 60. Prints one JSON line (and writes it
to --out).
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

AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0, ref_level_db=20,
             power=1.5, griffin_lim_iters=60, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0, spec_gain=20,
             signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0, clip_norm=True)


def _mel(ap, M, seed):
    n = ap.hop_length * (M - 1)
    t = np.arange(n) / ap.sample_rate
    y = 0.3 * np.sin(2 * np.pi * (200 + 300 * t / max(t[-1], 1e-9)) * t) + 0.05 * np.random.RandomState(seed).randn(n)
    return ap.melspectrogram(y)


class _Fixed:
    """An rng whose rand returns the given numbers (the GPU run's phase), as float64."""

    def __init__(self, u):
        self.u = np.asarray(u, np.float64)

    def rand(self, *shape):
        assert tuple(shape) == self.u.shape
        return self.u


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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--cpu-utts", type=int, default=32, help="sentences timed on the CPU path (0: skip)")
    p.add_argument("--cpu-threads", type=int, default=16)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    _, M = lj_profile()
    gpu, cpu = AudioProcessor(**AUDIO, griffin_lim_device="gpu"), AudioProcessor(**AUDIO)
    mels = [_mel(cpu, m, i) for i, m in enumerate(M)]
    B, Mx, F = len(M), max(M), 513
    batch = np.zeros((B, Mx, 80), np.float32)
    for i, m in enumerate(mels):
        batch[i, :m.shape[1]] = m.T
    rs = np.random.RandomState(0)
    phase = rs.rand(B, Mx, F).astype(np.float32)
    d_mel, d_phase = torch.from_numpy(batch).to(dev), torch.from_numpy(phase).to(dev)
    long_i = int(np.argmax(M))
    d_mel1 = d_mel[long_i:long_i + 1, :M[long_i]].contiguous()
    d_phase1 = d_phase[long_i:long_i + 1, :M[long_i]].contiguous()

    t_batch = _event_ms(lambda: gpu.inv_melspectrogram_batch(d_mel, M, d_phase), a.steps, a.warmup)
    t_one = _event_ms(lambda: gpu.inv_melspectrogram_batch(d_mel1, [M[long_i]], d_phase1), a.steps, a.warmup)

    # tts_griffin_lim alone at 60 and 0 iterations: the per-iteration kernel time
    eng = get_engine(dev)
    S = torch.empty(B, Mx, F, device=dev)
    scale, offset, clip = gpu._denorm_affine()
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)  # noqa: E731
    eng.mel_to_linear(d_mel, M, put(gpu.inv_mel_basis), put(scale), put(offset), clip, gpu.spec_gain, gpu.power, S)
    wav = torch.empty(B, 256 * (Mx - 1), device=dev)
    t60 = _event_ms(lambda: eng.griffin_lim(S, M, 1024, 1024, 256, 60, d_phase, wav), a.steps, a.warmup)
    t0 = _event_ms(lambda: eng.griffin_lim(S, M, 1024, 1024, 256, 0, d_phase, wav), a.steps, a.warmup)

    out = {"metric": "griffin_lim_batch_ms", "value": t_batch[0], "iters": 60, "batch": B, "frames": int(sum(M)),
           "M_max": Mx, "gpu_batch_ms": {"median": t_batch[0], "min": t_batch[1], "max": t_batch[2]},
           "gpu_single_ms": {"median": t_one[0], "min": t_one[1], "max": t_one[2], "frames": int(M[long_i])},
           "griffin_lim_60_ms": t60[0], "griffin_lim_0_ms": t0[0], "iteration_kernel_us": (t60[0] - t0[0]) / 60 * 1e3,
           "steps": a.steps, "warmup": a.warmup}

    if a.cpu_utts:
        torch.set_num_threads(a.cpu_threads)
        n = min(a.cpu_utts, B)
        y = None
        t_all = time.perf_counter()
        for i in range(n):
            w = cpu.inv_melspectrogram(mels[i], rng=_Fixed(phase[i, :M[i]].T))
            if i == long_i:
                y = w
        cpu_batch = time.perf_counter() - t_all
        t1 = time.perf_counter()
        w = cpu.inv_melspectrogram(mels[long_i], rng=_Fixed(phase[long_i, :M[long_i]].T))
        cpu_one = time.perf_counter() - t1
        y = w if y is None else y
        g = gpu.inv_melspectrogram_batch(d_mel1, [M[long_i]], d_phase1)[0][0].cpu().numpy()
        out["cpu"] = {"threads": a.cpu_threads, "sentences": n, "batch_ms": cpu_batch * 1e3, "single_ms": cpu_one * 1e3,
                      "kind": "AudioProcessor.inv_melspectrogram, float64 torch.stft/istft, one sentence at a time"}
        out["speedup_batch"] = cpu_batch * 1e3 * (B / n) / t_batch[0]
        out["speedup_single"] = cpu_one * 1e3 / t_one[0]
        out["gpu_vs_cpu_max_rel_err"] = float(np.abs(g - y).max() / np.abs(y).max())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
