"""Vocoder scoring on the GPU: the multi-resolution STFT distances (tts_stft_pair_sums through
MultiScaleSTFTLoss / MultiScaleSubbandSTFTLoss) and PQMF.analysis at three shapes:

    full     32 rows of 8 s at 22,050 Hz, the three full-band resolutions
    subband  the same 32 utterances as (32, 4, L / 4) sub-bands, the three sub-band resolutions
    single   one row of 0.5 s, full-band (launch-bound: a figure for overheads)

Signals are seeded noise plus sines and a distorted copy. Times are hipEvent times around the calls
on the current stream, warm-up excluded, median / min / max of --steps calls; each call includes the
float64 torch ops that turn the row sums into the two losses. ``flop`` is what the DFT GEMMs need,
computed from the shapes: 2 signals x frames x win_length x 2 (n_fft / 2 + 1) x 2 per resolution, the
tiles' padding not counted; ``tflops`` = flop / median time, an end-to-end rate of the call, not a
kernel's share of peak. Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tts_amd import PQMF, MultiScaleSTFTLoss, MultiScaleSubbandSTFTLoss  # noqa: E402
from tts_amd.vocoder_eval import SUBBAND_STFT_LOSS_PARAMS  # noqa: E402
from tts_amd.vocoder_losses import stft_frames  # noqa: E402


def _signals(B, L, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(L)

    def one():
        y = 0.05 * rs.randn(B, L)
        for _ in range(6):
            y += 0.1 * np.sin(2 * np.pi * rs.uniform(0.002, 0.45, (B, 1)) * t + rs.uniform(0, 2 * np.pi, (B, 1)))
        return y
    y = one()
    y_hat = y + 0.03 * rs.randn(B, L) + 0.2 * one()
    return y_hat.astype(np.float32), y.astype(np.float32)


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


def _flop(loss, rows, L):
    return sum(2.0 * rows * stft_frames(L, f.n_fft, f.hop_length) * f.win_length * 2 * (f.n_fft // 2 + 1) * 2
               for f in loss.loss_funcs)


def _timed(loss, y_hat, y, rows, L, steps, warmup):
    t = _event_ms(lambda: loss(y_hat, y), steps, warmup)
    flop = _flop(loss, rows, L)
    return dict(t, rows=rows, samples=L, flop=flop, tflops=flop / (t["median"] * 1e-3) / 1e12)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=32)
    p.add_argument("--seconds", type=float, default=8.0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    B, L = a.rows, int(a.seconds * 22050) // 4 * 4
    y_hat, y = (torch.from_numpy(x).to(dev) for x in _signals(B, L, 0))
    full, sub = MultiScaleSTFTLoss(), MultiScaleSubbandSTFTLoss(**SUBBAND_STFT_LOSS_PARAMS)
    pq = PQMF().to(dev)
    res = {"metric": "multi_scale_stft_loss_ms", "steps": a.steps, "warmup": a.warmup}
    res["full"] = _timed(full, y_hat, y, B, L, a.steps, a.warmup)
    res["value"] = res["full"]["median"]
    res["pqmf_analysis_ms"] = _event_ms(lambda: pq.analysis(y[:, None, :]), a.steps, a.warmup)
    bands_hat, bands = pq.analysis(y_hat[:, None, :]), pq.analysis(y[:, None, :])
    res["subband"] = _timed(sub, bands_hat, bands, 4 * B, L // 4, a.steps, a.warmup)
    L1 = 22050 // 2
    res["single"] = _timed(full, y_hat[:1, :L1], y[:1, :L1], 1, L1, a.steps, a.warmup)
    res["losses"] = {"full": [float(v) for v in full(y_hat, y)], "subband": [float(v) for v in sub(bands_hat, bands)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
