"""Generate tests/golden/vocoder_eval.npz by running the REFERENCE ``PQMF``, ``STFTLoss``,
``MultiScaleSTFTLoss`` and ``MultiScaleSubbandSTFTLoss`` on the CPU.

Run where the reference checkout is (``TTS_REFERENCE`` names it), from the repository root; no GPU is
needed:

    TTS_REFERENCE=<checkout> python tests/golden/make_vocoder_eval_golden.py

On torch >= 2 the reference's ``TorchSTFT.__call__`` raises ("stft requires the return_complex
parameter"), so that one method is replaced here: the same ``torch.stft`` call with
``return_complex=True`` and ``view_as_real``, and the reference's ``sqrt(clamp(M^2 + P^2, 1e-8))``.
Everything else runs as the reference wrote it.

Inputs come from tests/vocoder_eval_cases.py (seeds -> float32 signals). Every result is the reference
in float64 on those float32-rounded inputs; next to it (``*_dev``) stands the reference's own
float32-vs-float64 deviation, which the tests' tolerances are built from. Stored:

    pqmf_<len>, pqmf_<len>_dev          PQMF.analysis of one row of <len> samples (4, (len - 1) // 4 + 1)
    r<i>_row, r<i>_row_dev              (3, 2) per-row (loss_mag, loss_sc) of resolution i's ragged rows
    r<i>_pool, r<i>_pool_dev            (2,) the ragged batch pooled, from the per-row float64 sums
    r<i>_equal, r<i>_equal_dev          (2,) the reference's batch call on three equal-length rows
    r<i>_mag0                           (F, frames) magnitudes of y of the shortest row
    r<i>_mag2                           (F, 4) the first and last two frames of y of the third row
    r<i>_mag_dev                        (2,) their float32 deviations
    clamp_row, clamp_row_dev            (2,) a pair scaled so that part of its bins sit on the 1e-8 clamp
                                        (clamp_share: that part, of y)
    multi_full, multi_sub (+ _dev)      the two multi-scale classes at their defaults / the sub-band
                                        resolutions, on (2, 4096) and (2, 4, 1024)
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ["TTS_REFERENCE"])

import vocoder_eval_cases as vc  # noqa: E402
from TTS.vocoder.layers import losses as ref_losses  # noqa: E402
from TTS.vocoder.layers.pqmf import PQMF  # noqa: E402


def _torch_stft_call(self, x):
    o = torch.view_as_real(torch.stft(x, self.n_fft, self.hop_length, self.win_length, self.window, center=True,
                                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True))
    M = o[:, :, :, 0]
    P = o[:, :, :, 1]
    return torch.sqrt(torch.clamp(M ** 2 + P ** 2, min=1e-8))


ref_losses.TorchSTFT.__call__ = _torch_stft_call


def build(cls, dtype, *args):
    """An instance whose Hann windows are of dtype (TorchSTFT builds them at the default dtype)."""
    torch.set_default_dtype(dtype)
    try:
        return cls(*args)
    finally:
        torch.set_default_dtype(torch.float32)


def both(fn):
    """fn(dtype) -> array, in float64 and float32: (float64 result, |float32 - float64| per entry)."""
    r64 = np.asarray(fn(torch.float64), np.float64)
    r32 = np.asarray(fn(torch.float32), np.float64)
    return r64, np.abs(r32 - r64)


def t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def pair_of(loss, y_hat, y, dtype):
    with torch.no_grad():
        lm, lsc = loss(t(y_hat, dtype), t(y, dtype))
    return [float(lm), float(lsc)]


def row_sums(stft, y_hat, y, dtype):
    """Sums over one row's bins and frames as STFTLoss forms them, reduced at dtype: A, D, R, count."""
    with torch.no_grad():
        yh_M, y_M = stft(t(y_hat, dtype)[None]), stft(t(y, dtype)[None])
        A = (torch.log(y_M) - torch.log(yh_M)).abs().sum()
        D = ((y_M - yh_M) ** 2).sum()
        R = (y_M ** 2).sum()
    return np.array([float(A), float(D), float(R), y_M.numel()], np.float64)


def main():
    torch.set_num_threads(4)
    out = {}
    # ---- PQMF analysis, every row alone
    for j, n in enumerate(vc.PQMF_LENGTHS):
        x = vc.signal(vc.PQMF_SEED + j, n)

        def run(dtype):
            p = PQMF(N=4, taps=62, cutoff=0.15, beta=9.0).to(dtype)
            with torch.no_grad():
                return p.analysis(t(x, dtype)[None, None])[0].numpy()
        r64, r32 = run(torch.float64), run(torch.float32)
        assert r64.shape == (4, (n - 1) // 4 + 1)
        out[f"pqmf_{n}"], out[f"pqmf_{n}_dev"] = r64, np.abs(r32 - r64).max()

    # ---- each resolution alone
    for i, (n_fft, hop, win) in enumerate(vc.RESOLUTIONS):
        lens = vc.resolution_lengths(n_fft, hop)
        ragged, equal = vc.resolution_seeds(i)
        pairs = [vc.pair(s, n) for s, n in zip(ragged, lens)]
        loss = {d: build(ref_losses.STFTLoss, d, n_fft, hop, win) for d in (torch.float64, torch.float32)}
        out[f"r{i}_row"], out[f"r{i}_row_dev"] = both(
            lambda d: [pair_of(loss[d], yh[None], y[None], d) for yh, y in pairs])

        def pooled(d):
            s = sum(row_sums(loss[d].stft, yh, y, d) for yh, y in pairs)
            return [s[0] / s[3], np.sqrt(s[1]) / np.sqrt(s[2])]
        out[f"r{i}_pool"], out[f"r{i}_pool_dev"] = both(pooled)
        eq = [vc.pair(s, lens[1]) for s in equal]
        yh_eq, y_eq = np.stack([p[0] for p in eq]), np.stack([p[1] for p in eq])
        out[f"r{i}_equal"], out[f"r{i}_equal_dev"] = both(lambda d: pair_of(loss[d], yh_eq, y_eq, d))

        def mags(d):
            with torch.no_grad():
                m0 = loss[d].stft(t(pairs[0][1], d)[None])[0].numpy()
                m2 = loss[d].stft(t(pairs[2][1], d)[None])[0].numpy()
            return m0, m2
        (m0, m2), (m0f, m2f) = mags(torch.float64), mags(torch.float32)
        assert m0.shape == (n_fft // 2 + 1, vc.stft_frames(lens[0], n_fft, hop))
        assert m2.shape == (n_fft // 2 + 1, vc.stft_frames(lens[2], n_fft, hop))
        sel = [0, 1, m2.shape[1] - 2, m2.shape[1] - 1]
        out[f"r{i}_mag0"], out[f"r{i}_mag2"] = m0, m2[:, sel]
        out[f"r{i}_mag_dev"] = np.array([np.abs(m0f - m0).max(), np.abs(m2f - m2)[:, sel].max()])
        on_clamp = float(np.mean(m2 <= 1.0001e-4))
        print(f"r{i} {n_fft}/{hop}/{win} lens {lens}: rows {out[f'r{i}_row'].tolist()} dev {out[f'r{i}_row_dev']} "
              f"pool {out[f'r{i}_pool']} equal {out[f'r{i}_equal']}; bins on the clamp {on_clamp:.3%}")

    # ---- a quiet pair at 171 / 10 / 60: the noise floor sits under the 1e-8 clamp, the sines above it
    n_fft, hop, win = vc.CLAMP_RESOLUTION
    yh, y = (vc.CLAMP_GAIN * a for a in vc.pair(vc.CLAMP_SEED, vc.CLAMP_LENGTH))
    loss = {d: build(ref_losses.STFTLoss, d, n_fft, hop, win) for d in (torch.float64, torch.float32)}
    out["clamp_row"], out["clamp_row_dev"] = both(lambda d: pair_of(loss[d], yh[None], y[None], d))
    with torch.no_grad():
        m = loss[torch.float64].stft(t(y, torch.float64)[None]).numpy()
    out["clamp_share"] = np.mean(m <= 1e-4)
    print("clamp_row", out["clamp_row"], out["clamp_row_dev"], f"bins of y on the clamp {out['clamp_share']:.1%}")

    # ---- the two multi-scale classes
    n_ffts, hops, wins = (list(c) for c in zip(*vc.SUBBAND))
    yh, y = vc.pair(vc.MULTI_FULL_SEED, 2 * 4096)
    full = {d: build(ref_losses.MultiScaleSTFTLoss, d) for d in (torch.float64, torch.float32)}
    out["multi_full"], out["multi_full_dev"] = both(
        lambda d: pair_of(full[d], yh.reshape(2, 4096), y.reshape(2, 4096), d))
    yh, y = vc.pair(vc.MULTI_SUB_SEED, 2 * 4 * 1024)
    sub = {d: build(ref_losses.MultiScaleSubbandSTFTLoss, d, n_ffts, hops, wins)
           for d in (torch.float64, torch.float32)}
    out["multi_sub"], out["multi_sub_dev"] = both(
        lambda d: pair_of(sub[d], yh.reshape(2, 4, 1024), y.reshape(2, 4, 1024), d))
    print("multi_full", out["multi_full"], out["multi_full_dev"], "multi_sub", out["multi_sub"], out["multi_sub_dev"])

    path = os.path.join(HERE, "vocoder_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
