"""The multi-resolution STFT distances of ``TTS/vocoder/layers/losses.py:7-84`` on MI355X.

Same names and constructor signatures as the reference (``TorchSTFT``, ``STFTLoss``,
``MultiScaleSTFTLoss``, ``MultiScaleSubbandSTFTLoss``); evaluation only, no gradients. The spectra
are computed and compared inside one HIP kernel per resolution (``tts_stft_pair_sums``), which
returns three sums per waveform row; the losses are a few float64 torch ops on those sums.

Batching (new, optional): ``forward(y_hat, y, lengths=None, per_row=False)``. With ``lengths`` every
row counts as cut to its own length; ``per_row=True`` returns (B,) tensors whose entry b is the
reference's value on that cut row alone, ``per_row=False`` pools the sums over the valid frames of
all rows (with equal lengths: the reference's batch call).
"""

from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from ._lib import get_engine

_ROWS = 64  # rows per library call


def stft_frames(n_samples: int, n_fft: int, hop_length: int) -> int:
    """Frames of ``torch.stft(center=True)`` on ``n_samples`` samples."""
    return 1 + (n_samples + 2 * (n_fft // 2) - n_fft) // hop_length


def _check_resolution(n_fft, hop_length, win_length):
    if not 16 <= n_fft <= 2048:
        raise NotImplementedError(f"n_fft={n_fft} (16 to 2048 are built)")
    if not 16 <= win_length <= n_fft:
        raise NotImplementedError(f"win_length={win_length} (16 to n_fft={n_fft} are built)")
    if hop_length < 1:
        raise ValueError(f"hop_length={hop_length} must be at least 1")


def _rows(x, lengths, name="lengths"):
    """(B, L) float32 contiguous rows and their int64 lengths, checked as torch.stft checks them."""
    x = torch.as_tensor(x)
    eng = get_engine(x.device)
    if x.dim() != 2:
        raise ValueError(f"expected (B, L) waveform rows, got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    B, L = x.shape
    lens = np.full(B, L, np.int64) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), np.int64)
    if lens.shape != (B,) or (lens > L).any():
        raise ValueError(f"{name}: one value of at most L = {L} per row")
    return eng, x, lens


def _check_reflect(lens, n_fft):
    if (lens <= n_fft // 2).any():
        raise RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding "
                           f"({n_fft // 2}, {n_fft // 2}) at a row of {int(lens.min())} samples")


class TorchSTFT:
    """``losses.py:7-28``: magnitudes ``sqrt(clamp(re^2 + im^2, 1e-8))`` of ``torch.stft`` with a
    periodic Hann window, ``center=True`` and reflect padding: (B, L) -> (B, n_fft // 2 + 1, frames).
    With ``lengths`` row b is zero past its own ``stft_frames(lengths[b], ...)`` frames."""

    def __init__(self, n_fft, hop_length, win_length, window="hann_window"):
        if window != "hann_window":
            raise NotImplementedError(f"window={window!r} (only 'hann_window' is built)")
        _check_resolution(n_fft, hop_length, win_length)
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.window = torch.hann_window(win_length)

    @torch.no_grad()
    def __call__(self, x, lengths: Optional[Sequence[int]] = None):
        eng, x, lens = _rows(x, lengths)
        _check_reflect(lens, self.n_fft)
        B = x.shape[0]
        frames = max(stft_frames(int(n), self.n_fft, self.hop_length) for n in lens)
        mag = torch.empty(B, self.n_fft // 2 + 1, frames, device=x.device, dtype=torch.float32)
        with eng.lock:
            for b0 in range(0, B, _ROWS):
                eng.torch_stft_mag(x[b0:b0 + _ROWS], lens[b0:b0 + _ROWS], self.n_fft, self.win_length,
                                   self.hop_length, mag[b0:b0 + _ROWS])
        return mag


class STFTLoss(nn.Module):
    """``losses.py:36-52``: (mean |log y_M - log y_hat_M|, ||y_M - y_hat_M||_F / ||y_M||_F)."""

    def __init__(self, n_fft, hop_length, win_length):
        super().__init__()
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.stft = TorchSTFT(n_fft, hop_length, win_length)

    @torch.no_grad()
    def row_sums(self, y_hat, y, lengths=None):
        """(B, 3) float64 device tensor of per-row sums over the row's bins and frames: sum |log y_M -
        log y_hat_M|, sum (y_M - y_hat_M)^2, sum y_M^2; and the rows' element counts bins * frames."""
        eng, y, lens = _rows(y, lengths)
        _, y_hat, _ = _rows(y_hat, None)
        if y_hat.shape != y.shape:
            raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} differ in shape")
        _check_reflect(lens, self.n_fft)
        B = y.shape[0]
        sums = torch.empty(B, 3, device=y.device, dtype=torch.float64)
        with eng.lock:
            for b0 in range(0, B, _ROWS):
                eng.stft_pair_sums(y_hat[b0:b0 + _ROWS], y[b0:b0 + _ROWS], lens[b0:b0 + _ROWS], self.n_fft,
                                   self.win_length, self.hop_length, sums[b0:b0 + _ROWS])
        counts = np.array([(self.n_fft // 2 + 1) * stft_frames(int(n), self.n_fft, self.hop_length) for n in lens],
                          np.float64)
        return sums, torch.from_numpy(counts).to(y.device)

    def forward(self, y_hat, y, lengths=None, per_row=False):
        return _combine([self.row_sums(y_hat, y, lengths)], per_row)


def _combine(parts, per_row):
    """The mean over the resolutions of (sum A / count, sqrt(sum D) / sqrt(sum R)), in float64, from
    each resolution's (sums (R, 3), counts (R,)): per row, or pooled over the rows."""
    loss_mag = loss_sc = 0
    for sums, counts in parts:
        if not per_row:
            sums, counts = sums.sum(0), counts.sum()
        loss_mag = loss_mag + sums[..., 0] / counts
        loss_sc = loss_sc + torch.sqrt(sums[..., 1]) / torch.sqrt(sums[..., 2])
    return (loss_mag / len(parts)).float(), (loss_sc / len(parts)).float()


class MultiScaleSTFTLoss(nn.Module):
    """``losses.py:54-75``: the mean of `STFTLoss` over the resolutions."""

    def __init__(self, n_ffts=(1024, 2048, 512), hop_lengths=(120, 240, 50), win_lengths=(600, 1200, 240)):
        super().__init__()
        self.loss_funcs = nn.ModuleList()
        for n_fft, hop_length, win_length in zip(n_ffts, hop_lengths, win_lengths):
            self.loss_funcs.append(STFTLoss(n_fft, hop_length, win_length))

    def _parts(self, y_hat, y, lengths):
        return [f.row_sums(y_hat, y, lengths) for f in self.loss_funcs]

    def forward(self, y_hat, y, lengths=None, per_row=False):
        return _combine(self._parts(y_hat, y, lengths), per_row)

    def pooled_and_rows(self, y_hat, y, lengths=None):
        """``forward(..., per_row=False)`` and ``forward(..., per_row=True)`` from one pass over the signals."""
        parts = self._parts(y_hat, y, lengths)
        return _combine(parts, False), _combine(parts, True)


def subband_rows(x):
    """``x.view(-1, 1, L).squeeze(1)`` of ``losses.py:81-84``: (B, C, L) -> (B * C, L), row b * C + c."""
    return x.reshape(-1, x.shape[2])


class MultiScaleSubbandSTFTLoss(MultiScaleSTFTLoss):
    """``losses.py:78-84``: `MultiScaleSTFTLoss` on the (B, C, L) sub-bands viewed as B * C rows.
    ``lengths`` are per utterance and apply to all its bands; ``per_row=True`` returns one value per
    utterance, its C band rows pooled (the reference's call on that utterance alone)."""

    def _parts(self, y_hat, y, lengths):
        y_hat, y = torch.as_tensor(y_hat), torch.as_tensor(y)
        if y.dim() != 3 or y_hat.shape != y.shape:
            raise ValueError(f"expected two (B, C, L) tensors, got {tuple(y_hat.shape)} and {tuple(y.shape)}")
        B, C, _ = y.shape
        if lengths is not None:
            lengths = np.repeat(np.asarray(torch.as_tensor(lengths).cpu(), np.int64), C)
        parts = super()._parts(subband_rows(y_hat), subband_rows(y), lengths)
        return [(sums.view(B, C, 3).sum(1), counts.view(B, C).sum(1)) for sums, counts in parts]
