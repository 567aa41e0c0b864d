"""Scoring a vocoder by copy-synthesis on MI355X: waveform -> mel -> vocoder -> multi-resolution STFT
distances between the result and the input, the ``G_stft_loss_*`` / ``G_subband_stft_loss_*`` figures
of ``TTS/bin/train_vocoder.py`` ``evaluate()``. Every step runs on the device; only the scores leave it.
"""

import numpy as np
import torch

from .vocoder import MultibandMelganGenerator
from .vocoder_losses import MultiScaleSTFTLoss, MultiScaleSubbandSTFTLoss

# the sub-band resolutions of the reference's multiband_melgan_config.json
SUBBAND_STFT_LOSS_PARAMS = dict(n_ffts=[384, 683, 171], hop_lengths=[30, 60, 10], win_lengths=[150, 300, 60])


@torch.no_grad()
def copy_synthesis_scores(vocoder, ap, wavs, lengths, stft_loss_params=None, subband_stft_loss_params=None):
    """``wavs``: (B, L) waveform rows on a ROCm device, row b valid for ``lengths[b]`` samples; ``ap``:
    an `AudioProcessor` with ``analysis_device="gpu"``; ``vocoder``: a generator of `tts_amd.vocoder`
    with ``inference_padding == 0``. Returns a dict of floats and per-row float lists:

    ``G_stft_loss_mg`` / ``G_stft_loss_sc``: `MultiScaleSTFTLoss` between ``vocoder.inference(mel)`` and
    the input, both cut to ``lengths[b]``, pooled over the rows; ``<key>_rows``: each row on its own.
    For a `MultibandMelganGenerator` also ``G_subband_stft_loss_mg`` / ``_sc`` (and ``_rows``):
    `MultiScaleSubbandSTFTLoss` between the generator's sub-bands and ``pqmf_layer.analysis(wavs)``, cut
    to the shorter of the two per row."""
    if int(vocoder.inference_padding) != 0:
        raise ValueError(f"copy_synthesis_scores needs vocoder.inference_padding == 0 (got "
                         f"{vocoder.inference_padding}): padded frames would shift the copy against the input")
    if getattr(ap, "analysis_device", None) != "gpu":
        raise ValueError("copy_synthesis_scores needs an AudioProcessor with analysis_device='gpu'")
    wavs = torch.as_tensor(wavs)
    if wavs.dim() != 2:
        raise ValueError(f"expected (B, L) waveform rows, got {tuple(wavs.shape)}")
    lengths = [int(n) for n in lengths]
    mel, frames = ap.melspectrogram_batch(wavs, lengths)
    mel = mel.transpose(1, 2)
    y_hat = vocoder.inference(mel, lengths=frames)[:, 0]
    L = wavs.shape[1]
    if y_hat.shape[1] < L:
        y_hat = torch.nn.functional.pad(y_hat, (0, L - y_hat.shape[1]))
    full = MultiScaleSTFTLoss(**(stft_loss_params or {}))
    scores = {}

    def put(key, loss, a, b, lens):
        for suffix, (mg, sc) in zip(("", "_rows"), loss.pooled_and_rows(a, b, lengths=lens)):
            scores[f"G_{key}_mg{suffix}"] = mg.cpu().tolist()
            scores[f"G_{key}_sc{suffix}"] = sc.cpu().tolist()

    put("stft_loss", full, y_hat[:, :L], wavs, lengths)
    if isinstance(vocoder, MultibandMelganGenerator):
        sub = MultiScaleSubbandSTFTLoss(**(subband_stft_loss_params or SUBBAND_STFT_LOSS_PARAMS))
        bands_hat = vocoder.generator(mel, lengths=frames)
        bands = vocoder.pqmf_layer.analysis(wavs[:, None, :], lengths=lengths)
        N = vocoder.pqmf_layer.N
        up = vocoder.hop // N
        lens = [min(up * m, (n - 1) // N + 1) for m, n in zip(frames, lengths)]
        Ls = min(bands_hat.shape[2], bands.shape[2])
        put("subband_stft_loss", sub, bands_hat[:, :, :Ls], bands[:, :, :Ls], np.minimum(lens, Ls))
    return scores
