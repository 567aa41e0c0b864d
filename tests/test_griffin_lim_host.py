"""Host side of the GPU Griffin-Lim option: the default stays the CPU path, bit for bit; what the
GPU path does not cover is refused by name; a CPU tensor gets the library's no-CPU-fallback error."""
import os
import re

import numpy as np
import pytest
import torch

from tts_amd.audio import AudioProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ_AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0,
                ref_level_db=20, power=1.5, griffin_lim_iters=8, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0,
                spec_gain=1, signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0,
                clip_norm=True)


def _mel(ap, M=12):
    n = ap.hop_length * (M - 1)
    t = np.arange(n) / ap.sample_rate
    y = 0.3 * np.sin(2 * np.pi * (200 + 300 * t) * t) + 0.05 * np.random.RandomState(3).randn(n)
    return ap.melspectrogram(y)


def test_default_processor_stays_on_cpu_bit_for_bit():
    ap = AudioProcessor(**LJ_AUDIO)
    assert getattr(ap, "griffin_lim_device", None) is None
    mel = _mel(ap)
    S = np.maximum(1e-10, ap.inv_mel_basis @ ap._db_to_amp(ap._denormalize(mel))) ** ap.power
    direct = ap._griffin_lim(S, np.random.RandomState(1))
    wav = ap.inv_melspectrogram(mel, rng=np.random.RandomState(1))
    assert wav.dtype == np.float64 and np.array_equal(wav, direct)
    np.random.seed(5)
    a = ap.inv_melspectrogram(mel)
    np.random.seed(5)
    assert np.array_equal(a, ap._griffin_lim(S))
    assert np.array_equal(AudioProcessor(**LJ_AUDIO, griffin_lim_device="cpu").inv_melspectrogram(
        mel, rng=np.random.RandomState(1)), direct)


def test_griffin_lim_device_keyword():
    assert AudioProcessor(**LJ_AUDIO, griffin_lim_device="gpu").griffin_lim_device == "gpu"
    assert AudioProcessor(**LJ_AUDIO, griffin_lim_device="cpu").griffin_lim_device == "cpu"
    with pytest.raises(ValueError, match="griffin_lim_device"):
        AudioProcessor(**LJ_AUDIO, griffin_lim_device="tpu")


@pytest.mark.parametrize("name,override", [("stft_pad_mode", {"stft_pad_mode": "constant"}),
                                           ("fft_size", {"fft_size": 2048}),
                                           ("hop_length", {"hop_length": 32})])
def test_unsupported_parameters_are_named(name, override):
    ap = AudioProcessor(**dict(LJ_AUDIO, griffin_lim_device="gpu", **override))
    with pytest.raises(NotImplementedError, match=name):
        ap.inv_melspectrogram_batch(torch.zeros(1, 12, 80), [12])


def test_cpu_tensor_has_no_fallback():
    ap = AudioProcessor(**LJ_AUDIO, griffin_lim_device="gpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.inv_melspectrogram_batch(torch.zeros(1, 12, 80), [12])


def test_denorm_affine_matches_denormalize():
    """The (scale, offset, clip) form handed to tts_mel_to_linear against `_denormalize`."""
    x = np.random.RandomState(2).uniform(-5, 5, (80, 9))
    for kw in ({}, {"symmetric_norm": False}, {"clip_norm": False}, {"signal_norm": False}):
        ap = AudioProcessor(**dict(LJ_AUDIO, **kw))
        scale, offset, clip = ap._denorm_affine()
        y = x if clip is None else np.clip(x, *clip)
        assert np.abs(y * scale[:, None] + offset[:, None] - ap._denormalize(x)).max() <= 1e-12


def test_header_declares_the_audio_entries():
    src = open(os.path.join(ROOT, "include", "ttship.h")).read()
    for name in ("tts_mel_to_linear", "tts_griffin_lim"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
