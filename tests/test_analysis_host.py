"""Host side of the GPU analysis option (tts_stft_mag, tts_mag_to_feature, AudioProcessor's
``analysis_device``, SpeakerEncoder.compute_embedding_batch): the default stays the CPU path, bit for
bit; the affine form handed to the kernel equals `_normalize`; what the GPU path does not cover is
refused by name; a CPU tensor gets the library's no-CPU-fallback error."""
import ctypes
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


def _speech(ap, M=12):
    n = ap.hop_length * (M - 1)
    t = np.arange(n) / ap.sample_rate
    return 0.3 * np.sin(2 * np.pi * (200 + 300 * t) * t) + 0.05 * np.random.RandomState(3).randn(n)


@pytest.mark.parametrize("kw", [{}, {"preemphasis": 0.97, "spec_gain": 20}, {"analysis_device": "cpu"}])
def test_default_processor_stays_on_cpu_bit_for_bit(kw):
    ap = AudioProcessor(**dict(LJ_AUDIO, **kw))
    assert ap.analysis_device == kw.get("analysis_device")
    y = _speech(ap)
    mag = np.abs(ap._preemph_stft(y))
    mel = ap.melspectrogram(y)
    assert mel.dtype == np.float64 and mel.shape == (80, 12)
    assert np.array_equal(mel, ap._normalize(ap._amp_to_db(ap.mel_basis @ mag)))
    assert np.array_equal(ap.spectrogram(y), ap._normalize(ap._amp_to_db(mag)))


def test_analysis_device_keyword():
    assert AudioProcessor(**LJ_AUDIO).analysis_device is None
    assert AudioProcessor(**LJ_AUDIO, analysis_device="gpu").analysis_device == "gpu"
    assert AudioProcessor(**LJ_AUDIO, analysis_device="cpu").analysis_device == "cpu"
    with pytest.raises(ValueError, match="analysis_device"):
        AudioProcessor(**LJ_AUDIO, analysis_device="tpu")


def _stats_kw(tmp_path):
    """A mean-var stats file written as TTS/bin/compute_statistics.py writes it (the recipe of
    tests/test_griffin_lim.py case 5)."""
    rs = np.random.RandomState(11)
    st = {"mel_mean": rs.uniform(-3, -1, 80), "mel_std": rs.uniform(0.3, 0.8, 80),
          "linear_mean": rs.uniform(-3, -1, 513), "linear_std": rs.uniform(0.3, 0.8, 513)}
    acfg = {k: v for k, v in LJ_AUDIO.items() if k not in ("max_norm", "min_level_db", "symmetric_norm", "clip_norm")}
    acfg["stats_path"] = str(tmp_path / "scale_stats.npy")
    st["audio_config"] = acfg
    np.save(tmp_path / "scale_stats.npy", st, allow_pickle=True)
    return {"stats_path": acfg["stats_path"]}


@pytest.mark.parametrize("norm", ["symmetric", "asymmetric", "none", "meanvar"])
@pytest.mark.parametrize("C", [80, 513])
def test_norm_affine_matches_normalize(norm, C, tmp_path):
    """The (scale, offset, clip) form handed to tts_mag_to_feature against `_normalize`, on dB values
    that reach past both clip bounds."""
    kw = {"symmetric": {}, "asymmetric": {"symmetric_norm": False}, "none": {"signal_norm": False}}.get(norm)
    ap = AudioProcessor(**dict(LJ_AUDIO, **(_stats_kw(tmp_path) if kw is None else kw)))
    assert hasattr(ap, "mel_scaler") == (norm == "meanvar")
    S = np.random.RandomState(2).uniform(-140, 60, (C, 9))
    if norm == "meanvar" and C == 513:  # the reference compares the linear size with fft_size / 2
        with pytest.raises(RuntimeError, match="Mean-Var stats") as e1:
            ap._normalize(S)
        with pytest.raises(RuntimeError, match="Mean-Var stats") as e2:
            ap._norm_affine(C)
        assert str(e1.value) == str(e2.value)
        return
    scale, offset, clip = ap._norm_affine(C)
    assert scale.shape == offset.shape == (C,)
    assert (clip is not None) == (norm in ("symmetric", "asymmetric"))
    y = S * scale[:, None] + offset[:, None]
    y = y if clip is None else np.clip(y, *clip)
    ref = ap._normalize(S)
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"norm_affine {norm} C={C}: {err:.3e}")
    assert err <= 1e-12
    noclip = AudioProcessor(**dict(LJ_AUDIO, clip_norm=False))
    assert noclip._norm_affine(C)[2] is None


@pytest.mark.parametrize("name,override", [("stft_pad_mode", {"stft_pad_mode": "constant"}),
                                           ("fft_size", {"fft_size": 4096}),
                                           ("fft_size", {"fft_size": 32, "win_length": 32, "hop_length": 16}),
                                           ("fft_size", {"fft_size": 511, "win_length": 400}),
                                           ("hop_length", {"hop_length": 8}),
                                           ("hop_length", {"hop_length": 1100})])
def test_unsupported_parameters_are_named(name, override):
    ap = AudioProcessor(**dict(LJ_AUDIO, analysis_device="gpu", **override))
    for fn in (ap.melspectrogram_batch, ap.spectrogram_batch):
        with pytest.raises(NotImplementedError, match=name):
            fn(torch.zeros(1, 4096), [4096])


def test_cpu_tensor_has_no_fallback():
    ap = AudioProcessor(**LJ_AUDIO, analysis_device="gpu")
    for fn in (ap.melspectrogram_batch, ap.spectrogram_batch):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(1, 4096), [4096])


def test_header_declares_and_library_exports_the_analysis_entries():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    src = open(os.path.join(ROOT, "include", "ttship.h")).read()
    typed = {n for n, _, _ in SIGNATURES}
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("tts_stft_mag", "tts_mag_to_feature"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in typed, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("T", [1, 79, 80, 160, 161, 400])
def test_embedding_windows_match_the_reference_loop(T):
    """The window list of compute_embedding_batch against the (offset, end) pairs of the loop of
    TTS/speaker_encoder/model.py:77-84."""
    from tts_amd.speaker_encoder import SpeakerEncoder
    num_frames, overlap = 160, 0.5
    num_overlap = int(num_frames * overlap)
    ref = []
    for offset in range(0, T, num_frames - num_overlap):
        ref.append((offset, min(T, offset + num_frames)))
    assert SpeakerEncoder.embedding_windows(T, num_frames, overlap) == ref
    assert SpeakerEncoder.embedding_windows(T) == ref
