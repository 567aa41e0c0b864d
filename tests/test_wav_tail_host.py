"""Host side of the waveform tail on the GPU: the `wav_tail_device` keyword, the default processor's
inv_spectrogram / find_endpoint / save_wav results unchanged, the three library entries declared,
typed and exported, the no-CPU-fallback error of the batch methods, and the per-channel affine form
`inv_spectrogram_batch` hands to tts_spec_to_mag."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal
import torch

from tts_amd.audio import AudioProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ_AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0,
                ref_level_db=20, power=1.5, griffin_lim_iters=8, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0,
                spec_gain=20, signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0,
                clip_norm=True)
ENTRIES = ("tts_spec_to_mag", "tts_deemphasis", "tts_wav_finish")


def test_wav_tail_device_keyword():
    assert AudioProcessor(**LJ_AUDIO).wav_tail_device is None
    assert AudioProcessor(**LJ_AUDIO, wav_tail_device="gpu").wav_tail_device == "gpu"
    assert AudioProcessor(**LJ_AUDIO, wav_tail_device="cpu").wav_tail_device == "cpu"
    with pytest.raises(ValueError, match="wav_tail_device"):
        AudioProcessor(**LJ_AUDIO, wav_tail_device="tpu")


@pytest.mark.parametrize("preemphasis", [0.0, 0.97])
def test_default_inv_spectrogram_unchanged(preemphasis):
    """Against the formula of audio.py:232-239 written out here, for the default processor and for
    wav_tail_device="cpu" / "gpu" (the key moves nothing inside AudioProcessor's host methods)."""
    audio = dict(LJ_AUDIO, preemphasis=preemphasis)
    ap = AudioProcessor(**audio)
    t = np.arange(256 * 11) / 22050.0
    spec = ap.spectrogram(0.3 * np.sin(2 * np.pi * (200 + 300 * t) * t))
    S = np.power(10.0, ap._denormalize(spec) / 20.0) ** 1.5
    ref = ap._griffin_lim(S, np.random.RandomState(1))
    if preemphasis:
        ref = scipy.signal.lfilter([1], [1, -preemphasis], ref)
    for kw in ({}, {"wav_tail_device": "cpu"}, {"wav_tail_device": "gpu"}):
        y = AudioProcessor(**audio, **kw).inv_spectrogram(spec, np.random.RandomState(1))
        assert y.dtype == np.float64 and np.array_equal(y, ref), kw


def _endpoint(wav, window, hop, threshold):
    for x in range(hop, len(wav) - window, hop):
        if np.max(wav[x:x + window]) < threshold:
            return x + hop
    return len(wav)


@pytest.mark.parametrize("sample_rate", [22050, 22052])
def test_default_find_endpoint_and_save_wav_unchanged(sample_rate):
    ap = AudioProcessor(**dict(LJ_AUDIO, sample_rate=sample_rate), wav_tail_device="gpu")
    window = int(sample_rate * 0.8)
    rs = np.random.RandomState(4)
    wav = (0.2 * rs.randn(60000)).astype(np.float32)
    wav[30000:] *= 0.01
    wav[41000] = -0.5
    end = ap.find_endpoint(wav)
    assert end == _endpoint(wav, window, int(window / 4), 0.01) and 30000 < end < 60000
    assert ap.find_endpoint(wav[:window]) == window
    buf = io.BytesIO()
    ap.save_wav(wav[:end], buf)
    sr, pcm = scipy.io.wavfile.read(io.BytesIO(buf.getvalue()))
    factor = np.float32(32767) / np.abs(wav[:end]).max()
    assert sr == sample_rate and pcm.dtype == np.int16
    assert np.array_equal(pcm, (wav[:end] * factor).astype(np.int16))
    quiet = (wav[:5000] * np.float32(1e-3)).astype(np.float32)
    assert np.abs(quiet).max() < 0.01
    buf = io.BytesIO()
    ap.save_wav(quiet, buf)
    _, pcm = scipy.io.wavfile.read(io.BytesIO(buf.getvalue()))
    assert np.array_equal(pcm, (quiet * np.float32(3276700.0)).astype(np.int16))


def test_entries_declared_typed_and_exported():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    src = open(os.path.join(ROOT, "include", "ttship.h")).read()
    typed = {n: args for n, _, args in SIGNATURES}
    lib = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl, name
        assert len(typed[name]) == len(decl.group(1).split(",")), name
        assert hasattr(lib, name), name
    # the doubles of the header are doubles in the binding
    assert typed["tts_deemphasis"][5] is ctypes.c_double
    assert typed["tts_wav_finish"][7] is ctypes.c_double


def test_cpu_tensors_have_no_fallback():
    ap = AudioProcessor(**dict(LJ_AUDIO, preemphasis=0.97), griffin_lim_device="gpu", wav_tail_device="gpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.inv_spectrogram_batch(torch.zeros(1, 12, 513), [12])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.deemphasis_batch(torch.zeros(1, 100), [100])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.finish_batch(torch.zeros(1, 100), [100])


def test_inv_spectrogram_batch_behind_the_griffin_lim_fence():
    ap = AudioProcessor(**dict(LJ_AUDIO, fft_size=2048), griffin_lim_device="gpu")
    with pytest.raises(NotImplementedError, match="fft_size"):
        ap.inv_spectrogram_batch(torch.zeros(1, 12, 1025), [12])


def test_linear_denorm_affine_matches_denormalize():
    """The (scale, offset, clip) form handed to tts_spec_to_mag against `_denormalize` on 513 bins,
    for the settings of test_denorm_affine_matches_denormalize; the mel form is what it was."""
    x = np.random.RandomState(2).uniform(-5, 5, (513, 9))
    for kw in ({}, {"symmetric_norm": False}, {"clip_norm": False}, {"signal_norm": False}):
        ap = AudioProcessor(**dict(LJ_AUDIO, **kw))
        scale, offset, clip = ap._denorm_affine(513)
        assert scale.shape == offset.shape == (513,)
        y = x if clip is None else np.clip(x, *clip)
        assert np.abs(y * scale[:, None] + offset[:, None] - ap._denormalize(x)).max() <= 1e-12
        mel = ap._denorm_affine()
        assert mel[0].shape == (80,) and mel[0][0] == scale[0] and mel[1][0] == offset[0] and mel[2] == clip


def test_linear_denorm_affine_with_stats_follows_scaler_for(tmp_path):
    """Mean-var stats: 513 bins are refused as `_denormalize` refuses them (the reference compares
    with fft_size / 2), 512 channels pick the linear scaler, and the mel form is untouched."""
    rs = np.random.RandomState(11)
    st = {"mel_mean": rs.uniform(-3, -1, 80), "mel_std": rs.uniform(0.3, 0.8, 80),
          "linear_mean": rs.uniform(-3, -1, 512), "linear_std": rs.uniform(0.3, 0.8, 512)}
    acfg = {k: v for k, v in LJ_AUDIO.items() if k not in ("max_norm", "min_level_db", "symmetric_norm", "clip_norm")}
    acfg["stats_path"] = str(tmp_path / "scale_stats.npy")
    st["audio_config"] = acfg
    np.save(tmp_path / "scale_stats.npy", st, allow_pickle=True)
    ap = AudioProcessor(**dict(LJ_AUDIO, stats_path=acfg["stats_path"]), griffin_lim_device="gpu")
    with pytest.raises(RuntimeError, match="Mean-Var stats") as host:
        ap._denormalize(np.zeros((513, 3)))
    with pytest.raises(RuntimeError, match="Mean-Var stats") as affine:
        ap._denorm_affine(513)
    assert str(host.value) == str(affine.value)
    x = rs.uniform(-2, 2, (512, 5))
    scale, offset, clip = ap._denorm_affine(512)
    assert clip is None and np.abs(x * scale[:, None] + offset[:, None] - ap._denormalize(x)).max() <= 1e-12
    scale, offset, clip = ap._denorm_affine()
    assert np.array_equal(scale, st["mel_std"]) and np.array_equal(offset, st["mel_mean"]) and clip is None
