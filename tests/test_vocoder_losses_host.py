"""Host side of the vocoder scoring (tts_amd.vocoder_losses, tts_amd.vocoder_eval, PQMF.analysis): the
reference's names, signatures and defaults, the sub-band row order, the arithmetic from row sums to
losses, the fences that need no device, and the library's no-CPU-fallback error."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import tts_amd
import vocoder_eval_cases as vc
from tts_amd import vocoder_eval, vocoder_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tts_pqmf_analysis", "tts_stft_pair_sums", "tts_torch_stft_mag")


def _params(fn):
    return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def test_names_and_constructor_signatures_match_the_reference():
    """TTS/vocoder/layers/losses.py:7-84, restated: argument names, order and defaults."""
    E = inspect.Parameter.empty
    assert _params(tts_amd.TorchSTFT.__init__) == [("n_fft", E), ("hop_length", E), ("win_length", E),
                                                    ("window", "hann_window")]
    assert _params(tts_amd.STFTLoss.__init__) == [("n_fft", E), ("hop_length", E), ("win_length", E)]
    multi = [("n_ffts", (1024, 2048, 512)), ("hop_lengths", (120, 240, 50)), ("win_lengths", (600, 1200, 240))]
    assert _params(tts_amd.MultiScaleSTFTLoss.__init__) == multi
    assert _params(tts_amd.MultiScaleSubbandSTFTLoss.__init__) == multi
    assert issubclass(tts_amd.MultiScaleSubbandSTFTLoss, tts_amd.MultiScaleSTFTLoss)
    for cls in (tts_amd.STFTLoss, tts_amd.MultiScaleSTFTLoss):
        assert issubclass(cls, torch.nn.Module)
        assert _params(cls.forward) == [("y_hat", E), ("y", E), ("lengths", None), ("per_row", False)]
    m = tts_amd.MultiScaleSTFTLoss()
    assert [(f.n_fft, f.hop_length, f.win_length) for f in m.loss_funcs] == list(vc.FULLBAND)
    f = m.loss_funcs[0]
    assert isinstance(f.stft, tts_amd.TorchSTFT)
    assert (f.stft.n_fft, f.stft.hop_length, f.stft.win_length) == vc.FULLBAND[0]
    assert torch.equal(f.stft.window, torch.hann_window(600))
    assert len(m.state_dict()) == 0  # as in the reference: the windows are no buffers
    assert tts_amd.copy_synthesis_scores is vocoder_eval.copy_synthesis_scores
    sub = vocoder_eval.SUBBAND_STFT_LOSS_PARAMS
    assert list(zip(sub["n_ffts"], sub["hop_lengths"], sub["win_lengths"])) == list(vc.SUBBAND)


def test_subband_rows_follow_the_reference_view():
    x = torch.arange(2 * 4 * 5, dtype=torch.float32).reshape(2, 4, 5)
    rows = vocoder_losses.subband_rows(x)
    assert torch.equal(rows, x.view(-1, 1, x.shape[2]).squeeze(1))
    assert torch.equal(rows[1 * 4 + 2], x[1, 2])
    assert torch.equal(vocoder_losses.subband_rows(x.transpose(0, 1).contiguous().transpose(0, 1)), rows)


def test_frame_formula_for_both_parities():
    for n_fft, hop, n in ((1024, 120, 513), (1024, 120, 2040), (683, 60, 342), (683, 60, 1380), (171, 10, 339)):
        want = 1 + (n // hop if n_fft % 2 == 0 else (n - 1) // hop)
        assert vocoder_losses.stft_frames(n, n_fft, hop) == want == vc.stft_frames(n, n_fft, hop)
        assert want == torch.stft(torch.zeros(n), n_fft, hop, min(n_fft, 60), torch.hann_window(min(n_fft, 60)),
                                  center=True, pad_mode="reflect", return_complex=True).shape[1]


def test_losses_from_row_sums():
    """loss_mag = sum A / (F sum frames), loss_sc = sqrt(sum D) / sqrt(sum R), averaged over the
    resolutions: pooled over the rows, or per row."""
    s1 = torch.tensor([[6.0, 4.0, 16.0], [2.0, 5.0, 20.0]], dtype=torch.float64)
    c1 = torch.tensor([12.0, 4.0], dtype=torch.float64)
    s2 = torch.tensor([[1.0, 1.0, 4.0], [3.0, 8.0, 32.0]], dtype=torch.float64)
    c2 = torch.tensor([2.0, 6.0], dtype=torch.float64)
    mg, sc = vocoder_losses._combine([(s1, c1), (s2, c2)], per_row=False)
    assert mg.dtype == sc.dtype == torch.float32 and mg.shape == sc.shape == ()
    assert float(mg) == np.float32((8 / 16 + 4 / 8) / 2)
    assert float(sc) == np.float32((np.sqrt(9) / np.sqrt(36) + np.sqrt(9) / np.sqrt(36)) / 2)
    mg, sc = vocoder_losses._combine([(s1, c1), (s2, c2)], per_row=True)
    assert mg.tolist() == [np.float32((0.5 + 0.5) / 2), np.float32((0.5 + 0.5) / 2)]
    assert sc.tolist() == [np.float32((0.5 + 0.5) / 2), np.float32((0.5 + 0.5) / 2)]


def test_fences_that_need_no_device():
    with pytest.raises(NotImplementedError, match="n_fft"):
        tts_amd.STFTLoss(2049, 120, 600)
    with pytest.raises(NotImplementedError, match="n_fft"):
        tts_amd.TorchSTFT(8, 2, 8)
    with pytest.raises(NotImplementedError, match="win_length"):
        tts_amd.MultiScaleSTFTLoss((1024,), (120,), (1025,))
    with pytest.raises(NotImplementedError, match="win_length"):
        tts_amd.TorchSTFT(1024, 120, 15)
    with pytest.raises(ValueError, match="hop_length"):
        tts_amd.TorchSTFT(1024, 0, 600)
    with pytest.raises(NotImplementedError, match="window"):
        tts_amd.TorchSTFT(1024, 120, 600, window="hamming_window")
    with pytest.raises(ValueError, match="inference_padding"):
        tts_amd.copy_synthesis_scores(types.SimpleNamespace(inference_padding=2), None, torch.zeros(1, 4096), [4096])
    with pytest.raises(ValueError, match="analysis_device"):
        tts_amd.copy_synthesis_scores(types.SimpleNamespace(inference_padding=0),
                                      types.SimpleNamespace(analysis_device=None), torch.zeros(1, 4096), [4096])


def test_cpu_tensors_have_no_fallback():
    y = torch.zeros(2, 4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tts_amd.TorchSTFT(1024, 120, 600)(y)
    for loss in (tts_amd.STFTLoss(1024, 120, 600), tts_amd.MultiScaleSTFTLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(y, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tts_amd.MultiScaleSubbandSTFTLoss()(y.view(1, 2, 4096), y.view(1, 2, 4096))
    p = tts_amd.PQMF()
    for fn in (p.analysis, p.forward, tts_amd.MultibandMelganGenerator(upsample_factors=(8, 4, 2)).pqmf_analysis):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(1, 1, 64))


def test_header_declares_and_library_exports_the_entries():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    src = open(os.path.join(ROOT, "include", "ttship.h")).read()
    typed = {n: a for n, _, a in SIGNATURES}
    lib = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(typed[name]) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), name


def test_signals_are_reproducible():
    """The fixture stores seeds only: the signals the tests rebuild are float32 and fixed by the seed."""
    y_hat, y = vc.pair(1000, 513)
    assert y.dtype == y_hat.dtype == np.float32 and y.shape == y_hat.shape == (513,)
    assert np.array_equal(vc.pair(1000, 513)[1], y) and not np.array_equal(vc.pair(1001, 513)[1], y)
    assert 0.1 < np.abs(y).max() < 1.0
    assert vc.resolution_lengths(2048, 240) == (1025, 4080, 4079) and 4080 <= 4200
