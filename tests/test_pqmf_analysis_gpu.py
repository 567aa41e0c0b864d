"""PQMF.analysis on the GPU (tts_pqmf_analysis) against the reference in float64
(tests/golden/vocoder_eval.npz, written by tests/golden/make_vocoder_eval_golden.py).

Yardstick: the float64 fixture; a tensor of largest magnitude v may differ from it by at most
8 x max(the reference's own float32-vs-float64 deviation over that tensor, 2^-23 v)
(vocoder_eval_cases.tolerance). Every error is printed next to its tolerance before it is asserted.
"""
import numpy as np
import pytest
import torch

import vocoder_eval_cases as vc
from helpers import load_fixture

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ragged():
    """The seven fixture rows in one call, the caller's padding filled with 1e3."""
    from tts_amd import PQMF
    dev = _dev()
    p = PQMF().to(dev)
    rows = [vc.signal(vc.PQMF_SEED + j, n) for j, n in enumerate(vc.PQMF_LENGTHS)]
    x = np.full((len(rows), max(vc.PQMF_LENGTHS)), 1e3, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    y = p.analysis(torch.from_numpy(x[:, None, :]).to(dev), lengths=list(vc.PQMF_LENGTHS))
    return p, rows, y


def test_ragged_rows_match_the_reference(ragged):
    _, rows, y = ragged
    fx = load_fixture("vocoder_eval")
    assert y.shape == (7, 4, (1001 - 1) // 4 + 1) and y.dtype == torch.float32
    y = y.cpu().numpy()
    for b, n in enumerate(vc.PQMF_LENGTHS):
        ref, Lout = fx[f"pqmf_{n}"], (n - 1) // 4 + 1
        assert ref.shape == (4, Lout)
        err, tol = np.abs(y[b, :, :Lout] - ref).max(), vc.tolerance(fx[f"pqmf_{n}_dev"], ref)
        print(f"pqmf analysis len {n}: err {err:.3e} tol {tol:.3e} (reference float32 dev {fx[f'pqmf_{n}_dev']:.3e})")
        assert err <= tol, n
        assert (y[b, :, Lout:] == 0).all(), n


def test_each_row_equals_its_own_call(ragged):
    p, rows, y = ragged
    for b, r in enumerate(rows):
        single = p.analysis(torch.from_numpy(r[None, None, :]).to(y.device))
        assert single.shape == (1, 4, (len(r) - 1) // 4 + 1)
        assert torch.equal(single[0], y[b, :, :single.shape[2]]), len(r)


def test_example_wav_bands_and_round_trip():
    """The reference's example wav: analysis against its stored bands, the deviation term taken from
    those float32 bands against a float64 convolution; then synthesis(analysis(wav)) against
    TTS/vocoder/pqmf_output.wav with test_gpu_parity.py::test_pqmf_known_answer_wav's bound."""
    from tts_amd import PQMF
    dev = _dev()
    fx = load_fixture("pqmf")
    p = PQMF().to(dev)
    assert np.array_equal(p.H.cpu().numpy(), fx["H"])
    wav = fx["example_wav_int16"].astype(np.float32) / 32768.0
    ref64 = vc.pqmf_analysis64(wav, fx["H"][:, 0, :])
    assert ref64.shape == fx["example_bands"].shape[1:]
    dev32 = np.abs(fx["example_bands"][0] - ref64).max()
    x = torch.from_numpy(wav[None, None, :]).to(dev)
    for name, bands in (("analysis", p.analysis(x)), ("forward", p.forward(x))):
        assert bands.shape == fx["example_bands"].shape
        err, tol = np.abs(bands[0].cpu().numpy() - ref64).max(), vc.tolerance(dev32, ref64)
        print(f"pqmf {name} example wav: err {err:.3e} tol {tol:.3e} (reference float32 dev {dev32:.3e})")
        assert err <= tol
    rec = p.synthesis(p.analysis(x)).cpu().numpy()[0, 0]
    ka = fx["known_answer_int16"].astype(np.float64)
    n = len(ka) - 64
    lsb = np.abs(rec[:n].astype(np.float64) * 32768.0 - ka[:n]).max()
    print(f"pqmf round trip vs pqmf_output.wav: {lsb:.3f} LSB (bound 2.0)")
    assert lsb <= 2.0


def test_multiband_generator_analysis_and_fences():
    from tts_amd import PQMF, MultibandMelganGenerator
    dev = _dev()
    v = MultibandMelganGenerator(upsample_factors=(8, 4, 2)).to(dev)
    x = torch.from_numpy(vc.signal(7, 1001)[None, None, :]).to(dev)
    assert torch.equal(v.pqmf_analysis(x), PQMF().to(dev).analysis(x))
    with pytest.raises(ValueError, match=r"\(B, 1, L\)"):
        v.pqmf_analysis(x[0])
    with pytest.raises(RuntimeError, match="pqmf_analysis") as e:  # the library's own fence: 65 rows
        from tts_amd._lib import get_engine
        H = v.pqmf_layer.H.reshape(4, -1).contiguous()
        get_engine(dev).pqmf_analysis(torch.zeros(65, 8, device=dev), [8] * 65, H, torch.zeros(65, 4, 2, device=dev))
    print(e.value)
