"""The multi-resolution STFT distances on the GPU (tts_stft_pair_sums, tts_torch_stft_mag,
tts_amd.vocoder_losses, tts_amd.vocoder_eval) against the reference in float64
(tests/golden/vocoder_eval.npz, written by tests/golden/make_vocoder_eval_golden.py).

Yardstick: the float64 fixture; a quantity of value v may differ from it by at most
8 x max(the reference's own float32-vs-float64 deviation for it, 2^-23 |v|); for a tensor the
deviation is the largest over the tensor and |v| its largest magnitude
(vocoder_eval_cases.tolerance). Every error is printed next to its tolerance before it is asserted.
"""
import numpy as np
import pytest
import torch

import vocoder_eval_cases as vc
from helpers import build_melgan, load_fixture, melgan_state_dict

pytestmark = pytest.mark.gpu

IDS = [f"{n}-{h}-{w}" for n, h, w in vc.RESOLUTIONS]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture("vocoder_eval")


def _batch(pairs, fill=1e3):
    """(y_hat, y) device batches of the float32 row pairs, the caller's padding filled with `fill`."""
    dev = _dev()
    L = max(len(p[0]) for p in pairs)
    out = []
    for k in range(2):
        a = np.full((len(pairs), L), fill, np.float32)
        for b, p in enumerate(pairs):
            a[b, :len(p[k])] = p[k]
        out.append(torch.from_numpy(a).to(dev))
    return out[0], out[1], [len(p[0]) for p in pairs]


def _ragged(i):
    n_fft, hop, win = vc.RESOLUTIONS[i]
    return [vc.pair(s, n) for s, n in zip(vc.resolution_seeds(i)[0], vc.resolution_lengths(n_fft, hop))]


def _close(name, got, ref, dev32):
    """Every entry of got against ref, each with the tolerance of its own value and deviation."""
    got, ref, dev32 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, ref, dev32))
    assert got.shape == ref.shape == dev32.shape, (name, got.shape, ref.shape)
    ok = True
    for g, r, d in zip(got.ravel(), ref.ravel(), dev32.ravel()):
        tol = vc.tolerance(d, r)
        print(f"{name}: gpu {g:.9f} float64 {r:.9f} err {abs(g - r):.3e} tol {tol:.3e} (reference float32 dev {d:.3e})")
        ok = ok and abs(g - r) <= tol
    assert ok, name


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_torch_stft_magnitudes(fx, i):
    """TorchSTFT on the ragged batch: shape (B, n_fft // 2 + 1, frames) by torch.stft's frame formula,
    odd n_fft included, rows zero past their own frames, values against the stored slices."""
    from tts_amd import TorchSTFT
    n_fft, hop, win = vc.RESOLUTIONS[i]
    pairs = _ragged(i)
    _, y, lens = _batch(pairs)
    frames = [1 + (n // hop if n_fft % 2 == 0 else (n - 1) // hop) for n in lens]
    assert frames == [vc.stft_frames(n, n_fft, hop) for n in lens]
    mag = TorchSTFT(n_fft, hop, win)(y, lengths=lens)
    assert mag.shape == (3, n_fft // 2 + 1, max(frames)) and mag.dtype == torch.float32
    mag = mag.cpu().numpy()
    assert np.isfinite(mag).all()
    for b in range(3):
        assert (mag[b, :, frames[b]:] == 0).all(), b
        assert (mag[b, :, :frames[b]] >= 1e-4 * (1 - 1e-6)).all(), b
    sel = [0, 1, frames[2] - 2, frames[2] - 1]
    for name, got, ref, d in (("row 0", mag[0, :, :frames[0]], fx[f"r{i}_mag0"], fx[f"r{i}_mag_dev"][0]),
                              ("row 2 end frames", mag[2][:, sel], fx[f"r{i}_mag2"], fx[f"r{i}_mag_dev"][1])):
        assert got.shape == ref.shape, (got.shape, ref.shape)
        err, tol = np.abs(got - ref).max(), vc.tolerance(d, ref)
        print(f"TorchSTFT {IDS[i]} {name}: err {err:.3e} tol {tol:.3e} (reference float32 dev {d:.3e}, "
              f"peak {ref.max():.3f})")
        assert err <= tol
    single = TorchSTFT(n_fft, hop, win)(y[2:3, :lens[2]])  # no lengths: the reference's call
    assert single.shape == (1, n_fft // 2 + 1, frames[2])
    assert np.array_equal(single[0].cpu().numpy(), mag[2, :, :frames[2]])


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_stft_loss_rows_pool_and_batch(fx, i):
    """STFTLoss of one resolution: per-row and pooled values of the ragged batch, the equal-length
    batch against the reference's batch call, and every row alone bit-identical to itself in the batch."""
    from tts_amd import STFTLoss
    n_fft, hop, win = vc.RESOLUTIONS[i]
    loss = STFTLoss(n_fft, hop, win)
    y_hat, y, lens = _batch(_ragged(i))
    mg, sc = loss(y_hat, y, lengths=lens, per_row=True)
    assert mg.shape == sc.shape == (3,) and mg.dtype == torch.float32 and mg.device.type == "cuda"
    _close(f"STFTLoss {IDS[i]} rows", torch.stack([mg, sc], 1).cpu().numpy(), fx[f"r{i}_row"], fx[f"r{i}_row_dev"])
    pmg, psc = loss(y_hat, y, lengths=lens)
    assert pmg.shape == psc.shape == ()
    _close(f"STFTLoss {IDS[i]} pooled", [float(pmg), float(psc)], fx[f"r{i}_pool"], fx[f"r{i}_pool_dev"])
    sums, counts = loss.row_sums(y_hat, y, lens)
    assert sums.dtype == torch.float64 and sums.shape == (3, 3)
    for b, n in enumerate(lens):
        alone, c1 = loss.row_sums(y_hat[b:b + 1, :n], y[b:b + 1, :n])
        assert torch.equal(alone[0], sums[b]) and c1[0] == counts[b], b
        one = loss(y_hat[b:b + 1, :n], y[b:b + 1, :n])  # the reference's call on the cut row
        assert float(one[0]) == float(mg[b]) and float(one[1]) == float(sc[b]), b
    eq = [vc.pair(s, lens[1]) for s in vc.resolution_seeds(i)[1]]
    yh_eq, y_eq, _ = _batch(eq)
    emg, esc = loss(yh_eq, y_eq)
    _close(f"STFTLoss {IDS[i]} equal-length batch", [float(emg), float(esc)], fx[f"r{i}_equal"], fx[f"r{i}_equal_dev"])


def test_bins_on_the_clamp(fx):
    """A quiet pair at 171 / 10 / 60 whose noise floor lies under the 1e-8 clamp (about half of the
    bins sit on it) and whose sines lie above."""
    from tts_amd import STFTLoss
    assert 0.2 < float(fx["clamp_share"]) < 0.8
    y_hat, y = (vc.CLAMP_GAIN * a for a in vc.pair(vc.CLAMP_SEED, vc.CLAMP_LENGTH))
    yh, yy, _ = _batch([(y_hat, y)])
    mg, sc = STFTLoss(*vc.CLAMP_RESOLUTION)(yh, yy)
    _close("STFTLoss on the clamp", [float(mg), float(sc)], fx["clamp_row"], fx["clamp_row_dev"])


def test_multi_scale_classes(fx):
    from tts_amd import MultiScaleSTFTLoss, MultiScaleSubbandSTFTLoss
    dev = _dev()
    y_hat, y = (torch.from_numpy(a.reshape(2, 4096)).to(dev) for a in vc.pair(vc.MULTI_FULL_SEED, 2 * 4096))
    mg, sc = MultiScaleSTFTLoss()(y_hat, y)
    assert mg.shape == sc.shape == () and mg.dtype == torch.float32
    _close("MultiScaleSTFTLoss", [float(mg), float(sc)], fx["multi_full"], fx["multi_full_dev"])
    n_ffts, hops, wins = (list(c) for c in zip(*vc.SUBBAND))
    sub = MultiScaleSubbandSTFTLoss(n_ffts, hops, wins)
    y_hat, y = (torch.from_numpy(a.reshape(2, 4, 1024)).to(dev) for a in vc.pair(vc.MULTI_SUB_SEED, 2 * 4 * 1024))
    mg, sc = sub(y_hat, y)
    _close("MultiScaleSubbandSTFTLoss", [float(mg), float(sc)], fx["multi_sub"], fx["multi_sub_dev"])
    # per utterance: its own (1, C, L) call; lengths apply to all the bands of an utterance
    rmg, rsc = sub(y_hat, y, per_row=True)
    assert rmg.shape == (2,)
    for b in range(2):
        one = sub(y_hat[b:b + 1], y[b:b + 1])
        assert float(one[0]) == float(rmg[b]) and float(one[1]) == float(rsc[b])
    cut = sub(y_hat, y, lengths=[1024, 700], per_row=True)
    one = sub(y_hat[1:2, :, :700], y[1:2, :, :700])
    assert float(cut[0][0]) == float(rmg[0]) and float(cut[0][1]) == float(one[0]) and float(cut[1][1]) == float(one[1])


def test_more_rows_than_one_library_call():
    """70 rows go to the library in two calls; every row still equals its own call."""
    from tts_amd import STFTLoss
    loss = STFTLoss(64, 16, 32)
    pairs = [vc.pair(50 + (b % 3), 40 + (b % 5)) for b in range(70)]
    y_hat, y, lens = _batch(pairs)
    mg, sc = loss(y_hat, y, lengths=lens, per_row=True)
    assert mg.shape == (70,)
    for b in (0, 63, 64, 69):
        one = loss(y_hat[b:b + 1, :lens[b]], y[b:b + 1, :lens[b]])
        assert float(one[0]) == float(mg[b]) and float(one[1]) == float(sc[b]), b


def test_digital_silence_is_exactly_zero():
    """Both sides silent: every bin clamps to 1e-4 on both sides, so both distances are exactly 0."""
    from tts_amd import MultiScaleSTFTLoss, TorchSTFT
    dev = _dev()
    z = torch.zeros(2, 4096, device=dev)
    mg, sc = MultiScaleSTFTLoss()(z, z.clone())
    assert float(mg) == 0.0 and float(sc) == 0.0
    mag = TorchSTFT(171, 10, 60)(z[:, :340])
    assert float(mag.min()) == float(mag.max()) and abs(float(mag.max()) - 1e-4) <= 2 * 2.0 ** -37  # 2 float32 steps


def test_short_row_raises_and_leaves_the_context_usable(fx):
    from tts_amd import STFTLoss, TorchSTFT
    from tts_amd._lib import get_engine
    dev = _dev()
    i = 4  # 683 / 60 / 300
    n_fft, hop, win = vc.RESOLUTIONS[i]
    loss = STFTLoss(n_fft, hop, win)
    y_hat, y, lens = _batch(_ragged(i))
    bad = [lens[0], n_fft // 2, lens[2]]
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        loss(y_hat, y, lengths=bad)
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        TorchSTFT(n_fft, hop, win)(y[:, :n_fft // 2])
    sums = torch.full((3, 3), 7.0, device=dev, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Padding size should be less than") as e:  # the library's own check
        get_engine(dev).stft_pair_sums(y_hat, y, bad, n_fft, win, hop, sums)
    print(e.value)
    torch.cuda.synchronize()
    assert (sums == 7.0).all()
    mg, sc = loss(y_hat, y, lengths=lens, per_row=True)
    _close("STFTLoss after the error", torch.stack([mg, sc], 1).cpu().numpy(), fx[f"r{i}_row"], fx[f"r{i}_row_dev"])


@pytest.mark.parametrize("bad,match", [(dict(n_fft=2049), "n_fft"), (dict(win_length=1025), "win_length"),
                                       (dict(hop_length=0), "hop_length"),
                                       (dict(win_length=15, n_fft=16), "win_length"), (dict(rows=65), "B <= 64")])
def test_abi_fences_name_the_argument(bad, match):
    from tts_amd._lib import get_engine
    dev = _dev()
    kw = dict(n_fft=1024, win_length=600, hop_length=120, rows=2)
    kw.update(bad)
    B = kw.pop("rows")
    y = torch.zeros(B, 4096, device=dev)
    sums = torch.full((B, 3), 7.0, device=dev, dtype=torch.float64)
    mag = torch.full((B, kw["n_fft"] // 2 + 1, 40), 7.0, device=dev)
    eng = get_engine(dev)
    with pytest.raises(RuntimeError, match="stft_pair_sums.*" + match) as e:
        eng.stft_pair_sums(y, y, [4096] * B, kw["n_fft"], kw["win_length"], kw["hop_length"], sums)
    print(e.value)
    with pytest.raises(RuntimeError, match="torch_stft_mag.*" + match):
        eng.torch_stft_mag(y, [4096] * B, kw["n_fft"], kw["win_length"], kw["hop_length"], mag)
    torch.cuda.synchronize()
    assert (sums == 7.0).all() and (mag == 7.0).all()


def test_python_fences_name_the_argument():
    from tts_amd import MultiScaleSTFTLoss, STFTLoss, TorchSTFT
    _dev()
    with pytest.raises(NotImplementedError, match="n_fft"):
        STFTLoss(2049, 120, 600)
    with pytest.raises(NotImplementedError, match="win_length"):
        MultiScaleSTFTLoss((1024,), (120,), (1025,))
    with pytest.raises(ValueError, match="hop_length"):
        TorchSTFT(1024, 0, 600)
    with pytest.raises(NotImplementedError, match="window"):
        TorchSTFT(1024, 120, 600, window="hamming_window")


# ------------------------------------------------------------------------------ copy synthesis
LJ_AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0,
                ref_level_db=20, power=1.5, griffin_lim_iters=30, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0,
                spec_gain=1, signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0,
                clip_norm=True)


def test_copy_synthesis_scores_equal_the_public_calls():
    """copy_synthesis_scores on a small MB-MelGAN (the mbmelgan fixture's weights), two rows of about
    0.2 s: its eight values equal the same quantities assembled from melspectrogram_batch, inference,
    generator, analysis and the loss classes."""
    from tts_amd import MultiScaleSTFTLoss, MultiScaleSubbandSTFTLoss, copy_synthesis_scores
    from tts_amd.audio import AudioProcessor
    from tts_amd.vocoder_eval import SUBBAND_STFT_LOSS_PARAMS
    dev = _dev()
    cfg, sd = melgan_state_dict(int(load_fixture("mbmelgan")["seed"]))
    v = build_melgan(cfg, sd, dev)
    ap = AudioProcessor(**LJ_AUDIO, analysis_device="gpu")
    lens = [4410, 3901]
    wavs = np.zeros((2, 4410), np.float32)
    for b, n in enumerate(lens):
        wavs[b, :n] = vc.signal(400 + b, n)
    wavs = torch.from_numpy(wavs).to(dev)
    v.inference_padding = 2
    with pytest.raises(ValueError, match="inference_padding"):
        copy_synthesis_scores(v, ap, wavs, lens)
    v.inference_padding = 0
    scores = copy_synthesis_scores(v, ap, wavs, lens)
    assert sorted(scores) == sorted(f"G_{k}_{q}{s}" for k in ("stft_loss", "subband_stft_loss") for q in ("mg", "sc")
                                    for s in ("", "_rows"))

    mel, frames = ap.melspectrogram_batch(wavs, lens)
    assert frames == [18, 16]
    mel = mel.transpose(1, 2)
    y_hat = v.inference(mel, lengths=frames)[:, 0, :4410]
    full = MultiScaleSTFTLoss()
    want = {}
    for s, per_row in (("", False), ("_rows", True)):
        want["G_stft_loss_mg" + s], want["G_stft_loss_sc" + s] = full(y_hat, wavs, lengths=lens, per_row=per_row)
    bands_hat = v.generator(mel, lengths=frames)
    bands = v.pqmf_layer.analysis(wavs[:, None, :], lengths=lens)
    sub_lens = [min(64 * m, (n - 1) // 4 + 1) for m, n in zip(frames, lens)]
    assert sub_lens == [1103, 976]
    Ls = min(bands_hat.shape[2], bands.shape[2])
    sub = MultiScaleSubbandSTFTLoss(**SUBBAND_STFT_LOSS_PARAMS)
    for s, per_row in (("", False), ("_rows", True)):
        want["G_subband_stft_loss_mg" + s], want["G_subband_stft_loss_sc" + s] = sub(
            bands_hat[:, :, :Ls], bands[:, :, :Ls], lengths=sub_lens, per_row=per_row)
    for k in sorted(want):
        print(k, scores[k])
        assert scores[k] == want[k].cpu().tolist(), k
        assert np.isfinite(scores[k]).all() and np.all(np.asarray(scores[k]) > 0), k
    assert isinstance(scores["G_stft_loss_mg"], float) and len(scores["G_stft_loss_mg_rows"]) == 2
